/* libapk - C-ABI of the MI355X-native PLONK prover path for AlgoPlonk.
 *
 * Drop-in boundary.  The reference has no FFI of its own: the hot path is the Go call
 *     proof, err := plonk.Prove(cc.Ccs, cc.Pk, witness)         /root/reference/algoplonk.go:89
 * (second call site /root/reference/testutils/testutils.go:47) and the one-time
 *     plonk.Setup(ccs, srs, lagrangeSrs)                         /root/reference/setup/setup.go:107,149
 * A cgo shim replaces those calls with the entry points below.  Every buffer uses
 * gnark's in-memory layout so the shim passes unsafe.Pointer(&slice[0]) with zero copies:
 *   - Fr / Fp element : little-endian limbs, Montgomery form (gnark-crypto fr.Element / fp.Element);
 *                       32 bytes for Fr (both curves), 32 (BN254) / 48 (BLS12-381) bytes for Fp
 *   - G1 affine       : X || Y, each an Fp element as above; (0,0) is the point at infinity
 * No torch types, no C++ types: plain pointers and sizes.  All functions return APK_OK (0) or an error
 * code; apk_last_error() gives the message for the calling thread.  Nothing panics or aborts across the
 * boundary (the reference wraps errors with fmt.Errorf, algoplonk.go:90-92).
 *
 * There is NO CPU fallback: every compute entry point fails with APK_ERR_HIP when no gfx950 device is
 * usable.  The oracle under oracle/ is test infrastructure and is never linked into this library.
 *
 * Runtime environment: a context runs up to 16 HIP streams at a time - one proof each, or (circuits up to 2^16, more callers
 * than streams) a gang of two to four proofs that share a stream and its launches.  ROCm maps streams onto
 * GPU_MAX_HW_QUEUES hardware queues (default 4), read ONCE when the HIP runtime initialises; with 4 the streams serialise
 * (measured table: CHANGELOG "Hardware queues", profiles/hw_queues_ab.txt).  The library needs 16: a queue per proving stream.
 * When it is LOADED it therefore RAISES GPU_MAX_HW_QUEUES to 16: a value already in the environment that is at least 16
 * stays as the host set it; a lower one, a missing or an unreadable one (anything but decimal digits) becomes 16.  A host that
 * exported a value from 4 to 15 on purpose - a machine that exports the default of 4 has "set" it too - is therefore
 * OVERRIDDEN, silently but for apk_runtime_read (below), which reports what was found and what was left; such a host says
 * APK_HW_QUEUES=0, which leaves the environment exactly as found.  APK_HW_QUEUES = 4 .. 32 sets the need instead of 16.  The
 * library writes no value below 4 or above 32, and writes the variable nowhere else.
 * The trade-off behind 16: under load 16, 20, 24 and 32 queues give the same proofs/s (+5 % over 4 queues at BN254 2^17), but a
 * LONE proof takes 3.6 ms with 20 or more queues against 3.2 ms with 4, 8 or 16 (the parent build shows the same with the
 * variable set by hand: it is the queue count).  A host that sets 24 or 32 itself keeps its value and pays that.
 * A host process that initialises HIP BEFORE loading libapk (another GPU library, torch ...) must export
 * GPU_MAX_HW_QUEUES=16 itself before its first HIP call - by then the runtime no longer reads the variable, whatever the
 * library writes; such a host may say so with APK_HW_QUEUES=0.  The cgo shim of INTEGRATION.md loads libapk at program start,
 * so a plain AlgoPlonk process needs nothing.
 * With fewer queues than proving streams (APK_HW_QUEUES=0 on 4 queues, or HIP initialised earlier) leave the other defaults
 * alone: no stream budget (APK_MAX_SLOTS) or gang size (APK_GANG) measured there beats the 16 lone streams beyond the noise.
 */
#ifndef APK_H
#define APK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APK_ABI_VERSION 5

/* curve ids: the two curves the AVM supports (algoplonk.go:39-41) */
#define APK_BN254 0
#define APK_BLS12_381 1

#define APK_OK 0
#define APK_ERR_ARG 1      /* bad argument (unknown curve, n not a power of two, null pointer ...) */
#define APK_ERR_HIP 2      /* HIP runtime failure, including "no device" */
#define APK_ERR_STATE 3    /* call not valid for this context (e.g. Lagrange MSM without a Lagrange SRS) */
#define APK_ERR_WITNESS 4  /* the witness does not satisfy the circuit (quotient not a polynomial) */
#define APK_ERR_VERIFY 5   /* apk_verify: the proof does not verify against the key and public inputs */

#define APK_FR_BYTES 32
#define APK_G1_MAX_BYTES 96       /* BLS12-381 affine; BN254 uses the first 64 bytes of a slot */
#define APK_G2_MAX_BYTES 192      /* G2 affine, gnark in-memory: X.A0 || X.A1 || Y.A0 || Y.A1; BN254 uses the first 128 bytes */
#define APK_MAX_COMMITMENTS 2     /* BSB22 commitments per circuit (reference documents 0/1/2: README.md:27-30) */
#define APK_NB_BLINDING 9         /* bl0,bl1, br0,br1, bo0,bo1, bz0,bz1,bz2 */

typedef struct apk_ctx apk_ctx;

const char* apk_last_error(void);
int apk_abi_version(void);
/* number of visible HIP devices (0 and APK_OK when the runtime loads but no GPU is present) */
int apk_device_count(int* count);
/* bytes of one G1 affine point / one Fp element for a curve id; 0 for an unknown id */
size_t apk_g1_bytes(int curve);
size_t apk_fp_bytes(int curve);

/* ---- circuit context: replaces plonk.Setup's output + the per-proof trace rebuild ----------------------
 * One context per (device, curve, circuit).  It owns, resident in HBM: the KZG SRS with its windowed point
 * tables, the trace polynomials (Lagrange, canonical and 4n-coset forms), the permutation polynomials, the NTT
 * twiddles and `slots` independent proving workspaces.  Inputs are copied; the caller keeps ownership
 * (SURVEY.md §8b "nothing is retained by the callee").
 */
typedef struct {
    int curve;                 /* APK_BN254 / APK_BLS12_381 */
    int device;                /* HIP device ordinal */
    uint64_t n;                /* domain size: NextPowerOfTwo(nbConstraints + nbPublic), >= 8 (setup/setup.go:113-114) */
    uint32_t nb_public;        /* VK NbPublicVariables */
    uint32_t nb_commitments;   /* BSB22 commitments (<= APK_MAX_COMMITMENTS) */
    const void* srs_g1;        /* n+3 G1 affine: canonical SRS  = gnark kzg.ProvingKey.G1 (setup/setup.go:113-114) */
    const void* srs_g1_lagrange; /* n G1 affine: Lagrange SRS = gnark's ProvingKey.KzgLagrange (setup/setup.go:124,138), or NULL: the
                                  * context then derives it from srs_g1 on the device (kzg.ToLagrangeG1) unless APK_WIRES_LAGRANGE=0
                                  * and nb_commitments == 0.  It serves the BSB22 commitments and - round 5 - [L][R][O], which gnark
                                  * commits over this basis: the scalars are then the witness values themselves (mostly 0 / 1 / small
                                  * in real circuits: few non-zero digits).  APK_WIRES_LAGRANGE (read at apk_ctx_create): -1 = the
                                  * context decides per proof from the wires' non-zero digits (default), 0 = always the canonical
                                  * SRS (rounds 1-4), 1 = always the Lagrange SRS.  Same group elements, same proof bytes. */
    const void* ql;            /* trace columns in Lagrange form, n Fr each  = gnark plonk.Trace{Ql,Qr,Qm,Qo,Qk} */
    const void* qr;
    const void* qm;
    const void* qo;
    const void* qk;            /* public rows zero */
    const int64_t* perm;       /* 3n entries = gnark Trace.S */
    const void* qcp[APK_MAX_COMMITMENTS];               /* n Fr each */
    uint32_t commitment_constraint_index[APK_MAX_COMMITMENTS]; /* VK CommitmentConstraintIndexes */
    int msm_window;            /* signed-digit window bits (7..20; 18..20 = 2^17..2^19 buckets, two-level sort only: needs
                                * bases x windows < 2^(31 - partition bits)); 0 = choose from n and slots */
    int slots;                 /* concurrent proofs in flight on this context; 0 = 1; at most APK_MAX_SLOTS (16) proving streams run at a
                                * time on the DEVICE, over all its contexts: more callers wait their turn or, on small circuits, share a stream */
} apk_circuit_desc;

int apk_ctx_create(const apk_circuit_desc* desc, apk_ctx** out);
/* the window width the context chose (msm_window = 0) or was given; 0 for a null context */
int apk_ctx_msm_window(apk_ctx* ctx);
void apk_ctx_destroy(apk_ctx* ctx);
/* MSM-only context over an arbitrary base set (`count` G1 affine, host memory): windowed tables + one MSM
 * workspace, no circuit.  Used to shard ONE large MSM by index range across GPUs (BASELINE.json configs[3]):
 * each rank builds a context over its slice of the SRS, runs apk_msm_g1 on its slice of the scalars, and the
 * partial sums (one point per rank) are all-gathered and added (algoplonk_amd/parallel.py).  apk_msm_g1* with
 * basis 0 and the device-memory helpers work on it; apk_prove / apk_ntt / apk_ctx_get_vk return APK_ERR_STATE.
 * The bases must lie in the prime-order subgroup (every KZG SRS does): the tables hold R^-1 * P_i so that Montgomery-form scalars
 * are used as they arrive, and (a R)(R^-1 P) = a P holds only for points of order r.  BN254's G1 has cofactor 1; an on-curve
 * BLS12-381 point outside the subgroup gives a different sum than gnark's MultiExp (not checked: a subgroup test per base would
 * double the table build). */
int apk_msm_ctx_create(int curve, int device, const void* bases, uint64_t count, int msm_window, apk_ctx** out);

/* Verifying-key commitments produced during context creation (the 8+k MSMs of plonk.Setup).
 * Each slot is APK_G1_MAX_BYTES wide, gnark in-memory affine form. Order: Ql,Qr,Qm,Qo,Qk,S1,S2,S3,Qcp_0.. */
typedef struct {
    uint8_t ql[APK_G1_MAX_BYTES], qr[APK_G1_MAX_BYTES], qm[APK_G1_MAX_BYTES], qo[APK_G1_MAX_BYTES], qk[APK_G1_MAX_BYTES];
    uint8_t s[3][APK_G1_MAX_BYTES];
    uint8_t qcp[APK_MAX_COMMITMENTS][APK_G1_MAX_BYTES];
    uint8_t size_inv[APK_FR_BYTES], generator[APK_FR_BYTES], coset_shift[APK_FR_BYTES]; /* Fr, Montgomery */
} apk_vk;
int apk_ctx_get_vk(apk_ctx* ctx, apk_vk* out);

/* ---- primitives (row a4 / a6 of SURVEY.md §8a) --------------------------------------------------------- */
/* kzg.Commit: sum scalars[i] * SRS[i].  basis 0 = canonical SRS (len <= n+3), 1 = Lagrange SRS (len <= n; the context's table
 * continues with the three blinding points [tau^(n+k)]G1 - [tau^k]G1 at indices n..n+2, so len <= n+3 is accepted).
 * scalars: host memory, `len` Fr in Montgomery form.  out: one G1 affine (apk_g1_bytes). */
int apk_msm_g1(apk_ctx* ctx, int basis, const void* scalars, uint64_t len, void* out);
/* same, scalars already resident in device memory (what bench.py times: inputs in HBM) */
int apk_msm_g1_device(apk_ctx* ctx, int basis, const void* d_scalars, uint64_t len, void* out);
/* `count` (<= 4) partial commitments in one launch sequence: out[b] = sum_{i < lens[b]} d_scalars[b][i] * SRS[offsets[b] + i].
 * The building block of an MSM split by index range over GPUs that each hold the whole SRS (algoplonk_amd/parallel.py
 * SplitCommitter): a rank commits the slices it was dealt, the partial sums are all-gathered and added (apk_g1_sum). */
int apk_msm_g1_batch_device(apk_ctx* ctx, int basis, uint32_t count, const void* const* d_scalars, const uint64_t* offsets,
                            const uint64_t* lens, void* out);
/* fft.Domain.FFT / FFTInverse on the context's size-n (which=0) or size-4n (which=1) domain, natural order in
 * and out; coset != 0 evaluates on / interpolates from the coset CosetShift * <omega>.  data: host, in place.
 * coset = 2 (forward only, a test seam): the form the prover hands to its quotient kernel - the same residues, each word only
 * below 2r instead of canonical. */
int apk_ntt(apk_ctx* ctx, int which, int inverse, int coset, void* data);

/* ---- KZG openings (row a9 of SURVEY.md §8a: gnark-crypto's kzg.Open / BatchOpenSinglePoint / Verify / BatchVerifySinglePoint) ----
 * The opening calls work on circuit contexts and on MSM-only contexts, over the canonical SRS (basis 0).  Polynomials are
 * coefficient vectors, Fr Montgomery; the point, the values and gamma are one Fr each; H and the digests are G1 affine
 * (apk_g1_bytes).  Any length, any point (on the domain, 0, a root of the polynomial ...): kernels_kzg.h keeps no table of
 * powers.  A call takes a proving slot like apk_msm_g1_device and never joins a gang.  There is no CPU fallback: the checks run
 * in the order  arguments other than the context (APK_ERR_ARG) - a usable HIP device (APK_ERR_HIP) - the context and the length
 * against its SRS (APK_ERR_ARG). */
#define APK_KZG_MAX_POLYS 32
typedef struct {
    int curve;
    uint8_t g1[APK_G1_MAX_BYTES];        /* SRS G1[0] */
    uint8_t g2[2][APK_G2_MAX_BYTES];     /* ([1]G2, [tau]G2), gnark in-memory G2Affine */
} apk_kzg_vk;
/* kzg.Open: H = [(f - f(z)) / (X - z)], value = f(z).  1 <= len <= n + 3 (MSM-only context: <= its base count).
 * One chain of launches, no host synchronisation before the result. */
int apk_kzg_open(apk_ctx* ctx, const void* poly /* host */, uint64_t len, const void* point_fr, void* out_h, void* out_value);
int apk_kzg_open_device(apk_ctx* ctx, const void* d_poly, uint64_t len, const void* point_fr, void* out_h, void* out_value);
/* kzg.BatchOpenSinglePoint: out_values[i] = f_i(z); gamma = sha256("gamma" || z || digests || values || extra) mod r (points X || Y
 * big-endian with the transcript's infinity encodings, scalars canonical big-endian); H = [(g - g(z)) / (X - z)] of the fold
 * g = sum gamma^i f_i.  1 <= count <= APK_KZG_MAX_POLYS, each lens[i] as for apk_kzg_open.  digests: `count` G1 affine (host), or
 * NULL: the call commits each polynomial first (one MSM batch per <= 4).  out_gamma may be NULL.  One host synchronisation
 * between the evaluations and the fold (gamma hashes the values). */
int apk_kzg_batch_open_device(apk_ctx* ctx, uint32_t count, const void* const* d_polys, const uint64_t* lens, const void* digests,
                              const void* point_fr, const uint8_t* extra, size_t extra_len,
                              void* out_h, void* out_values, void* out_gamma);
int apk_kzg_batch_open(apk_ctx* ctx, uint32_t count, const void* const* polys /* host */, const uint64_t* lens, const void* digests,
                       const void* point_fr, const uint8_t* extra, size_t extra_len,
                       void* out_h, void* out_values, void* out_gamma);
/* Host only, no GPU.  kzg.Verify: e(digest - value G1 + z H, G2_0) e(-H, G2_1) == 1, after on-curve and subgroup checks of digest and
 * H.  kzg.BatchVerifySinglePoint: the same on the fold of `count` digests and values under the challenge above.
 * APK_OK / APK_ERR_VERIFY / APK_ERR_ARG (bad key, a scalar not below r, count out of range). */
int apk_kzg_verify(const apk_kzg_vk* vk, const void* digest, const void* point_fr, const void* value_fr, const void* h);
int apk_kzg_batch_verify(const apk_kzg_vk* vk, uint32_t count, const void* digests, const void* values, const void* point_fr,
                         const uint8_t* extra, size_t extra_len, const void* h);
/* the fold challenge by itself (host only): digests / values as above; out_gamma = one Fr Montgomery */
int apk_kzg_fold_challenge(int curve, uint32_t count, const void* digests, const void* values, const void* point_fr,
                           const uint8_t* extra, size_t extra_len, void* out_gamma);
/* `count` independent openings: out_h[i] = [(f_i - f_i(z_i)) / (X - z_i)], out_values[i] = f_i(z_i).  1 <= count <= APK_KZG_MAX_POLYS;
 * each lens[i] as for apk_kzg_open; polys[i] may repeat (one polynomial at several points: a host vector is staged once);
 * points: count Fr.  The bytes are those of apk_kzg_open on every pair.  The openings go through in call order, in groups of up
 * to four (as many MSMs as the context's workspace takes in one batch): per group three launches over its rows, ONE MSM batch
 * over its quotients and one host synchronisation.  A constant (lens[i] == 1) has H = infinity and is no operand of the batch. */
int apk_kzg_open_multi(apk_ctx* ctx, uint32_t count, const void* const* polys /* host */, const uint64_t* lens,
                       const void* points, void* out_h, void* out_values);
int apk_kzg_open_multi_device(apk_ctx* ctx, uint32_t count, const void* const* d_polys, const uint64_t* lens,
                              const void* points, void* out_h, void* out_values);
/* kzg.BatchVerifyMultiPoints: ONE pairing check for `count` openings (digests[i], points[i], values[i], hs[i]), 1 <= count <=
 * APK_KZG_MAX_POLYS.  device -1 folds on the host, >= 0 on that GPU.  gnark draws the fold's weights at random; here
 * lambda_0 = 1 and lambda_j = the low 128 bits of sha256("apk-kzg-multi" || D || be32(j)), D = sha256(be32(curve) || g1 || g2[0] ||
 * g2[1] || be32(count) || per opening: digest, point, value, H) - G1 points X || Y big-endian with the transcript's infinity
 * encodings, scalars canonical big-endian, the G2 points as they lie in the key - so that a verdict can be reproduced.
 * e(sum lambda_i digest_i + sum lambda_i z_i H_i - (sum lambda_i v_i) G1, G2_0) e(-sum lambda_i H_i, G2_1) == 1 after the checks of
 * apk_kzg_verify on every digest, H and scalar; count == 1 is apk_kzg_verify.  One verdict, no per-opening status. */
int apk_kzg_batch_verify_multi(const apk_kzg_vk* vk, int device, uint32_t count, const void* digests, const void* points,
                               const void* values, const void* hs);
/* the fold's weights by themselves (host only): count Fr, Montgomery */
int apk_kzg_multi_weights(const apk_kzg_vk* vk, uint32_t count, const void* digests, const void* points, const void* values,
                          const void* hs, void* out_weights);
/* the opening kernels' lane map (kernels_kzg.h): coefficients per lane, coefficients per workgroup */
int apk_kzg_shape(int* lane_chunk, int* block_span);
/* ---- the same openings in evaluation form: circuit contexts only, over the Lagrange SRS (basis 1) ----
 * The polynomial f of degree < n is given by its n values f(omega^i), natural order - index i belongs to omega^i, the order of
 * srs_g1_lagrange and of apk_ntt - so what apk_msm_g1(basis 1) commits can be opened without a transform: H and the value are the
 * bytes apk_kzg_open returns for the coefficients of f, and apk_kzg_verify / apk_kzg_batch_verify take them against the basis-1
 * commitments as they are.  Any point: off the domain, 0, or omega^m (kernels_kzg_lagrange.h has the formulas).  len must equal
 * the context's n (APK_ERR_ARG); every vector of the batch call has n values.  Checks in the order above: arguments other than
 * the context (APK_ERR_ARG) - a usable HIP device (APK_ERR_HIP, no CPU fallback) - the context: an MSM-only context has no domain
 * (APK_ERR_STATE), and a circuit context whose Lagrange table cannot be had answers as apk_msm_g1 does for basis 1
 * (APK_ERR_STATE).  A call takes a proving slot and never joins a gang.  The single opening has no host synchronisation before
 * the result; the batch call has one, like apk_kzg_batch_open, and with digests = NULL commits each vector over basis 1 first. */
int apk_kzg_open_lagrange(apk_ctx* ctx, const void* evals /* host */, uint64_t len, const void* point_fr, void* out_h, void* out_value);
int apk_kzg_open_lagrange_device(apk_ctx* ctx, const void* d_evals, uint64_t len, const void* point_fr, void* out_h, void* out_value);
int apk_kzg_batch_open_lagrange(apk_ctx* ctx, uint32_t count, const void* const* evals /* host */, const void* digests,
                                const void* point_fr, const uint8_t* extra, size_t extra_len,
                                void* out_h, void* out_values, void* out_gamma);
int apk_kzg_batch_open_lagrange_device(apk_ctx* ctx, uint32_t count, const void* const* d_evals, const void* digests,
                                       const void* point_fr, const uint8_t* extra, size_t extra_len,
                                       void* out_h, void* out_values, void* out_gamma);
/* `count` independent openings in evaluation form: out_h[i] and out_values[i] are what apk_kzg_open_lagrange returns for
 * (evals[i], points[i]), byte for byte - and so the bytes of apk_kzg_open on the coefficients.  1 <= count <= APK_KZG_MAX_POLYS;
 * every evals[i] has the context's n values (there is no length array); evals[i] may repeat (one vector at several points: a
 * host vector is staged once); points: count Fr, each off the domain, 0 or omega^m - rows of both kinds may share a group.  The
 * openings go through in call order, in groups of up to four: per group at most six launches over its rows, ONE MSM batch over
 * the Lagrange SRS whose operands are the rows' quotients (a zero or constant vector reaches infinity through it) and one host
 * synchronisation.  Checks in the order above; a null vector, or in the _device form one that is not device memory, is the
 * context's answer (APK_ERR_ARG, after APK_ERR_STATE for an MSM-only context).  apk_kzg_batch_verify_multi takes the outputs
 * against the basis-1 commitments as they are. */
int apk_kzg_open_multi_lagrange(apk_ctx* ctx, uint32_t count, const void* const* evals /* host */,
                                const void* points, void* out_h, void* out_values);
int apk_kzg_open_multi_lagrange_device(apk_ctx* ctx, uint32_t count, const void* const* d_evals,
                                       const void* points, void* out_h, void* out_values);
/* their kernels' lane map (kernels_kzg_lagrange.h): values per lane, values per workgroup */
int apk_kzg_lagrange_shape(int* lane_chunk, int* block_span);
/* ---- ONE polynomial opened at EVERY point of the domain: circuit contexts only, coefficient form, over the canonical SRS ----
 * The n openings at omega^0 .. omega^(n-1) in one call (Feist - Khovratovich): three transforms in the exponent and 2n scalar
 * multiplications, O(n log n) group operations, instead of n MSMs through apk_kzg_open_multi (kernels_kzg_all.h has the formulas).
 * Polynomials of at most n coefficients: the blinded polynomials of a proof (n + 2, n + 3 coefficients) are OUT OF SCOPE - open
 * those with apk_kzg_open_multi.
 * apk_kzg_all_prepare: the transform of the reversed SRS the calls below need, kept by the context (2n affine points and n
 * twiddle records).  srs_g1: host, `count` >= n - 1 G1 affine: the canonical SRS the context was created with (it is not checked
 * against the context: openings over another SRS do not verify).  Idempotent; safe beside proofs.
 * apk_kzg_open_all*: out_h[i], out_values[i] (host; n G1 affine, n Fr; out_values may be NULL) = what apk_kzg_open(poly, len,
 * omega^i) returns, byte for byte, i = 0 .. n-1 in natural order (the order of apk_ntt and of srs_g1_lagrange).  1 <= len <= n.
 * Checks in the order of the other KZG calls: arguments other than the context (a null pointer, len = 0, count < n - 1:
 * APK_ERR_ARG) - a usable HIP device (APK_ERR_HIP, no CPU fallback) - the context: an MSM-only context, or a call before
 * apk_kzg_all_prepare, is APK_ERR_STATE; len > n is APK_ERR_ARG.  A call takes a proving slot and never joins a gang; the slot's
 * scratch (2n XYZZ points, 3n scalars) is allocated on its first such call.  APK_KZG_ALL_GLV (read at apk_kzg_all_prepare): 1 =
 * the butterflies' twiddles are split in two half-length scalars (default), 0 = full-length twiddles.  Same bytes either way. */
int apk_kzg_all_prepare(apk_ctx* ctx, const void* srs_g1, uint64_t count);
int apk_kzg_open_all(apk_ctx* ctx, const void* poly /* host */, uint64_t len, void* out_h, void* out_values);
int apk_kzg_open_all_device(apk_ctx* ctx, const void* d_poly, uint64_t len, void* out_h, void* out_values);
/* ---- ONE polynomial opened on EVERY COSET of the domain: circuit contexts only, coefficient form, over the canonical SRS ----
 * l = coset_size = 2^k, 2 <= l <= n / 2, n' = n / l.  Coset i < n' holds the l points omega^(i + n' j), j < l, which all satisfy
 * x^l = a_i = omega^(i l).  ONE proof opens the polynomial on all l of them:  H_i = [(f - I_i) / (X^l - a_i)],  I_i = f mod
 * (X^l - a_i), the polynomial of degree < l through the l values.  The n' proofs in one call (Feist - Khovratovich, the
 * multi-point form): transforms in the exponent over 2n' and n' points and 2n fixed-base scalar multiplications arranged as 2n'
 * sums of l terms (kernels_kzg_cosets.h has the formulas) - the sampling form of apk_kzg_open_all, without its size-2n transform.
 * apk_kzg_cosets_prepare: the table the calls below need, kept by the context (8n affine points; the n twiddle records are
 * shared with apk_kzg_all_prepare - either call may come first, or alone - and APK_KZG_ALL_GLV is read by the first).  srs_g1:
 * host, `count` >= n - l G1 affine: the canonical SRS the context was created with (not checked against it).  ONE coset size per
 * context: the same size again is APK_OK and does nothing, another size is APK_ERR_STATE.  Safe beside proofs.
 * apk_kzg_open_cosets*: out_h[i] (host, n' G1 affine) = H_i; out_values (host, n Fr, or NULL) coset-major: out_values[i l + j] =
 * f(omega^(i + n' j)).  1 <= len <= n; with len <= l every H is infinity (zeros) and only the value transform runs.  Checks in the
 * order of the other KZG calls: arguments other than the context (a null pointer, len = 0, a coset size that is no power of two
 * or below 2, count = 0: APK_ERR_ARG) - a usable HIP device (APK_ERR_HIP, no CPU fallback) - the context: an MSM-only context, or
 * a call before apk_kzg_cosets_prepare, is APK_ERR_STATE; len > n, l > n / 2 or count < n - l is APK_ERR_ARG.  A call takes a
 * proving slot and never joins a gang, and has one host synchronisation, at its end; the slot's scratch (2n' XYZZ points, 5n
 * scalars) is allocated on its first such call.
 * apk_kzg_verify_coset: host only, no GPU.  e(digest - [I_i(tau)]G1 + a_i H, G2_0) e(-H, [tau^l]G2) == 1 for coset `index` < n / l
 * of a domain of n points, after the checks of apk_kzg_verify on digest and H: the single-opening check with [tau^l]G2 in place
 * of g2[1], the shifted digest, value 0 and point a_i.  g2_tau_l: [tau^l]G2 in the in-memory form of apk_kzg_vk.g2 (a ceremony
 * SRS has it; apk_g2_mul_generator makes it for a TestOnly SRS).  srs_g1: host, the first coset_size canonical SRS points, for
 * [I_i(tau)]G1.  values: the coset's coset_size values in the order j = 0 .. l-1 (a row of out_values), canonical.  APK_OK /
 * APK_ERR_VERIFY / APK_ERR_ARG (a bad key or g2_tau_l, n or coset_size no power of two or out of range for the field,
 * coset_size > n / 2, index >= n / coset_size, a scalar not below r, a null pointer).
 * OUT OF SCOPE: evaluation-form input; polynomials of more than n coefficients (the blinded polynomials of a proof); several
 * coset sizes on one context; cosets of a size-2n extension of the domain (a polynomial of len <= n / 2 coefficients IS
 * erasure-coded by its n' cells, and apk_kzg_recover_cosets below brings it back from any half of them). */
int apk_kzg_cosets_prepare(apk_ctx* ctx, const void* srs_g1 /* host */, uint64_t count, uint32_t coset_size);
int apk_kzg_open_cosets(apk_ctx* ctx, const void* poly /* host */, uint64_t len, void* out_h, void* out_values);
int apk_kzg_open_cosets_device(apk_ctx* ctx, const void* d_poly, uint64_t len, void* out_h, void* out_values);
int apk_kzg_verify_coset(const apk_kzg_vk* vk, const void* g2_tau_l, const void* srs_g1 /* host, coset_size points */,
                         uint64_t n, uint32_t coset_size, uint64_t index,
                         const void* digest, const void* values /* coset_size Fr */, const void* h);
/* ---- MANY polynomials opened on every coset in ONE call: the producing side for a block's worth of polynomials -------------------
 * A call of apk_kzg_open_cosets spends most of its time in 2 log(2n') - 1 stage launches that each last as long as one butterfly's
 * serial chain, however few lanes they have.  These calls lay up to 16 polynomials side by side in the SAME launches (`count` up to
 * APK_KZG_COSETS_MULTI_MAX runs as cdiv(count, 16) groups of nearly equal size, one after another): the stage launches are paid
 * once per group, the pointwise sums once per polynomial (kernels_kzg_cosets_multi.h).
 * polys: host array of `count` pointers (host memory, or device memory in the _device form), lens[b] coefficients each; the same
 * pointer may occur several times and the lengths may differ.  out_h: host, count x n' G1 affine, polynomial-major: out_h[b n' + i]
 * is the H_i apk_kzg_open_cosets(polys[b], lens[b]) returns.  out_values: host, count x n Fr, or NULL: out_values[b n + i l + j] is
 * that call's out_values[i l + j].  THE BYTES ARE THOSE OF apk_kzg_open_cosets ON EVERY POLYNOMIAL (a row with lens[b] <= l: zeros).
 * After a usable HIP device (APK_ERR_HIP, no CPU fallback) and a non-null context, the rules are checked in this order, the
 * message naming the offending row where there is one: (1) an MSM-only context: APK_ERR_STATE; (2) a call before
 * apk_kzg_cosets_prepare: APK_ERR_STATE; (3) count = 0 or above APK_KZG_COSETS_MULTI_MAX; (4) a null polys, lens, out_h or polys[b];
 * (5) a lens[b] outside 1..n; (6) in the _device form a d_polys[b] that is not device memory: APK_ERR_ARG.  (Behind rule 5, not a rule of the call but a limit
 * of its 32-bit lane indices: a largest group of G polynomials with G n >= 2^32 is APK_ERR_ARG - beyond any domain whose scratch
 * fits a device.)  In the host form a (pointer, length) that occurs several times in a group is uploaded once.  A call takes ONE proving
 * slot and never joins a gang, and has one host synchronisation, at its end; the slot's scratch (3 G n' XYZZ points and 6 G n
 * scalars for its largest group G so far) is allocated on its first such call and grows with G.  The single call, its scratch and
 * its bytes are untouched.
 * OUT OF SCOPE: more than APK_KZG_COSETS_MULTI_MAX polynomials per call; what apk_kzg_open_cosets leaves out; a batched
 * apk_kzg_open_all; a batched recovery. */
#define APK_KZG_COSETS_MULTI_MAX 64
int apk_kzg_open_cosets_multi(apk_ctx* ctx, uint32_t count, const void* const* polys /* host */, const uint64_t* lens, void* out_h,
                              void* out_values);
int apk_kzg_open_cosets_multi_device(apk_ctx* ctx, uint32_t count, const void* const* d_polys, const uint64_t* lens, void* out_h,
                                     void* out_values);
/* ---- MANY coset openings, ONE pairing check: the consuming side of apk_kzg_open_cosets ------------------------------------------
 * A batch has `count` rows, 1 <= count <= APK_KZG_COSETS_MAX_ROWS.  Row k: a commitment digests[digest_of[k]] (1 <= nb_digests <=
 * count), a coset indices[k] < n / l, its l = coset_size values (values: count x l Fr, row-major, canonical - rows of out_values)
 * and its proof hs[k].  Rows may repeat a coset, or a whole (commitment, coset) pair.  With w the domain's generator, a_k =
 * w^(indices[k] l) and s_c = [tau^c]G1 (srs_g1: host, the first l canonical SRS points, as for apk_kzg_verify_coset):
 *     q_c  = sum_k lambda_k w^(-indices[k] c) IDFT_l(values_k)_c          c < l        (apk_kzg_cosets_fold with weights lambda)
 *     A    = sum_d (sum_{k : digest_of[k] = d} lambda_k) C_d - sum_c q_c s_c + sum_k (lambda_k a_k) H_k,    B = sum_k lambda_k H_k
 *     e(A, G2_0) e(-B, [tau^l]G2) == 1
 * A and B are ONE segmented sum (apk_g1_lincomb_segments' path).  The weights are hashed from the statement, so a verdict can be
 * reproduced (apk_kzg_cosets_weights returns them: count Fr; host only):
 *     r_k = sha256(be32(digest_of[k]) || be64(indices[k]) || the row's l values || H_k)
 *     D   = sha256(be32(curve) || g1 || g2[0] || g2_tau_l || be64(n) || be32(l) || be32(nb_digests) || the digests || be32(count) ||
 *                  r_0 .. r_(count-1))       - the encodings of apk_kzg_multi_weights
 *     lambda_0 = 1,  lambda_j = the low 128 bits of sha256("apk-kzg-cosets" || D || be32(j))
 * With count = 1 the verdict is apk_kzg_verify_coset's.  One verdict for the batch, no per-row status.
 * Checks, in this order and before any fold: the arguments (APK_ERR_ARG: a null pointer; n, coset_size no powers of two with 2 <=
 * l <= n / 2 or out of range for the field; count or nb_digests out of range; a bad key or g2_tau_l; a digest_of[k] >= nb_digests;
 * an indices[k] >= n / l; a scalar not below r; an SRS point that is no point of the group), then every digest and every H as a
 * point of the group (APK_ERR_VERIFY; the message says which kind failed).  device = -1: everything on the host threads
 * (APK_VERIFY_THREADS).  device >= 0: the point checks, the fold (kernels_kzg_cosets_fold.h) and the segmented sum run on that GPU
 * - APK_ERR_HIP without one, no CPU fallback - while the hashing, the scalar checks and the pairing stay on the host; for
 * coset_size > 1024 the interpolation runs on the host threads as well, the point checks and the sum stay on the device.
 * apk_kzg_cosets_fold: the primitive underneath, as apk_g1_lincomb_segments is for the sums.  out_coeffs[c] (coset_size Fr) =
 * sum_k weights[k] I_k[c], I_k the interpolant of row k on coset indices[k] (what apk_kzg_verify_coset interpolates); weights:
 * count Fr, canonical.  device = -1 and device >= 0 return the same bytes.  Argument checks (APK_ERR_ARG) come before the device
 * check (APK_ERR_HIP).
 * apk_kzg_cosets_phase_ms: a measurement aid - the milliseconds of the calling thread's last apk_kzg_batch_verify_cosets: [0] key,
 * SRS and scalar checks, [1] point checks, [2] weights (hashing), [3] fold, [4] segmented sum, [5] pairing. */
#define APK_KZG_COSETS_MAX_ROWS (1u << 20)
int apk_kzg_batch_verify_cosets(const apk_kzg_vk* vk, int device, const void* g2_tau_l, const void* srs_g1 /* host, coset_size points */,
                                uint64_t n, uint32_t coset_size, uint32_t nb_digests, const void* digests,
                                uint32_t count, const uint32_t* digest_of, const uint64_t* indices,
                                const void* values /* count x coset_size Fr, row-major */, const void* hs);
int apk_kzg_cosets_weights(const apk_kzg_vk* vk, const void* g2_tau_l, uint64_t n, uint32_t coset_size, uint32_t nb_digests,
                           const void* digests, uint32_t count, const uint32_t* digest_of, const uint64_t* indices,
                           const void* values, const void* hs, void* out_weights);          /* host only */
int apk_kzg_cosets_fold(int curve, int device, uint64_t n, uint32_t coset_size, uint32_t count, const uint64_t* indices,
                        const void* weights, const void* values, void* out_coeffs /* coset_size Fr */);
int apk_kzg_cosets_phase_ms(double* out_ms /* 6 */);
/* ---- the polynomial BACK from any sufficient set of its cells: the middle between apk_kzg_open_cosets and the verifiers ----------
 * A cell is a row of apk_kzg_open_cosets' out_values: the l = coset_size values f(omega^(i + n' j)), j < l, of coset i < n' = n / l,
 * in the same Fr form.  A polynomial of len <= k l coefficients is determined by ANY k of its n' cells.  values: `count` rows of l Fr,
 * row-major, in any order; indices[r] = the coset of row r (host, distinct).  out_poly receives the len coefficients; the existing
 * apk_kzg_open_cosets_device on them gives every missing cell and proof (recover_cells_and_kzg_proofs of the sampling
 * specifications).  With M the m = n' - count missing cosets, a_i = omega^(i l) and g the coset shift of the context's vk:
 *     Z = prod_{i in M} (X^l - a_i);   E = (values scaled by Z on the known cosets, 0 on the missing ones) = (f Z) on the domain;
 *     P = IDFT_n(E) = f Z;   f = P / Z on the coset g <omega>, then back to coefficients          (kernels_kzg_recover.h)
 * three size-n transforms and 2 n' m multiplications for Z.  ANY count rows give a polynomial of fewer than count l coefficients;
 * when one of them at or above len is non-zero the rows are not cells of one polynomial of len coefficients: APK_ERR_VERIFY,
 * decided on the device, and out_poly is not written.  The scalars are taken as apk_kzg_open_cosets takes its coefficients.
 * Circuit contexts only.  NO prepare call and no SRS: any coset size in any call ("one coset size per context" is the opening's
 * rule, not this one's).  Checks in the order of the other KZG calls: arguments other than the context (a null pointer, count = 0,
 * len = 0, a coset size that is no power of two or below 2: APK_ERR_ARG) - a usable HIP device (APK_ERR_HIP, no CPU fallback) - the
 * context: an MSM-only one is APK_ERR_STATE; then APK_ERR_ARG for l > n / 2, count > n', an index >= n', a repeated index, len >
 * count l (too few cells: the message says how many are needed), n' > APK_KZG_RECOVER_MAX_COSETS; the _device form also for values
 * or d_out_poly that are not device memory.  A call takes a proving slot and never joins a gang, and has one host synchronisation,
 * at its end (the context's first call has a second one: it builds the one table the context keeps, n Fr); the slot's scratch
 * (2n + 3n' scalars, 2n' words) is allocated on its first such call and grows with n'.
 * apk_kzg_recover_cosets_host: the same rules and the same result bytes on the calling thread - no context, no GPU; n a power of
 * two in [4, 2^24] (APK_ERR_ARG otherwise, after the context-free checks).  The reference the device form is tested against.
 * OUT OF SCOPE: polynomials of more than n coefficients; recovery from single points instead of whole cosets; n' above the limit
 * (the product for Z is quadratic in n': 2^16 cosets stay below a tenth of a second by instruction count, 2^20 would take many
 * seconds of one kernel); a sub-quadratic vanishing polynomial. */
#define APK_KZG_RECOVER_MAX_COSETS (1u << 16)
int apk_kzg_recover_cosets(apk_ctx* ctx, uint32_t coset_size, uint32_t count, const uint64_t* indices /* host */,
                           const void* values /* host, count x coset_size Fr, row-major */, uint64_t len, void* out_poly /* host, len Fr */);
int apk_kzg_recover_cosets_device(apk_ctx* ctx, uint32_t coset_size, uint32_t count, const uint64_t* indices /* host */,
                                  const void* d_values, uint64_t len, void* d_out_poly /* device, len Fr */);
int apk_kzg_recover_cosets_host(int curve, uint64_t n, uint32_t coset_size, uint32_t count, const uint64_t* indices,
                                const void* values, uint64_t len, void* out_poly);      /* host only, no GPU */

/* ---- the prover: replaces plonk.Prove (algoplonk.go:89) ------------------------------------------------ */
typedef struct {
    uint32_t curve;
    uint32_t nb_commitments;
    uint8_t lro[3][APK_G1_MAX_BYTES];                      /* Proof.LRO */
    uint8_t z[APK_G1_MAX_BYTES];                           /* Proof.Z */
    uint8_t h[3][APK_G1_MAX_BYTES];                        /* Proof.H */
    uint8_t bsb22[APK_MAX_COMMITMENTS][APK_G1_MAX_BYTES];  /* Proof.Bsb22Commitments */
    uint8_t batched_h[APK_G1_MAX_BYTES];                   /* Proof.BatchedProof.H */
    uint8_t claimed_values[6 + APK_MAX_COMMITMENTS][APK_FR_BYTES]; /* Proof.BatchedProof.ClaimedValues: lin,l,r,o,s1,s2,qcp.. */
    uint8_t zshift_h[APK_G1_MAX_BYTES];                    /* Proof.ZShiftedOpening.H */
    uint8_t zshift_value[APK_FR_BYTES];                    /* Proof.ZShiftedOpening.ClaimedValue */
    /* diagnostics (not part of gnark's Proof): the Fiat-Shamir challenges, Fr Montgomery */
    uint8_t gamma[APK_FR_BYTES], beta[APK_FR_BYTES], alpha[APK_FR_BYTES], zeta[APK_FR_BYTES], gamma_kzg[APK_FR_BYTES];
} apk_proof;

/* Inputs (host memory, gnark layout): the solved wire columns L,R,O in Lagrange form (n Fr each) - what gnark's
 * solver leaves in `SparseR1CSSolution{L,R,O}`; the public inputs (nb_public Fr) = fullWitness[:nbPublic];
 * the 9 blinding scalars (APK_NB_BLINDING Fr) that gnark draws from crypto/rand - explicit here so proofs are
 * reproducible; pi2 = BSB22 committed columns (Lagrange, n Fr each, hiding entries placed) or NULL.
 * Blocks the calling thread; safe to call from several threads (each takes a free slot).
 * This is the call the cgo shim makes (algoplonk.go:89 hands plonk.Prove Go slices).  L, R, O (and pi2) travel
 * to the device on a copy stream of their own, started BEFORE the caller queues for a proving slot: with more callers than
 * slots the upload of the next proof runs beside the rounds of the proofs in flight.  The transfer is true asynchronous DMA
 * when the buffers are page-locked - allocate them with apk_host_alloc or register existing ones once with
 * apk_host_register (the shim does, per buffer pool); pageable buffers work too, staged by the HIP runtime on the calling
 * thread.  The buffers must stay unchanged until the call returns. */
int apk_prove(apk_ctx* ctx, const void* L, const void* R, const void* O, const void* public_inputs,
              const void* blinding, const void* const* pi2, apk_proof* out);

/* Variant with L,R,O already resident in device memory (n Fr each). */
int apk_prove_device(apk_ctx* ctx, const void* d_L, const void* d_R, const void* d_O, const void* public_inputs,
                     const void* blinding, const void* const* d_pi2, apk_proof* out);

/* Intra-proof multi-GPU.  With a hook installed, apk_prove* does not run its KZG commitments on
 * the context's own GPU: at each Fiat-Shamir sync point it calls the hook with the batch's scalar vectors (device memory of
 * this context, `lens[b]` Fr each, commitment b = sum d_scalars[b][i] * SRS_basis[i]) and expects `count` G1 affine points
 * (apk_g1_bytes each) in out_points.  The hook deals the work to the other GPUs of the node (algoplonk_amd/parallel.py:
 * scatter of scalar slices over RCCL, apk_msm_g1_batch_device on every rank, all-gather of the partial sums) while this GPU
 * runs the launches the prover queued behind the batch.  Return APK_OK or an error code.  NULL removes the hook. */
typedef int (*apk_commit_hook)(void* user, int basis, uint32_t count, const void* const* d_scalars, const uint32_t* lens, void* out_points);
int apk_ctx_set_commit_hook(apk_ctx* ctx, apk_commit_hook hook, void* user);
/* Same idea for the per-wire transforms of round 1 ("per-wire NTTs batch across the GPUs", BASELINE.json north_star): with a
 * wire hook installed the prover does not run the 4n-coset evaluations of l, r, o itself; it hands the hook the `count` blinded
 * canonical polynomials (device memory of this context, lens[i] Fr) and expects d_evals[i] (4n Fr each, device memory of this
 * context) filled when the hook returns.  apk_coset_ntt_device is what a rank runs on the polynomial it was dealt. */
typedef int (*apk_wire_hook)(void* user, uint32_t count, const void* const* d_canonical, const uint32_t* lens, void* const* d_evals);
int apk_ctx_set_wire_hook(apk_ctx* ctx, apk_wire_hook hook, void* user);
int apk_coset_ntt_device(apk_ctx* ctx, const void* d_canonical, uint64_t len, void* d_evals);
/* Sub-coset split of round 3, for the replicated prover: rank k of `world`
 * (2, 4 or 8) evaluates the wire and permutation polynomials only on the points i = k (mod world) of the 4n coset (a coset of
 * 4n / world points: one transform of that size per polynomial), runs the quotient kernel there and inverse-transforms locally;
 * ONE all-gather of 4n / world field elements per rank - the hook: `d_all` holds world x bytes_per_rank bytes of THIS context's
 * device memory, rank r's part at r * bytes_per_rank, this rank's part filled in; the hook returns with every part filled in -
 * and the last log2(world) butterfly stages on every rank give the quotient's 4n coefficients, bit for bit those of the whole-
 * coset path.  world = 1 or hook = NULL switches it off.  Needs a context whose Qk is completed inside the quotient kernel (the
 * default: at most 6 public inputs + commitments); APK_ERR_STATE otherwise. */
typedef int (*apk_gather_hook)(void* user, void* d_all, size_t bytes_per_rank);
int apk_ctx_set_subcoset(apk_ctx* ctx, int k, int world, apk_gather_hook hook, void* user);

/* ---- multi-GPU behind the boundary: one process per GPU, libapk's own communicator ---------------------
 * The reference's host is Go (algoplonk.go:89): a cgo caller cannot use a Python process group, so the exchange steps of the
 * path live here.  An apk_comm is one rank of `world` cooperating processes.
 *   control plane : a TCP star through rank 0 (rendezvous, headers, the 64/96-byte partial sums, barriers) - apk_comm_create;
 *   data plane    : RCCL over xGMI on libapk's OWN HIP runtime and stream (ncclSend/ncclRecv groups for the scatter of scalar
 *                   slices and the peer copies of polynomials; librccl is dlopen'ed by apk_comm_bind when world > 1, each rank
 *                   owns a different GPU and APK_COMM_RCCL is not 0); else HIP IPC (the sender exports its staging buffer, the
 *                   receiver maps it and pulls with one device-to-device copy: peer reads over xGMI between GPUs, on-device
 *                   copies when ranks share a GPU; APK_COMM_IPC=0 switches it off); else the same bytes are staged through the
 *                   host and the TCP star - what the CPU tier tests drive (two processes, no GPU).
 * Schedules (csrc/comm.cpp):
 *   apk_msm_g1_sharded : BASELINE configs[3] - ONE MSM split by index range: every rank commits its slice on the MSM-only
 *                        context bound to the communicator, ONE all-gather of a 64/96-byte point per rank, local additions;
 *                        the result is returned on every rank.  (A numeric all-reduce cannot add curve points.)
 *   split proof        : ONE proof, several GPUs.  The leader (rank 0) calls apk_comm_split_begin, proves as usual
 *                        (apk_prove*), then apk_comm_split_end; every other rank sits in apk_comm_serve.  Each commitment batch
 *                        is dealt by index range of its flattened (scalar, point) pairs: header broadcast, one scatter of the
 *                        scalar slices, apk_msm_g1_batch_device on every rank, all-gather of the partial sums; with
 *                        APK_SPLIT_WIRES=1 the 4n-coset evaluation of wire i is dealt to rank i mod world (peer copies of the
 *                        canonical polynomial out and of the evaluations back).
 * Every rank holds the circuit context (apk_ctx_create with the same inputs), so any rank can commit any index range.
 * Errors on one rank are reported on all ranks of the step (status words travel with the partial sums); a peer that stops
 * answering INSIDE a step fails the call after APK_COMM_TIMEOUT_S seconds (default 300); between steps a worker in apk_comm_serve
 * waits for the leader's next header without a timeout (the leader may be idle for any length of time).  When APK_COMM_TOKEN is
 * set, its hash travels in every rank's hello and rank 0 refuses connections that do not carry it.
 * With RCCL as the data plane the partial sums of a sharded MSM / a dealt commitment batch are exchanged with ncclAllGather
 * (north_star: "RCCL-over-xGMI ... for the final bucket-sum of a single MSM"); the ranks add the gathered points themselves. */
typedef struct apk_comm apk_comm;
int apk_comm_create(int rank, int world, const char* addr, int port, apk_comm** out);   /* rank 0 listens on addr:port */
void apk_comm_destroy(apk_comm* comm);
int apk_comm_rank(const apk_comm* comm);
int apk_comm_world(const apk_comm* comm);
int apk_comm_barrier(apk_comm* comm);
int apk_comm_max_f64(apk_comm* comm, double* value);       /* in place: maximum over the ranks (bench.py's timing protocol) */
/* This rank's context (a circuit context for the split proof, an MSM-only context for the sharded MSM) and the data plane.
 * Collective: every rank calls it.  The communicator allocates its staging buffers through the bound context, so the context
 * must outlive the binding: apk_comm_bind(comm, NULL) (not collective) or apk_comm_destroy BEFORE apk_ctx_destroy. */
int apk_comm_bind(apk_comm* comm, apk_ctx* ctx);
const char* apk_comm_transport(const apk_comm* comm);      /* "rccl", "ipc" or "tcp" (after apk_comm_bind) */
/* Size of the RCCL communicator behind the data plane (ncclCommCount): `world` when the transport is "rccl", 0 otherwise. */
int apk_comm_rccl_ranks(const apk_comm* comm);
/* Why the data plane is NOT RCCL after apk_comm_bind ("" when it is): "single rank", "APK_COMM_RCCL=0", "librccl.so could not be
 * loaded", "ranks q and r share device d", "RCCL bring-up failed ..." - bench.py prints it as "fallback:<why>" instead of silently
 * timing the TCP star. */
const char* apk_comm_transport_reason(const apk_comm* comm);
/* One timed pass over the data plane as it came up (collective, after apk_comm_bind on a device context): a ring of grouped
 * ncclSend / ncclRecv of ring_bytes (RCCL plane only; 0 elsewhere) and an in-place all-gather of gather_bytes per rank on the active
 * plane.  GB/s = bytes this rank received / wall time of the second of two passes.  This is how the first run on a multi-GPU node
 * reports its per-link rate (DESIGN.md section 6 prices its projections at 48 GB/s per xGMI link, unmeasured). */
int apk_comm_link_probe(apk_comm* comm, size_t ring_bytes, size_t gather_bytes, double* ring_gbps, double* gather_gbps);
/* Where a schedule's time went on this rank since the last reset, host wall clock: out[0] = this rank's commitment MSMs (ms),
 * out[1] = the partial sums' exchange, out[2] = the sub-coset all-gather, out[3] = commitment rounds, out[4] = gathers. */
int apk_comm_phase_ms(apk_comm* comm, double* out5, int reset);
/* A world-1 RCCL communicator on `device` driven through every RCCL call of the data plane (unique id, ncclCommInitRank, a grouped
 * ncclSend / ncclRecv to itself on a non-blocking stream, ncclAllGather, ncclCommCount, ncclCommDestroy), results checked byte for
 * byte.  One-GPU boxes cannot run two RCCL ranks (RCCL refuses two ranks per device): this is how that branch's init, stream
 * use and teardown execute on hardware there.  *ranks receives ncclCommCount (1). */
int apk_comm_rccl_selftest(int device, int* ranks);
int apk_msm_g1_sharded(apk_comm* comm, const void* d_scalars, uint64_t len, void* out);
int apk_comm_split_begin(apk_comm* comm);
int apk_comm_split_end(apk_comm* comm);
int apk_comm_serve(apk_comm* comm, uint64_t* steps_served);
/* Test seam: the GPU touch points of the schedules as a table, so that the CPU tier can run the SAME C code (transport, dealing,
 * error propagation) in two processes without a GPU - "device" pointers are then host pointers and the table's msm is the
 * oracle's.  NULL entries keep the built-in implementation (the bound context).  kind: 0 device-to-device, 1 host-to-device,
 * 2 device-to-host. */
typedef struct {
    void* user;
    int (*msm_batch)(void* user, int basis, uint32_t count, const void* const* d_scalars, const uint64_t* offsets,
                     const uint64_t* lens, void* out_points);
    int (*coset_ntt)(void* user, const void* d_in, uint64_t len, void* d_out);
    int (*alloc)(void* user, size_t bytes, void** d_ptr);
    int (*release)(void* user, void* d_ptr);
    int (*copy)(void* user, void* dst, const void* src, size_t bytes, int kind);
    size_t g1_bytes;          /* 64 / 96 */
    uint64_t n;               /* domain size (coset evaluations are 4n Fr) */
} apk_compute;
int apk_comm_set_compute(apk_comm* comm, const apk_compute* table);
/* the schedules' entry points as the hooks call them (exposed for the tests of the seam) */
int apk_comm_commit(apk_comm* comm, int basis, uint32_t count, const void* const* d_scalars, const uint32_t* lens, void* out_points);
int apk_comm_wires(apk_comm* comm, uint32_t count, const void* const* d_canonical, const uint32_t* lens, void* const* d_evals);
/* Replicated prover ("SPMD", round 4): every rank holds the circuit context AND the witness and makes the same apk_prove* call
 * between apk_comm_spmd_begin and apk_comm_spmd_end (both called on every rank).  Only the commitments are shared out: rank r
 * commits its index range of each batch from its OWN copy of the polynomials, one all-gather of the partial sums, every rank adds
 * them - nothing is scattered (the leader / worker split above moves 604 MB per BLS12-381 2^21 proof out of rank 0) and the
 * Fiat-Shamir transcripts of the ranks stay identical, so every rank returns the same proof.  One proof at a time per
 * communicator.  apk_comm_commit_local is the step the hook runs (exposed for the tests of the seam). */
/* The sub-coset split of round 3 is ON by default in this mode for worlds of 2, 4 and 8 (APK_SPMD_SUBCOSET=0 switches it off) on
 * the strength of ELEMENT COUNTS only (24 n transformed elements per proof against 4 n + 20 n / G) and a projected 48 GB/s per xGMI
 * link: no box of the build had two GPUs.  bench.py --mode prove-spmd prints the measured link rate (apk_comm_link_probe) and the
 * per-phase times (apk_comm_phase_ms) so that the first multi-GPU run can confirm or overturn that default. */
int apk_comm_spmd_begin(apk_comm* comm);
int apk_comm_spmd_end(apk_comm* comm);
int apk_comm_commit_local(apk_comm* comm, int basis, uint32_t count, const void* const* d_scalars, const uint32_t* lens, void* out_points);
/* In-place all-gather of device memory (the sub-coset split's one exchange): d_all holds world x bytes_per_rank bytes, rank r's
 * part at r * bytes_per_rank.  ncclAllGather on the RCCL plane, pulls from the peers' exported buffers on the IPC plane, staged
 * through the host and the TCP star otherwise.  apk_comm_spmd_begin installs it as the bound context's gather hook when the world
 * is 2, 4 or 8 and APK_SPMD_SUBCOSET is not 0. */
int apk_comm_allgather_device(apk_comm* comm, void* d_all, size_t bytes_per_rank);
int apk_comm_subcoset_active(const apk_comm* comm);        /* 1 between spmd_begin and spmd_end when round 3 runs on sub-cosets */

/* ---- the verifier: the host-side mirror of plonk.Verify(proof, vk, publicWitness) (algoplonk.go:93) --------------------
 * (*CompiledCircuit).Verify runs the prover AND gnark's verifier before it hands out a VerifiedProof (algoplonk.go:79-98).
 * A Go integration keeps calling gnark's plonk.Verify on the returned *Proof; hosts without gnark (algoplonk_amd's Python
 * mirror of the API) call apk_verify.  Host only, no GPU: transcript, ~25 G1 scalar multiplications, one two-pair pairing
 * check.  The statement checked is the one the reference's generated AVM verifiers check
 * (verifier/templateLogicSigBN254.go:110-356).  Returns APK_OK, APK_ERR_VERIFY (proof rejected) or APK_ERR_ARG (bad key). */
typedef struct {
    int curve;
    uint64_t n;                /* VK Size */
    uint32_t nb_public;        /* VK NbPublicVariables */
    uint32_t nb_commitments;
    uint8_t ql[APK_G1_MAX_BYTES], qr[APK_G1_MAX_BYTES], qm[APK_G1_MAX_BYTES], qo[APK_G1_MAX_BYTES], qk[APK_G1_MAX_BYTES];
    uint8_t s[3][APK_G1_MAX_BYTES];
    uint8_t qcp[APK_MAX_COMMITMENTS][APK_G1_MAX_BYTES];
    uint32_t commitment_constraint_index[APK_MAX_COMMITMENTS];
    uint8_t g1[APK_G1_MAX_BYTES];        /* VK Kzg.G1 = SRS G1[0] */
    uint8_t g2[2][APK_G2_MAX_BYTES];     /* VK Kzg.G2 = ([1]G2, [tau]G2), gnark in-memory G2Affine */
} apk_verifying_key;
int apk_verify(const apk_verifying_key* vk, const apk_proof* proof, const void* public_inputs);   /* public_inputs: vk->nb_public Fr */
/* Same check with (a) the length of the public witness stated by the caller - gnark's plonk.Verify rejects
 * len(publicWitness) != vk.NbPublicVariables, and so does this call (APK_ERR_VERIFY) instead of reading vk->nb_public values
 * from a shorter buffer - and (b) optionally the intermediate values of the verification under the names the reference's
 * AVM template gives them (verifier/templateLogicSigBN254.go:137-140 gamma/beta/alpha/zeta, :181-193 PI, :218
 * linearized_poly_at_z, :256-278 lin_poly_com, :281-287 the folding challenge, :289-320 digest/claims before the two openings are
 * batched).  Scalars canonical big-endian; points X || Y big-endian as the AVM's ec ops return them (all zero = infinity).
 * tests/test_template_pin.py compares them with the values the executed template produced (tests/golden/template_verdicts.json).
 * Fields behind the point of rejection stay zero. */
typedef struct {
    uint8_t gamma[APK_FR_BYTES], beta[APK_FR_BYTES], alpha[APK_FR_BYTES], zeta[APK_FR_BYTES];
    uint8_t pi[APK_FR_BYTES], lin_at_zeta[APK_FR_BYTES], gamma_kzg[APK_FR_BYTES], folded_claim[APK_FR_BYTES];
    uint8_t lin_commitment[APK_G1_MAX_BYTES], folded_digest[APK_G1_MAX_BYTES];
} apk_verify_trace;
int apk_verify_ex(const apk_verifying_key* vk, const apk_proof* proof, const void* public_inputs, uint32_t nb_public_inputs,
                  apk_verify_trace* trace /* may be NULL */);
/* ---- batch verification: `count` proofs of ONE circuit, one pairing check when nothing is wrong (DESIGN.md "Batch verification").
 * Every proof is checked by itself first (sizes, canonical scalars, points on the curve and in the subgroup, zeta off the domain);
 * a proof that fails there is rejected alone.  Stage 1 computes [lin]_j of every other proof (segments of 11 + k scalar x point
 * terms); the pairing equations e(A_j, G2_0) e(B_j, G2_1) = 1 are then added with weights rho_0 = 1, rho_j = the low 128 bits of
 * sha256("apk-batch" || D || be32(j)), D = sha256 over the key's G1 points, be32(count) and, per proof, a marker byte (1 = the
 * proof's sizes match the key) followed by its 9 + k points, its claimed values l, r, o, s1, s2, qcp_i, z(zeta w) and its public
 * inputs (points X || Y big-endian as the transcript hashes them, scalars canonical big-endian); stage 2 is A = sum rho_j A_j,
 * B = sum rho_j B_j as one sum of two segments.  When the folded check fails the proofs are bisected (stage 1 is kept).
 * device >= 0: both stages and an additional on-curve / subgroup check of every proof point run on that GPU (APK_ERR_HIP when it is
 * not usable - no silent fallback); device = -1: the same sums on the host.  status[j] = APK_OK / APK_ERR_VERIFY per proof.
 * Returns APK_OK when every proof is accepted, APK_ERR_VERIFY when at least one is rejected, APK_ERR_ARG for a bad key exactly as
 * apk_verify.  Thread-safe; needs no apk_ctx, takes no proving slot and works on a stream of its own.
 * The trace holds what host mode, device mode and a restatement must agree on, in apk_verify_trace's encodings: D, rho_j and
 * [lin]_j of the first four proofs, A and B of the first fold, and the number of folds run (1 when nothing is rejected). */
typedef struct {
    uint8_t d[32];
    uint8_t rho[4][APK_FR_BYTES];
    uint8_t lin_commitment[4][APK_G1_MAX_BYTES];
    uint8_t a[APK_G1_MAX_BYTES], b[APK_G1_MAX_BYTES];
    uint32_t folds;
} apk_verify_batch_trace;
int apk_verify_batch(int device, const apk_verifying_key* vk, const apk_proof* proofs, const void* const* public_inputs,
                     const uint32_t* nb_public_inputs, uint32_t count, int* status, apk_verify_batch_trace* trace /* may be NULL */);
/* ---- batch verification across circuits: `count` proofs, each under one of `nb_keys` keys (proof j under keys[key_of[j]]).
 * It is apk_verify_batch with a key per proof: every per-proof check is made against the proof's own key, and a proof whose sizes
 * do not match its key (curve, number of commitments, number of public inputs) is rejected alone.  Every pairing equation has the
 * form e(A_j, G2_0) e(B_j, G2_1) = 1, so proofs of different circuits over the same SRS fold into one check: the keys are put into
 * GROUPS by curve and the bytes of g1, g2[0], g2[1] (numbered in the order of their first key), and each group with a proof that
 * passed its own checks gets one stage 1 ([lin]_j segments of 11 + k_j terms), one stage 2 (two segments; the scalars of every
 * KEY's own points S1, S2, Qcp_i are summed over that key's proofs, the scalar of G1 over the group) and one pairing check; a
 * failed fold is bisected inside its group.  Keys of both curves may be mixed in one call: they are different groups.
 * Weights: ONE digest over the whole call,
 *   D = sha256( be32(nb_keys)
 *               || per key:   be32(curve) || Ql Qr Qm Qo Qk S1 S2 S3 Qcp_0.. G1 || be64(n) || be32(nb_public) || be32(k)
 *                             || be32(commitment_constraint_index[i]) for i < k || g2[0] || g2[1]
 *               || be32(count)
 *               || per proof: marker byte || be32(key_of[j]) || when the marker is 1, what apk_verify_batch's D holds per proof:
 *                             the 9 + k points, the claimed values l, r, o, s1, s2, qcp_i, z(zeta w), the public inputs )
 * with G1 points X || Y big-endian as the transcript hashes them, scalars canonical big-endian, the G2 points as the 4 Fp elements
 * of the key's in-memory bytes (128 | 192 bytes each) and min(k, APK_MAX_COMMITMENTS) Qcp points and indexes; the marker is 1 when
 * the proof's sizes match its key and it arrived readable (apk_verify_blobs: a well-formed blob).  For EVERY j, the first included,
 *   rho_j = the low 128 bits of sha256("apk-batch-keys" || D || be32(j)).
 * device >= 0: the sums and an additional on-curve / subgroup check of every proof point run on that GPU (kernels_lincomb.h;
 * APK_ERR_HIP when it is not usable - no silent fallback); device = -1: the same sums on the host.  The host's own checks are
 * unconditional.  status[j] = APK_OK / APK_ERR_VERIFY.  Returns APK_OK when every proof is accepted (count = 0: the keys are
 * checked), APK_ERR_VERIFY when at least one is rejected, APK_ERR_ARG for a call that is wrong: a null pointer, nb_keys = 0 with
 * count > 0, key_of[j] >= nb_keys, an unknown curve in a key, or a bad key exactly as apk_verify reports one.  Thread-safe; needs
 * no apk_ctx and takes no proving slot.
 * The trace, in apk_verify_trace's encodings: D, rho_j and [lin]_j of the first four proofs, A and B of the first fold that ran
 * (the first fold of the first group with a proof to fold), the number of groups among the keys and the number of folds run. */
typedef struct {
    uint8_t d[32];
    uint8_t rho[4][APK_FR_BYTES];
    uint8_t lin_commitment[4][APK_G1_MAX_BYTES];
    uint8_t a[APK_G1_MAX_BYTES], b[APK_G1_MAX_BYTES];
    uint32_t groups;
    uint32_t folds;
} apk_verify_keys_trace;
int apk_verify_batch_keys(int device, const apk_verifying_key* keys, uint32_t nb_keys, const uint32_t* key_of,
                          const apk_proof* proofs, const void* const* public_inputs, const uint32_t* nb_public_inputs,
                          uint32_t count, int* status, apk_verify_keys_trace* trace /* may be NULL */);
/* ---- marshalled proofs: what MarshalProof / MarshalPublicInputs wrote (the wire formats below; csrc/proof_codec.h), read back.
 * A reader knows the curve and takes the number of commitments k from the length: a proof blob is apk_proof_blob_len(curve, k)
 * bytes for one k in 0..APK_MAX_COMMITMENTS, a public-inputs blob nb_public x 32.  Every coordinate must be below p and every
 * scalar below r; an all-zero point is infinity (on BLS12-381 the writer's own infinity encoding, 0x40 then zeros, has a
 * coordinate above p and is refused like any other: no proof the prover makes holds such a point).  Curve and subgroup membership
 * are the verifier's business, not the reader's.  claimed_values[0] and the five challenges of apk_proof come back zero.
 * Bytes that are not an acceptable proof are a REJECTED PROOF, APK_ERR_VERIFY, as they are for the AVM (the verifier templates
 * assert the lengths and return False on a non-canonical scalar); apk_last_error names the field and its byte offset.
 * APK_ERR_ARG is kept for a call that is wrong: a null pointer, an unknown curve, a `cap` that is too small.
 * apk_verify_blob: the verdict of apk_verify_ex on the unmarshalled proof and inputs, and the same trace; a blob whose k is not
 * the key's, or a public blob that is not 32 x vk->nb_public bytes, is rejected.
 * apk_verify_blobs: apk_verify_batch_keys on blobs; a malformed blob is rejected alone, by index, and enters D with marker 0. */
size_t apk_proof_blob_len(int curve, uint32_t nb_commitments);   /* 0: unknown curve or k > APK_MAX_COMMITMENTS */
int apk_unmarshal_proof(int curve, const uint8_t* blob, size_t len, apk_proof* out);
int apk_unmarshal_public_inputs(int curve, const uint8_t* blob, size_t len, void* out_fr, uint32_t cap, uint32_t* nb_public);
int apk_verify_blob(const apk_verifying_key* vk, const uint8_t* proof, size_t proof_len,
                    const uint8_t* public_inputs, size_t public_len, apk_verify_trace* trace /* may be NULL */);
int apk_verify_blobs(int device, const apk_verifying_key* keys, uint32_t nb_keys, const uint32_t* key_of,
                     const uint8_t* const* proofs, const size_t* proof_lens,
                     const uint8_t* const* public_inputs, const size_t* public_lens,
                     uint32_t count, int* status, apk_verify_keys_trace* trace /* may be NULL */);
/* The primitive underneath, host arrays in and out: out[s] = sum over i in [seg[s], seg[s+1]) of scalars[i] * points[i] for
 * s < nb_segments; seg holds nb_segments + 1 offsets, seg[0] = 0, non-decreasing; points G1 affine (any points of the curve,
 * infinity included), scalars Fr Montgomery.  An empty segment gives infinity.  device >= 0: kernels_lincomb.h on that GPU;
 * device = -1: the host. */
int apk_g1_lincomb_segments(int curve, int device, const void* points, const void* scalars, const uint64_t* seg,
                            uint32_t nb_segments, void* out_points);
/* G2 points for apk_verifying_key.g2 (host only).  apk_g2_decompress: one compressed G2 exactly as it sits in the
 * reference's vk.bin files (64 | 96 bytes, X.A1 || X.A0 big-endian with gnark's flag bits) -> in-memory form.
 * apk_g2_mul_generator: [scalar]G2 - the G2 side of a TestOnly SRS whose tau is known (unsafekzg, setup/setup.go:102-108);
 * scalar = one Fr in Montgomery form. */
int apk_g2_decompress(int curve, const uint8_t* compressed, void* out);
int apk_g2_mul_generator(int curve, const void* scalar_fr, void* out);

/* ---- test-only SRS generation: the device half of gnark's test/unsafekzg.NewSRS (setup/setup.go:102-108) ---
 * out[i] = scalars[i] * base.  Host buffers; scalars Fr Montgomery; base/out G1 affine.  The caller supplies
 * tau^i (canonical SRS) or L_i(tau) (Lagrange SRS) as the scalars. */
int apk_g1_mul_batch(int curve, int device, const void* base, const void* scalars, uint64_t count, void* out);

/* ---- trusted-setup loading on the GPU: what setup.Run's trusted branch does before plonk.Setup ----
 * apk_g1_decompress : kzg SRS ReadFrom (setup/setup.go:173-174,189-190).  `compressed` = count x (32 | 48) bytes exactly as
 *                     they sit in pk.bin after the 4-byte count (big-endian X with gnark's flag bits);
 *                     out = count G1 affine in gnark's in-memory form.  APK_ERR_ARG if any encoding is not a curve point.
 * apk_g1_to_lagrange: kzg.ToLagrangeG1 (setup/setup.go:124,138): out[i] = [L_i(tau)]G1 from points[j] = [tau^j]G1, n a
 *                     power of two, without knowing tau (inverse FFT in the exponent).  Host buffers. */
int apk_g1_decompress(int curve, int device, const uint8_t* compressed, uint64_t count, void* out);
int apk_g1_to_lagrange(int curve, int device, const void* points, uint64_t n, void* out);

/* ---- wire formats (host only, no GPU needed): replace MarshalProof / MarshalPublicInputs ----------------- */
/* helper.go:13-24,27-88: 768 + 96k bytes (BN254) / 1056 + 128k bytes (BLS12-381).  Returns the length in *len. */
int apk_marshal_proof(const apk_proof* proof, uint8_t* out, size_t cap, size_t* len);
/* helper.go:91-110: nb_public * 32 big-endian canonical bytes. */
int apk_marshal_public_inputs(int curve, const void* public_inputs, uint32_t nb_public, uint8_t* out, size_t cap);
/* Montgomery <-> canonical big-endian conversions for Fr (field=0) and Fp (field=1) elements; host only. */
int apk_fe_from_be(int curve, int field, const uint8_t* be, void* out);
int apk_fe_to_be(int curve, int field, const void* in, uint8_t* be);
/* hash_to_field with DST "BSB22-Plonk" over a marshalled G1 point (templateLogicSigBN254.go:386-397); host only. */
int apk_hash_fr(int curve, const void* g1_affine, void* out_fr);

/* ---- diagnostics: run the library's own field / curve templates on the HOST (no GPU).  The kernels are built
 * from the same templates, so the CPU-only test tier can pin the formulas against the oracle.
 * field ops: 0 add, 1 sub, 2 mul (Montgomery), 3 inverse, 4 neg; 10-13 = mul / add / sub / neg on unsaturated limbs; 14 = ten
 * lazy butterfly stages (u, v) <- (u + b v, u - b v) from (a, b) as the NTT tile runs them, returns u.  field: 0 = Fr, 1 = Fp.
 * g1 ops: 0 mixed add p+q, 1 full XYZZ add p+q, 2 double p, 3 scalar mul q*p (q = Fr Montgomery); 10/11 = 0/1 on the
 * MSM's unsaturated limbs; 12/13 = a fixed 17-step signed chain ending at p+3q through the accumulate loop's lazy
 * mixed addition / the plain one; 14 = lazy full additions and doublings ending at 4p+6q; 15 = 320 signed lazy mixed additions
 * of the points p + i q (selftest_ops.h lists the signs and the special steps), the lazy class checked after every step (an
 * all-ones record reports a state outside it). */
int apk_host_fe_op(int curve, int field, int op, const void* a, const void* b, void* out);
int apk_host_g1_op(int curve, int op, const void* p, const void* q, void* out);
/* The same bodies batched, one op per record (`count` records, host arrays in and out), and on the GPU: the device compile takes
 * other branches of the templates (the MacChain product of ff.h, the generated ffu_asm.h chains of ffu.h, the four-lane DPP point
 * forms of ec.h).  Test seams: nothing on the prove / MSM / NTT path calls them.
 * apk_device_fe_op: the field ops above; a, b, out = count elements each.
 * apk_device_g1_op: the g1 ops above (q = count Fr scalars for op 3, count points otherwise; q may be NULL for ops 2 and 21), plus
 * two device-only ops on four lanes per operation, whose `out` holds 4 points per op, one per lane: 20 = a + b through
 * add_quad_general, 21 = 2a through dbl_quad_general, both on operands taken into the lazy class by lazy operations (2a - a).  An
 * infinite operand is a copy, as in the MSM tails; a degenerate addition (a = +-b) is reported as an all-ones record.
 * apk_host_feu_op / apk_device_feu_op: raw unsaturated limbs (ffu.h FeU), no conversion.  `in` = count records of 4 operands
 * (a, b, c, d) of UL 32-bit words each, `out` = count records of UL words (words an op does not write are zero).  Ops:
 *   0 reduce_once(a)  1 add(a,b)  2 sub(a,b)  3 neg(a)  4 mul_nr(a,b)  5 mul(a,b)  6 sqr_nr(a)  7 sqr(a)  8 mul2_nr(a,b,c,d)
 *   9 add_n(a,b)  10 triple_n(a)  11 sub2_k<4>(a,b,c)  12..15 sub_k<1,2,4,6>(a,b)  16..18 neg_k<1,2,4>(a)
 *   19..24 canon<1,2,4,8,16,32>(a)  25 is_zero_mod_p(a) -> word 0  26 unpack(N packed words of a)  27 pack(a) -> N words
 *   28 from_fe(N words of a, gnark radix)  29 to_fe(a) -> N words.
 *   carry-save forms (limbs of the operands and results may exceed 2^UB): 40 add_s(a,b)  41 sub_s<2>(a,b)  42 neg_s<2>(a)
 *   43 sub_n<2>(a,b)  44..46 reduce_2p<4,8,32>(a)  47 canon<1>(reduce_2p<32>(a))  48 words 0..3 of a = limb factors fa, fb, fc, fd
 *   -> mul_takes(fa,fb), mul2_takes(fa,fb,fc,fd), sqr_takes(fa), COLUMN_ROOM.
 * apk_feu_shape: UL (limbs), UB (bits per limb) and HEADROOM (ffu.h) of the field's limb form. */
int apk_device_fe_op(int curve, int field, int op, int device, uint64_t count, const void* a, const void* b, void* out);
int apk_device_g1_op(int curve, int op, int device, uint64_t count, const void* p, const void* q, void* out);
int apk_host_feu_op(int curve, int field, int op, uint64_t count, const void* in, void* out);
int apk_device_feu_op(int curve, int field, int op, int device, uint64_t count, const void* in, void* out);
int apk_feu_shape(int curve, int field, int* ul, int* ub, uint32_t* headroom);
/* apk_device_poly_op: the prover's polynomial-stage kernels (csrc/kernels_poly.h) one stage per call, outside a proof.  Host arrays
 * in and out, no context; the stage's PRODUCTION kernels run with the launch geometry of a proof (csrc/poly_run.h holds the launch
 * sequences, shared with the prover) on scratch the call allocates and frees.  A test seam: nothing on the prove path calls it.
 * Every vector holds Fr elements in Montgomery form (32 bytes each, both curves), fr[] holds Fr constants the same way, iv[]
 * integers; len[] / out_len[] count elements and must be exactly what the op's layout below says - a vector that an op does not
 * take must be NULL.  The kernels' radix factors are part of what is tested and are NOT undone: constants and tables go in as the
 * kernels' headers list them (32 x, 1024 x ...: the product's radix R' = 32 R) and results come out as the kernels write them.
 * Unknown ops and arguments outside the layouts return APK_ERR_ARG before any device is touched.
 *   APK_POLY_GRAND_PRODUCT  vec 0..5 = L R O S1 S2 S3 (n), vec 6 = omega^i, i < n / 2; fr 0..3 = 32 beta, gamma, 32 beta u,
 *                           32 beta u^2; iv 0 = n (a power of two).  out 0, 1 = the rows' numerators and denominators (each the
 *                           exact product / 1024), out 2 = Z (n each).  A zero denominator is the caller's to avoid.
 *   APK_POLY_SCAN           vec 0 = data; iv 0 = 0 multiply / 1 add, iv 1 = rev, iv 2 = shift (forward only).  out 0 = the scan.
 *   APK_POLY_QUOTIENT       QuotientArgs field by field.  vec 0..3 = l r o z, vec 4 = zs (eight classes only), vec 5, 6 = pi2 (n4
 *                           each); vec 7..16 = qk ql qr qm qo s1 s2 s3 x l0, vec 17, 18 = qcp, vec 19..24 = inj_tab (n4 << sub_glog
 *                           each); fr 0..5 = alpha beta gamma beta_u beta_u2 alpha2, fr 6..9 = zh_inv, fr 10..15 = inj_delta;
 *                           iv 0..4 = n4 nb_commit nb_inject sub_k sub_glog.  out 0 = n4 values.
 *   APK_POLY_MERGE          vec 0 = part (G m), vec 1 = post (G m); fr 0..7 = rho_inv; iv 0 = m, iv 1 = log2 G.  out 0 = G m.
 *   APK_POLY_EVAL           vec 0..11 = the polynomials, vec 12..23 = a polynomial's own table of powers or NULL, vec 24 = the shared
 *                           table (at least as long as every polynomial that uses it); iv 0 = count.  out 0 = count values f(z) / 32.
 *   APK_POLY_LINCOMB        vec 0..19 = the vectors; fr 0..19 = 32 x the coefficients; iv 0 = count, iv 1 = out_len.  out 0 = out_len.
 *   APK_POLY_DERIVE_POWERS  vec 0, 1 = the two inputs (count), vec 2 = 32 omega^j, j < n / 2; iv 0 = n, iv 1 = count, iv 2, 3 = inverse
 *                           of each.  out 0, 1 = count each.
 *   APK_POLY_KZG_QUOTIENT   vec 0 = f (len), vec 1 = z^i, vec 2 = z^-i (len each; not taken when z = 0); iv 0 = len, iv 1 = z is
 *                           zero.  out 0 = len - 1 coefficients of (f - f(z)) / (X - z).
 *   APK_POLY_KZG_QUOTIENT2  two such quotients, neither at z = 0, in one batched launch sequence (the prover's pair of openings): vec 0..2 =
 *                           f, z^i, z^-i of the first (iv 0 elements each), vec 3..5 = of the second (iv 1).  out 0, 1 = len - 1 each.
 *   APK_POLY_BLIND          vec 0 = p (n + d, the last d ignored); fr 0..2 = b; iv 0 = n, iv 1 = d.  out 0 = n + d.
 *   APK_POLY_BLIND3         vec 0..2 = p or NULL, vec 3..5 = lag or NULL (n + d each); fr 4 j + i = b[j].v[i]; iv 0 = n, iv 1 = d.
 *                           out 0..5 = the vectors given, n + d each.
 *   APK_POLY_TAIL           vec 0 = len[0] records of 16 bytes; iv 0 = epoch, iv 1 = the flag word before the launch.  out 0 = the
 *                           flag word after it (one uint32_t). */
#define APK_POLY_GRAND_PRODUCT 0
#define APK_POLY_SCAN 1
#define APK_POLY_QUOTIENT 2
#define APK_POLY_MERGE 3
#define APK_POLY_EVAL 4
#define APK_POLY_LINCOMB 5
#define APK_POLY_DERIVE_POWERS 6
#define APK_POLY_KZG_QUOTIENT 7
#define APK_POLY_BLIND 8
#define APK_POLY_BLIND3 9
#define APK_POLY_TAIL 10
#define APK_POLY_KZG_QUOTIENT2 11
#define APK_POLY_VECS 32
#define APK_POLY_FRS 24
#define APK_POLY_INTS 8
#define APK_POLY_OUTS 6
typedef struct {
    const void* vec[APK_POLY_VECS];
    uint64_t len[APK_POLY_VECS];
    uint8_t fr[APK_POLY_FRS][32];
    int64_t iv[APK_POLY_INTS];
    void* out[APK_POLY_OUTS];
    uint64_t out_len[APK_POLY_OUTS];
} apk_poly_args;
int apk_device_poly_op(int curve, int op, int device, const apk_poly_args* args);
/* out = sum of `count` G1 affine points (host; 0 points give infinity): the local half of a sharded MSM's one exchange
 * step - the all-gathered per-rank partial sums are added with this call (algoplonk_amd/parallel.py). */
int apk_g1_sum(int curve, const void* points, uint64_t count, void* out);

/* ---- page-locked host memory for the inputs of apk_prove -------------------------------------------------------------------
 * apk_host_alloc: `bytes` of page-locked host memory, visible to every device (hipHostMalloc, portable); apk_host_free.
 * apk_host_register / apk_host_unregister: page-lock an EXISTING buffer for the lifetime of the registration (hipHostRegister) -
 * what a cgo host does once per witness-buffer pool: Go's heap does not move objects, and the pointer is only dereferenced
 * during apk_prove calls, which the cgo pointer rules allow.  APK_ERR_HIP without a device (no CPU fallback: nothing to feed). */
int apk_host_alloc(int device, size_t bytes, void** ptr);
int apk_host_free(void* ptr);
int apk_host_register(void* ptr, size_t bytes);
int apk_host_unregister(void* ptr);

/* ---- device memory helpers for callers that keep inputs resident (bench, batched proofs) ------------------ */
int apk_device_alloc(apk_ctx* ctx, size_t bytes, void** d_ptr);
int apk_device_free(apk_ctx* ctx, void* d_ptr);
int apk_device_upload(apk_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int apk_device_download(apk_ctx* ctx, void* dst, const void* d_src, size_t bytes);
int apk_device_copy(apk_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);   /* device to device, same GPU */

/* ---- timing hooks used by bench.py: HIP-event time of the dominant kernel on the stream it runs on ------- */
typedef struct {
    double msm_accumulate_ms;  /* sum of msm_accumulate_kernel durations since the last reset */
    uint64_t msm_accumulate_launches;
    uint64_t msm_pairs;        /* (scalar, point) pairs those launches covered */
    double msm_total_ms;       /* whole MSM batches (digits .. final) */
    uint64_t msm_batches;
    double ntt_ms;             /* all NTT passes */
    uint64_t ntt_elements;     /* elements transformed (sum of sizes) */
    double prove_ms;           /* wall time inside apk_prove* */
    uint64_t proofs;
    /* host wall clock per round of the prover, summed over `proofs` (the rounds of SURVEY.md section 3.3: R1 = wire polynomials,
     * BSB22 commitments, [L][R][O]; R2 = grand product, [Z]; R3 = quotient, [H1..3]; R4 = evaluations, [lin], the two
     * openings).  Each includes the Fiat-Shamir hashing that follows it.  host_lincomb_ms = the part of R4 spent in the
     * host-side combination of commitments that replaces the MSM of the linearised polynomial. */
    double round_ms[4];
    double host_lincomb_ms;
    double msm_sort_ms;        /* of msm_total_ms: recoding + counting sort + scans (everything in front of msm_accumulate_kernel) */
    double msm_tail_ms;        /* of msm_total_ms: merge of unit partials, row/column sums, bit sums, final scaling (everything behind it) */
} apk_stats;
int apk_stats_enable(apk_ctx* ctx, int enable); /* enabling inserts hipEvents around the kernels above */
int apk_stats_read(apk_ctx* ctx, apk_stats* out, int reset);

/* ---- which forms the library took ------------------------------------------------------------------------------------------
 * Several kernels exist in two forms and the library picks one per launch from the LOAD it sees (how many proving slots are busy):
 * a lone proof gets the short-chain / latency forms, proofs under load the instruction-lean ones.  All forms give the same bytes;
 * the parity tests prove it by asserting, through these counters, that the loaded forms really ran while the blobs they compare
 * were produced (tests/test_gpu_parity.py::test_proofs_under_load_*).  Counted always, independent of apk_stats_enable - the
 * statistics synchronise the host with every batch and would change the very load the choices depend on. */
typedef struct {
    uint64_t proofs;                    /* apk_prove* calls that returned a proof */
    uint64_t msm_batches;               /* MSM launch sequences (1..4 MSMs each) */
    uint64_t msm_sort_two_level;        /* ... sorted in two levels (partitions, then LDS tiles) */
    uint64_t msm_sort_two_level_by_load;/* ... of those, two-level only BECAUSE other proofs were in flight (below 2^16 bases) */
    uint64_t msm_sort_fused;            /* ... two-level in the two-launch form */
    uint64_t msm_lean_tail;             /* lean tail: one lane per bucket in the merge from 32 768 buckets, lean row/column sums */
    uint64_t msm_rowcol_serial;         /* sixteen-lane serial row/column sums */
    uint64_t msm_combine_quad;          /* four lanes per addition in the merge (small lone batch) */
    uint64_t msm_small_units;           /* shrunken accumulate units (small lone batch) */
    uint64_t msm_one_launch;            /* whole MSM in one cooperative launch (small lone batch) */
    uint64_t msm_lagrange_wires;        /* [L][R][O] committed over the Lagrange SRS (small-scalar fast path) */
    uint64_t ntt_sequences;             /* NTT launch sequences */
    uint64_t ntt_radix4;                /* ... with radix-4 steps */
    uint64_t ntt_radix4_by_load;        /* ... radix-4 only BECAUSE other proofs were in flight (2^17..2^19) */
    uint64_t tail_fill_proofs;          /* lone proofs whose coset transforms ran beside the MSM tails (side stream) */
    uint64_t host_lincomb_pooled;       /* [lin] combinations of nearly idle contexts dealt to parked host threads (BLS12-381 by default; BN254 with APK_HOST_LINCOMB_THREADS > 1) */
    uint64_t msm_units_by_load;         /* MSM batches whose accumulate units were lengthened BECAUSE other proofs were in flight */
    uint64_t host_inputs;               /* proofs whose L, R, O came from host memory through a staging set (apk_prove) */
    uint64_t gang_proofs;               /* proofs made as members of a gang (two to four proofs sharing one stream and its MSM / NTT launches) */
    uint64_t gang_msm_launches;         /* MSM launch sequences that carried the batches of more than one proof */
    uint64_t gang_ntt_launches;         /* NTT launch sequences that carried the transforms of more than one proof */
    uint64_t gang_kernel_launches;      /* other kernels (grand product, quotient, evaluations, openings ...) launched once for several proofs */
    uint64_t forms_by_device_load;      /* launch sequences that took a loaded form ONLY because of OTHER contexts' proofs on the device (this context's own count was below the threshold) */
    uint64_t msm_inplace;               /* MSM batches whose one-unit buckets were summed in place: the merge neither loads nor stores for them (APK_MSM_INPLACE) */
} apk_path_counts;
int apk_paths_read(apk_ctx* ctx, apk_path_counts* out, int reset);

/* ---- the device-wide scheduler ---------------------------------------------------------------------------------------------
 * A process may hold several contexts on one GPU (one per compiled circuit).  They share what belongs to the device: the proving
 * streams (APK_MAX_SLOTS of them, default 16, over ALL contexts of the device), the load figure the load-dependent kernel forms
 * and the gangs are decided from, and the order in which waiting callers get a stream (first come, first served, across
 * contexts).  APK_DEVICE_SCHED=0 (read once per process) gives every context a stream pool and a load figure of its own again.
 * apk_device_sched_read touches host state only: without a GPU, or before any context exists, it returns APK_OK with zero counts,
 * max_streams and device_wide.  APK_ERR_ARG for device < 0 or a null out. */
typedef struct {
    uint32_t contexts;          /* contexts attached to this device's scheduler */
    uint32_t max_streams;       /* the device's budget (APK_MAX_SLOTS) */
    uint32_t streams_in_use, streams_peak;   /* proving streams held now / most at once since the last reset */
    uint32_t proofs_in_flight, proofs_peak;  /* slots held over all contexts */
    uint32_t waiting;           /* callers waiting for a slot or a stream */
    uint32_t device_wide;       /* 1 = this scheduler is on, 0 = APK_DEVICE_SCHED=0 */
} apk_device_sched;
int apk_device_sched_read(int device, apk_device_sched* out, int reset);

/* ---- the runtime environment -------------------------------------------------------------------------------------------------
 * What the library did to GPU_MAX_HW_QUEUES when it was loaded (the contract at the top of this file), and whether the variable
 * still held that at the library's first call into the HIP runtime - the first entry point that can reach a device, host-only
 * ones (marshalling, verification on the host, this one) do not count.  Queue counts are the variable's value, or
 * APK_HWQ_UNSET for a missing variable, APK_HWQ_UNREADABLE for an empty one or one with any character that is not a decimal digit.
 * Host state only: works without a GPU.  Whether the RUNTIME took the value shows only in a kernel trace's queue count - a
 * host that initialised HIP before it loaded the library is not visible from here.  APK_ERR_ARG for a null out. */
#define APK_HWQ_UNSET (-1)
#define APK_HWQ_UNREADABLE (-2)
typedef struct {
    int32_t hw_queues_found;        /* GPU_MAX_HW_QUEUES when the library was loaded */
    int32_t hw_queues_left;         /* ... after the library's constructor */
    int32_t hw_queues_need;         /* what the library asks for: 16, or APK_HW_QUEUES held to 4 .. 32; 0 = APK_HW_QUEUES=0, nothing asked */
    int32_t hw_queues_written;      /* 1 = the constructor wrote the variable (hw_queues_left is then hw_queues_need) */
    int32_t hw_queues_now;          /* the variable at the time of this call */
    int32_t first_hip_call;         /* -1 = the library has not called the HIP runtime yet; 1 = the variable still held hw_queues_left then; 0 = somebody changed it in between */
    int32_t hw_queues_at_first_hip; /* the variable at that call (APK_HWQ_UNSET before it) */
    int32_t reserved;
} apk_runtime;
int apk_runtime_read(apk_runtime* out);

#ifdef __cplusplus
}
#endif
#endif /* APK_H */
