// Per-curve backend: circuit context resident in HBM + the PLONK prover driven from one host thread per
// proof.  Instantiated for BN254 and BLS12-381 in backend_bn254.hip / backend_bls12381.hip.
//
// Replaces plonk.Prove (/root/reference/algoplonk.go:89) and the device-relevant part of plonk.Setup
// (/root/reference/setup/setup.go:107,149) [both UPSTREAM gnark v0.15.0, not vendored].  The round
// structure follows SURVEY.md §3.3; what every round must produce is pinned by the verifier template
// (/root/reference/verifier/templateLogicSigBN254.go, lines cited at each step).  GPU-natural schedule,
// not gnark's: everything between two Fiat-Shamir challenges is a chain of launches on one HIP stream with
// all polynomials resident; [Z], [H1..3] and the openings are committed over the CANONICAL SRS, [L][R][O] over the canonical SRS
// after the iNTT or - round 5, when the witness makes it cheaper - over the Lagrange SRS the way gnark does (same group
// elements either way); the quotient is evaluated on ONE 4n coset (4 coset NTTs per proof, the 7 trace polynomials' coset
// evaluations are precomputed per circuit).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <new>
#include <mutex>
#include <string.h>
#include <time.h>
#include <vector>

#include "backend.h"
#include "dev_buf.h"    // DevBuf and the CHK macros
#include "slot_pinned.h"   // PIN_*: a slot's page-locked result buffer
#include "msm_run.h"   // the MSM: kernels_msm.h, msm_plan.h, its workspace and launches
#include "kzg_run.h"   // the KZG openings: kernels_kzg.h, kernels_kzg_lagrange.h, their scratch and launches
#include "kzg_all_run.h"   // the openings at every point of the domain: kernels_kzg_all.h, their tables, scratch and launches
#include "kzg_cosets_run.h"   // the openings on every coset of the domain: kernels_kzg_cosets.h, their table, scratch and launches
#include "kzg_cosets_multi_run.h"   // many polynomials on every coset in one call: kernels_kzg_cosets_multi.h, a group's scratch and launches
#include "kzg_recover_run.h"  // the polynomial back from a sufficient set of those cosets: kernels_kzg_recover.h, scratch and launches
#include "ntt_run.h"   // the NTT: kernels_ntt.h, ntt_plan.h, its knobs and launches
#include "kernels_poly.h"
#include "poly_run.h"  // the polynomial stages' launch sequences, shared with the test seam (seam_run.h)
#include "gang_run.h"  // a gang's recorded launches and requests: gang_kernel.h, gang_plan.h
#include "setup_run.h" // the setup-time entry points (kernels_setup.h); g1_to_lagrange_dev for the Lagrange SRS derived on the device
#include "host_msm.h"
#include "slot_gate.h"
#include "gang.h"
#include "plonk_protocol.h"

namespace apk {

template <class FRP, class FPP, int CURVE_ID>
class CurveBackend : public Backend {
  public:
    using Fr = Fe<FRP>;
    using Fp = Fe<FPP>;
    using Aff = Affine<FPP>;
    using Pt = XYZZ<FPP>;
    using PtU = XYZZ<FPP, FeU<FPP>>;  // MSM-internal points: unsaturated limbs (ffu.h)
    using Proto = PlonkProtocol<FRP, FPP>;   // transcript, hash-to-field, PI(zeta), the scalars of [lin]: shared with the verifier

    // ---------------------------------------------------------------------------------------------- host Fr
    static Fr fr_u64(uint64_t v) {
        Fr a = Fr::zero();
        a.l[0] = (uint32_t)v;
        a.l[1] = (uint32_t)(v >> 32);
        return Fr::to_mont(a);
    }

    // what each region of a slot's pinned buffer (slot_pinned.h) holds at most, for this curve
    static_assert(PIN_AFF + MSM_MAX_BATCH * sizeof(Aff) <= PIN_XYZZ, "a proof's batch of affine commitments fits its region");
    static_assert(PIN_XYZZ + MSM_ARGS_MAX * sizeof(Pt) <= PIN_FR, "the XYZZ sums of a launch sequence fit their region");
    static_assert(PIN_FR + (EVAL_MAX > KZG_MAX_POLYS ? EVAL_MAX : KZG_MAX_POLYS) * sizeof(Fr) <= PIN_TAIL, "evaluations and an opening's values fit the scalar region");

    // ---------------------------------------------------------------------------------------------- prover knobs
    // The prover's run-time knobs, from the environment: latched at the first proof of the process (per curve).
    struct ProverKnobs {
        // The context's parked host threads for the [lin] combination while a proof has the context (nearly) to itself - then the
        // GPU idles through it; with many proofs in flight the callers' own threads already keep the host busy.  Since the combination
        // takes GLV halves and fixed-base tables (host_msm.h) one thread does BN254's in 0.10 ms (0.15 before) and waking three more
        // costs what they save; BLS12-381's (0.23 ms) still gains a little from three (same box: tools/ab_lone.sh).
        int lc_threads = env_int("APK_HOST_LINCOMB_THREADS", FPP::N <= 8 ? 1 : 3, 1, 8);
        bool host_glv = env_int("APK_HOST_GLV", 1, 0, 1) != 0;       // 0: full-length scalars (measurement aid; same bytes)
        bool host_fixed = env_int("APK_HOST_FIXED", 1, 0, 1) != 0;   // 0: [Ql][Qr][Qm][Qo][S3] through the Straus pass (measurement aid; same bytes)
        int powers_derive = env_int("APK_POWERS_DERIVE", 1, 0, 1);   // 0: four square-and-multiply tables of powers (zeta_powers)
        int open_pair = env_int("APK_OPEN_PAIR", 1, 0, 1);           // 0: the two opening quotients as two launch sequences (round 4)
        int lin_early_h = env_int("APK_LIN_EARLY_H", 1, 0, 1);       // 0: the [H] part of [lin] with the rest, after the evaluations
        int tail_fill = env_int("APK_TAIL_FILL", 1, 0, 2);           // tail_fill()
    };
    static const ProverKnobs& prover_knobs() { static const ProverKnobs k{}; return k; }

    // ---------------------------------------------------------------------------------------------- state
    // APK_MSM_GRAPH=1: the launch sequence of an MSM batch (10 kernels + the result copy) is captured once per (slot, table,
    // scalar vectors, lengths) into a hipGraph and replayed with one hipGraphLaunch.
    struct GraphKey {
        const void* table; MsmBatchArgs a;
        bool operator==(const GraphKey& o) const { return table == o.table && memcmp(&a, &o.a, sizeof a) == 0; }
    };
    struct Slot {
        hipStream_t stream = nullptr;      // the stream this slot's launches go to: its own, or - as a gang member - its lead's
        hipStream_t own_stream = nullptr;  // one of the context's stream_pool_, held while this slot leads a gang or proves alone (not owned)
        // gang membership of the proof in flight on this slot (gang.h; set by MemberGuard)
        Slot* lead = nullptr;              // whose stream, MSM workspace, transform scratch and XYZZ result area it uses (itself when alone)
        int gang_idx = 0;
        bool in_gang = false;
        uint32_t res_off = 0;              // first point of this proof's pending MSM sums in the lead's XYZZ area
        uint32_t res_write_off = 0;        // (as a lead) where the launch sequence being queued writes its sums in that area
        Gang gang;                         // used when this slot leads
        GangRecorder cmds;                 // launches recorded since the last merge point (as a gang member; gang_run.h)
        hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
        size_t index = 0;          // position in slots_ = the slot's number at the gate
        // polynomials
        DevBuf wl, wr, wo;             // L,R,O Lagrange (n)
        DevBuf cl, cr, co, cz;         // blinded canonical (n+3 capacity)
        DevBuf qk_lag, qk_can;         // completed Qk
        DevBuf ratio, zlag, scan_tot;  // grand product
        DevBuf el, er, eo, ez, eqk;    // 4n coset evaluations
        DevBuf quot, hcan;             // quotient evaluations / coefficients (4n)
        DevBuf pw_z, pw_zi, pw_zw, pw_zwi;  // powers of zeta, 1/zeta, omega*zeta, 1/(omega*zeta)   (n+3)
        DevBuf tmp2, folded, tmp, q1, q2;   // n+3 (tmp2: scratch of the second opening quotient when the two share their launches)
        DevBuf eval_partial, eval_result;
        DevBuf pi2_can[APK_MAX_COMMITMENTS], epi2[APK_MAX_COMMITMENTS];
        DevBuf scratch_in;  // upload staging for primitives
        KzgScratch<FRP> kzg;  // apk_kzg_*: the openings' scratch (kzg_run.h; allocated on a slot's first opening)
        KzgAllScratch<FRP, FPP> kzg_all;  // apk_kzg_open_all: 2n XYZZ points and 3n scalars (kzg_all_run.h; allocated on a slot's first such call)
        KzgCosetsScratch<FRP, FPP> kzg_cosets;  // apk_kzg_open_cosets: 2n' XYZZ points and 5n scalars (kzg_cosets_run.h; allocated on a slot's first such call)
        KzgCosetsMultiScratch<FRP, FPP> kzg_cosets_multi;  // apk_kzg_open_cosets_multi: 3 G n' XYZZ points and 6 G n scalars for the slot's largest group so far (kzg_cosets_multi_run.h)
        KzgRecoverScratch<FRP> kzg_recover;     // apk_kzg_recover_cosets: 2n + 3n' scalars and the maps (kzg_recover_run.h; allocated on a slot's first such call)
        DevBuf ntt_wide;    // NTT_MAX_BATCH transforms of 4n unsaturated-limb elements: the NTT's inter-pass form
        MsmWorkspace<FPP> msm;     // the MSM's buffers (msm_run.h); a gang member's batches run on its lead's
        void* h_pinned = nullptr;  // small pinned staging for results (PIN_* above: affine points, XYZZ sums, scalars, flags)
        uint32_t pending_pts = 0;  // MSM sums waiting in h_pinned for their affine conversion (sync_results)
        uint8_t* d_pinned = nullptr;   // the device's view of h_pinned (zero-copy results: the last kernel of a batch writes them there), or null
        std::vector<std::pair<GraphKey, hipGraphExec_t>> graphs;   // APK_MSM_GRAPH
        bool hook_pending = false; // a commitment batch handed to the context's commit hook at the next sync_results()
        int hook_basis = 0;
        MsmBatchArgs hook_args{};
        DevBuf sc_gather;          // sub-coset split: the G parts of the inverse transform (4n elements), all-gathered in place
        DevBuf tail_flag;          // epoch of the last proof whose quotient had a non-zero tail (tail_nonzero_kernel)
        uint32_t epoch = 0;
        // tail filling (a lone proof only, see tail_fill()): the coset transforms that follow a commitment run on `side` from the
        // moment the batch's accumulate kernel is done, beside the reduction tail that would otherwise have the GPU to itself
        hipStream_t side = nullptr;
        hipEvent_t ev_acc = nullptr, ev_side = nullptr;
        hipEvent_t ev_sync = nullptr;   // blocking-wait event (hipEventBlockingSync): the host thread sleeps instead of spinning
        int mark_acc = 0; bool side_pending = false;   // mark_acc: 1 = event behind the accumulate kernel, 2 = in front of the batch
    };

    int curve_ = CURVE_ID;
    int device_ = 0;
    uint32_t n_ = 0, log_n_ = 0, n4_ = 0;
    uint32_t nb_public_ = 0, nb_commit_ = 0;
    uint32_t cci_[APK_MAX_COMMITMENTS] = {0, 0};
    MsmCtxPlan msm_ctx_{};    // the window, its layout and the two-level sort's (choose_window, from msm_plan_context)
    bool msm_only_ = false;
    std::unique_ptr<HostPool> lc_pool_;   // parked host threads for the [lin] combination of a lone proof (created on first use)
    bool many_slots_ = false;   // a throughput context (more than two proving slots): small MSMs may take the two-level sort under load
    // gangs (gang.h, slot_gate.h): up to gang_cap_ proofs per stream, their MSM / NTT batches in one launch sequence.  A slot's MSM
    // workspace, transform scratch and XYZZ result area are sized for ws_batch_ = MSM_MAX_BATCH x gang_cap_ operands.
    int gang_cap_ = 1;
    uint32_t ws_batch_ = MSM_MAX_BATCH;
    Gang::Launcher gang_launcher_;
    uint32_t msm_bases_ = 0;  // bases the MSM workspaces are sized for
    Fr omega_, omega_inv_, omega4_, omega4_inv_, shift_, shift_inv_, n_inv_, n4_inv_;
    Fr zh_inv_[4];
    // circuit-level device data
    // NTT tables hold w * R' (R' = 2^261, the radix of the tile arithmetic: kernels_ntt.h); tw_n_ = omega^i in gnark's radix
    // is what the grand product and the permutation columns read
    DevBuf tw_n_, twu_n_, twi_n_, tw_4n_, twi_4n_, coset_pre_, coset_post_inv_, scales_;  // scales_: [1/n, 1/(4n)]
    DevBuf twu_n_x_, twi_n_x_, tw_4n_x_, twi_4n_x_;   // the four transform tables once more as FeU records (ntt_pass_kernel<.., TWU>); built with APK_NTT_TWU=1 (default 0: measured neutral)
    bool ntt_twu_ = false;
    DevBuf x4_, l0_4_;
    DevBuf s_lag_[3], ql_c_, qr_c_, qm_c_, qo_c_, qk_c_, s_c_[3], qcp_c_[APK_MAX_COMMITMENTS];
    DevBuf qk_lag_trace_;
    // Qk completion in the quotient kernel (kernels_poly.h QuotientArgs::nb_inject): trace Qk on the coset, the Lagrange
    // polynomials of the written rows on the coset, the trace's own values in those rows
    bool qk_direct_ = false;
    DevBuf eqk_trace_, inj_tab_[QK_INJECT_MAX];
    std::vector<uint32_t> inj_row_;
    std::vector<Fr> inj_trace_val_;
    DevBuf eql_, eqr_, eqm_, eqo_, es_[3], eqcp_[APK_MAX_COMMITMENTS];
    // tab_lag_ (round 5): PLAIN multiples of the n Lagrange-SRS points followed by the three blinding points
    // D_k = [tau^(n+k)]G1 - [tau^k]G1, so that  [f + b(X)(X^n - 1)] = sum f(omega^i) [L_i(tau)] + sum b_k D_k  is ONE MSM over the
    // witness values themselves (gnark commits L, R, O this way: setup/setup.go:124,138 builds the Lagrange SRS for it).  Plain:
    // a witness value 0 / 1 / small then has 0 / 1 / few non-zero digits, where R^-1 tables see a uniform a * R mod r.
    MsmTables tab_can_, tab_lag_;
    int wires_lag_mode_ = -1;                            // APK_WIRES_LAGRANGE at context creation: -1 auto, 0 never, 1 always
    // The extended Lagrange table is REQUIRED only by BSB22 commitments and by a forced Lagrange route (it is then built when the
    // context is created and a failure fails the creation).  In the automatic mode without a caller's Lagrange SRS it is an
    // optimisation some witnesses never use (uniform wires measure >= 90 % density; contexts with hooks commit canonically): the
    // context keeps the canonical SRS on the device (8 / 12 MB at 2^17; the table itself would be 134 / 280 MB and a device iFFT in
    // the exponent) and DERIVES the table the first time a proof's density - or the basis-1 primitive - asks for it, best effort:
    // a failure (out of memory ...) clears the error and leaves the canonical route in place.
    DevBuf srs_keep_;                                    // canonical SRS (n + 3 points) for the lazy derive; released after it
    Aff lag_dk_[3];                                      // D_k = [tau^(n+k)]G1 - [tau^k]G1 (host, at creation)
    std::mutex lag_mu_;
    std::atomic<bool> lag_ready_{false};                 // tab_lag_ is built (release / acquire around the build)
    std::atomic<bool> lag_failed_{false};                // a lazy derive failed: never tried again
    std::atomic<uint32_t> wire_density_pm_{0xffffffffu}; // non-zero digits of the last measured proof's wires, per mille of uniform
    std::atomic<uint32_t> proof_seq_{0};
    enum { VK_QL, VK_QR, VK_QM, VK_QO, VK_QK, VK_S1, VK_S2, VK_S3, VK_QCP };   // vk_pts_: the order of apk_vk
    Aff vk_pts_[8 + APK_MAX_COMMITMENTS];
    HostFixedBase<FPP> vk_fixed_;   // host tables of [Ql][Qr][Qm][Qo][S3] for the [lin] combination (host_msm.h)
    // apk_kzg_all_prepare / apk_kzg_open_all (kzg_all_run.h): T^ and the twiddles, built once under all_mu_
    KzgAllTables<FRP, FPP> all_tab_;
    std::mutex all_mu_;
    std::atomic<bool> all_ready_{false};
    bool tw_ready_ = false;              // all_tab_'s stage form is chosen and its twiddle records are built (under all_mu_: by whichever prepare ran first)
    // apk_kzg_cosets_prepare / apk_kzg_open_cosets (kzg_cosets_run.h): the table of one coset size, built once under all_mu_
    KzgCosetsTables cos_tab_;
    std::atomic<uint32_t> cos_l_{0};     // the coset size the context is prepared for (0: none)
    // apk_kzg_recover_cosets (kzg_recover_run.h): g^(-c) / n, c < n, in the NTT's radix - the `post` operand of the last inverse
    // transform, as coset_post_inv_ is for 4n.  Built by the first such call, under recover_mu_.
    DevBuf recover_post_;
    std::mutex recover_mu_;
    std::atomic<bool> recover_ready_{false};
    std::vector<Slot*> slots_;
    // The context's streams: as many as it may run at a time (max 16), whichever of its slots lead.  A stream per SLOT - 32 slots
    // for gangs of two - put 23 hardware queues to work within 150 ms and starved some of them for up to 90 ms (with the spinning
    // waits of that build on top: profiles/r06_gang_sweep.txt).
    // Since the device-wide scheduler (device_sched.h) the pool is a BORROWED view of the device's proving streams - created once
    // per device ordinal (apk_api.cpp device_stream_pool), shared by every context on it, never destroyed by a context - and the
    // stream ids come from the device's scheduler, so all contexts of a process together run max 16 streams.  APK_DEVICE_SCHED=0:
    // a pool of the context's own, as before (owns_streams_).
    std::vector<hipStream_t> stream_pool_;
    bool owns_streams_ = false;
    SlotGate gate_;            // who proves on which slot; the DEVICE's load figure behind it picks the load-dependent kernel forms (slot_gate.h, device_sched.h)
    // Host inputs (apk_prove: the call the cgo shim makes): a caller takes one of `in_sets_` BEFORE it takes a
    // proving slot and sends L, R, O on the context's copy stream - so the upload of a proof that still waits for a slot (32 callers
    // on 16 slots) runs beside the rounds of the proofs in flight, and a proof in flight never has a PCIe transfer in its chain.
    // Pinned sources (apk_host_alloc / apk_host_register) are true asynchronous DMA; pageable ones are pinned on the fly by the
    // runtime inside hipMemcpyAsync on the calling thread, which is waiting for a slot anyway (both 46 GB/s for 3 x 4 MiB on the
    // boxes of this build: tools/ubench/h2d_probe.hip).  ONE copy stream for all sets: PCIe serialises the transfers anyway, and
    // every further stream is a further hardware queue - a stream per set (32 of them beside the 16 proving streams, on 24
    // hardware queues) cost 8 % proofs/s and 2.4 ms of a lone proof's latency (profiles/r06_host_inputs_ab.txt).
    // Created on the first host-input proof.
    struct InputSet {
        DevBuf w[3], pi2[APK_MAX_COMMITMENTS];
        hipStream_t copy = nullptr;     // the context's copy stream (not owned)
        hipEvent_t ready = nullptr;
        size_t index = 0;
    };
    std::vector<InputSet*> in_sets_;
    SlotGate in_gate_;
    hipStream_t copy_stream_ = nullptr;
    std::mutex mu_;
    // intra-proof multi-GPU (apk_ctx_set_commit_hook): the prover's commitments go through the host's hook instead of this GPU
    apk_commit_hook hook_ = nullptr;
    void* hook_user_ = nullptr;
    apk_wire_hook wire_hook_ = nullptr;
    void* wire_hook_user_ = nullptr;
    // Sub-coset split of round 3 (apk_ctx_set_subcoset): this context stands for the points
    // i = k (mod G) of the 4n coset - a coset of m = 4n / G points, u w^k <w^G> (w = omega_4n).
    //   forward   f(u w^k w_m^j) = NTT_m( fold_m( f_i (u w^k)^i ) )        pre[0] = (u w^k)^i;  pre[1]: class (k + 4) mod 8 for Z(omega X) at G = 8
    //   inverse   part_k[c'] = w^(-k c') * (unscaled inverse NTT_m of the quotient values)[c']        post = w^(-k c')
    //   merge     h_(c' + m t) = u^-c / (4n) * sum_k rho^(-k t) part_k[c'],  rho = w^m       (subcoset_merge_kernel, after the all-gather)
    struct SubCoset {
        int k = 0, G = 1, glog = 0;
        apk_gather_hook hook = nullptr;
        void* user = nullptr;
        DevBuf pre[2], post;
        Fr rho_inv[8];
        bool on() const { return G > 1 && hook; }
    } sc_;
    // which forms the load-dependent choices took (apk_paths_read): always counted, relaxed atomics
    enum PathIdx { P_PROOFS, P_MSM_BATCHES, P_SORT2, P_SORT2_LOAD, P_SORT_FUSED, P_LEAN_TAIL, P_ROWCOL_SERIAL, P_COMBINE_QUAD, P_SMALL_UNITS,
                   P_ONE_LAUNCH, P_LAGRANGE_WIRES, P_NTT_SEQ, P_NTT_R4, P_NTT_R4_LOAD, P_TAIL_FILL, P_LINCOMB_POOL, P_UNIT_LOADED, P_HOST_INPUTS, P_GANG_PROOFS, P_GANG_MSM, P_GANG_NTT, P_GANG_KERNELS, P_DEVICE_LOAD, P_MSM_INPLACE, P_COUNT };
    std::atomic<uint64_t> paths_[P_COUNT] = {};
    void path(PathIdx i) { paths_[i].fetch_add(1, std::memory_order_relaxed); }
    // More than `thr` proofs in flight on the DEVICE (every context attached to its scheduler; this caller's own included)?
    // *foreign: only the other contexts' proofs say so - this context's own count is at or below `thr` (forms_by_device_load).
    bool device_load_over(int thr, bool* foreign = nullptr) {
        int own = 0;
        const int dev = gate_.load(&own);
        if (foreign) *foreign = dev > thr && own <= thr;
        return dev > thr;
    }
    int paths_read(apk_path_counts* out, int reset) override {
        static_assert(sizeof(apk_path_counts) >= P_COUNT * sizeof(uint64_t), "apk_path_counts holds every counter");
        memset(out, 0, sizeof *out);
        uint64_t* o = reinterpret_cast<uint64_t*>(out);    // the struct's fields are in PathIdx order
        for (int i = 0; i < P_COUNT; i++) o[i] = reset ? paths_[i].exchange(0, std::memory_order_relaxed) : paths_[i].load(std::memory_order_relaxed);
        return APK_OK;
    }
    // stats
    bool stats_on_ = false;
    uint32_t simds_ = 1024;  // SIMDs of the device (4 per CU); set at init
    std::mutex stats_mu_;
    apk_stats stats_{};

    ~CurveBackend() override {
        (void)hipSetDevice(device_);
        gate_.detach();      // (nobody of this context is inside the gate any more: the device's scheduler forgets it first)
        // Borrowed streams carry other contexts' proofs as well.  They are synchronised - whatever this context still has in flight
        // on them (an error return drains its stream itself: release()) is then over, and what other contexts queue meanwhile is
        // not waited for - but never destroyed: the next holder of an id finds its stream as it was.
        for (hipStream_t st : stream_pool_) if (st) (void)hipStreamSynchronize(st);
        if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
        for (InputSet* is : in_sets_) {
            if (is->ready) (void)hipEventDestroy(is->ready);
            delete is;
        }
        if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
        for (Slot* s : slots_) {
            for (auto& e : s->graphs) (void)hipGraphExecDestroy(e.second);
            if (s->ev0) (void)hipEventDestroy(s->ev0);
            if (s->ev1) (void)hipEventDestroy(s->ev1);
            if (s->ev2) (void)hipEventDestroy(s->ev2);
            if (s->ev3) (void)hipEventDestroy(s->ev3);
            if (s->h_pinned) (void)hipHostFree(s->h_pinned);
            if (s->side) { (void)hipStreamSynchronize(s->side); (void)hipStreamDestroy(s->side); }
            if (s->ev_acc) (void)hipEventDestroy(s->ev_acc);
            if (s->ev_side) (void)hipEventDestroy(s->ev_side);
            if (s->ev_sync) (void)hipEventDestroy(s->ev_sync);
            delete s;
        }
        if (owns_streams_) for (hipStream_t st : stream_pool_) if (st) (void)hipStreamDestroy(st);
    }

    // ---------------------------------------------------------------------------------------------- NTT runner
    // natural in -> natural out; in != out.  which: 0 = size n, 1 = size 4n.  `count` same-size transforms per launch.
    // sub_log > 0: a transform of 1 / 2^sub_log of the size, on the same twiddle table (sub-coset transforms)
    int run_ntt_batch(hipStream_t st, int which, bool inverse, int count, const Fr* const* ins, Fr* const* outs, const uint32_t* in_lens,
                      uint32_t out_len, const Fr* pre, const Fr* post, const Fr* scale, int sub_log = 0, bool semi = false) {
        Slot* m = gang_member();
        if (m && m->in_gang && st == m->stream && count <= NTT_MAX_BATCH) {     // a merge point of the gang (gang_launch)
            NttReq<Fr> nr{};
            nr.which = which; nr.inverse = inverse; nr.count = count;
            for (int i = 0; i < count; i++) { nr.ins[i] = ins[i]; nr.outs[i] = outs[i]; nr.in_lens[i] = in_lens[i]; }
            nr.out_len = out_len; nr.pre = pre; nr.post = post; nr.scale = scale; nr.sub_log = sub_log; nr.semi = semi;
            GangReq r;
            r.kind = GANG_KIND_NTT; r.args = &nr; r.member = m;
            const int rc = m->lead->gang.meet(m->gang_idx, r, gang_launcher_);
            if (rc != APK_OK) set_error("%s", r.err.c_str());
            return rc;
        }
        return run_ntt_batch_now(st, which, inverse, count, ins, outs, in_lens, out_len, pre, post, scale, sub_log, semi);
    }
    // the transform's twiddle table: tw[j] = w^j R' (FeU records with APK_NTT_TWU)
    const Fr* ntt_table(int which, bool inverse) const {
        if (ntt_twu_) return which ? (inverse ? ptr<Fr>(twi_4n_x_) : ptr<Fr>(tw_4n_x_)) : (inverse ? ptr<Fr>(twi_n_x_) : ptr<Fr>(twu_n_x_));
        return which ? (inverse ? ptr<Fr>(twi_4n_) : ptr<Fr>(tw_4n_)) : (inverse ? ptr<Fr>(twi_n_) : ptr<Fr>(twu_n_));
    }
    // What the sequence takes is ntt_plan.h's decision (ntt_plan), its launches are ntt_run.h's (ntt_launch): here the context's
    // table, the workspace of the slot that owns the stream, the device's load, the path counters and the statistics.
    int run_ntt_batch_now(hipStream_t st, int which, bool inverse, int count, const Fr* const* ins, Fr* const* outs, const uint32_t* in_lens,
                          uint32_t out_len, const Fr* pre, const Fr* post, const Fr* scale, int sub_log = 0, bool semi = false) {
        const int log_n = (which ? (int)log_n_ + 2 : (int)log_n_) - sub_log;
        Slot* owner = nullptr;
        for (Slot* s : slots_) if (s->own_stream == st || (s->side && s->side == st)) owner = s;    // (a gang's stream is its lead's own)
        bool busy_now = false, busy_foreign = false;     // other proofs in flight on the device (the choice of run_msm_body's lean forms); ... of other contexts only
        if (slots_.size() > 2 && ntt_plan_reads_load(log_n)) busy_now = device_load_over(1, &busy_foreign);
        const NttPlanIn in{log_n, count, out_len, sub_log, semi, (uint32_t)sizeof(FeU<FRP>), owner != nullptr, busy_now, busy_foreign};
        const NttPlan plan = ntt_plan(ntt_knobs(), in);
        if (plan.rc != APK_OK) { set_error("%s", plan.message); return plan.rc; }
        NttBatch nb{};
        for (int i = 0; i < count; i++) { nb.in[i] = ins[i]; nb.out[i] = outs[i]; nb.in_len[i] = in_lens[i]; }
        if (plan.needs_wide) for (int i = 0; i < count; i++) nb.wide[i] = ptr<FeU<FRP>>(owner->ntt_wide) + ((size_t)i << log_n);
        static constexpr PathIdx PATH_OF_BIT[] = {P_NTT_SEQ, P_NTT_R4, P_NTT_R4_LOAD, P_DEVICE_LOAD};   // NttPathBit order
        for (uint32_t i = 0; i < sizeof PATH_OF_BIT / sizeof PATH_OF_BIT[0]; i++) if (plan.paths >> i & 1u) path(PATH_OF_BIT[i]);
        Slot* timed = stats_on_ ? owner : nullptr;
        if (timed) HIPCHK(hipEventRecord(timed->ev2, st));
        CHK(ntt_launch<FRP>(st, plan, nb, count, ntt_table(which, inverse), ntt_twu_, pre, post, scale));
        if (timed) {
            HIPCHK(hipEventRecord(timed->ev3, st));
            HIPCHK(hipEventSynchronize(timed->ev3));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, timed->ev2, timed->ev3));
            std::lock_guard<std::mutex> g(stats_mu_);
            stats_.ntt_ms += ms;
            stats_.ntt_elements += ((uint64_t)1 << log_n) * count;
        }
        return APK_OK;
    }
    int run_ntt(hipStream_t st, int which, bool inverse, const Fr* in, Fr* out, uint32_t in_len, uint32_t out_len,
                const Fr* pre, const Fr* post, const Fr* scale, int sub_log = 0, bool semi = false) {
        return run_ntt_batch(st, which, inverse, 1, &in, &out, &in_len, out_len, pre, post, scale, sub_log, semi);
    }
    // evaluations of `count` canonical polynomials on the points of the 4n coset this context stands for: all 4n of them, or -
    // sub-coset split - the m = 4n / G points of class k (cls = 0) or of the class Z(omega X) needs at G = 8 (cls = 1)
    // These are the prover's own evaluations of l, r, o, Z and the BSB22 columns, read by the quotient kernel alone: the whole-coset
    // form leaves them SEMI-CANONICAL (below 2r, kernels_ntt.h NttPassArgs::semi).  The sub-coset form and every transform whose
    // output leaves the prover (apk_ntt, coset_ntt_dev, the setup tables) stay canonical.
    int coset_eval(hipStream_t st, int count, const Fr* const* ins, const uint32_t* lens, Fr* const* outs, int cls = 0) {
        if (!sc_.on()) return run_ntt_batch(st, 1, false, count, ins, outs, lens, n4_, ptr<Fr>(coset_pre_), nullptr, nullptr, 0, true);
        return run_ntt_batch(st, 1, false, count, ins, outs, lens, n4_ >> sc_.glog, ptr<Fr>(sc_.pre[cls]), nullptr, nullptr, sc_.glog);
    }
    int inv_ntt_n(hipStream_t st, const Fr* in, Fr* out) { return run_ntt(st, 0, true, in, out, n_, n_, nullptr, nullptr, ptr<Fr>(scales_)); }
    // evaluations of a canonical polynomial (len coefficients) on the 4n coset
    int coset_ntt_4n(hipStream_t st, const Fr* in, uint32_t len, Fr* out, bool semi = false) {
        return run_ntt(st, 1, false, in, out, len, n4_, ptr<Fr>(coset_pre_), nullptr, nullptr, 0, semi);
    }

    // ---------------------------------------------------------------------------------------------- MSM runner
    // tab_lag_ = plain multiples of the n Lagrange-SRS points (given on the host, or derived from d_srs on the device) + D_0..D_2
    int build_lagrange_table(hipStream_t st, const Aff* d_srs, const void* h_lagrange) {
        DevBuf lag;
        CHK(lag.alloc((size_t)(n_ + 3) * sizeof(Aff)));
        if (h_lagrange) HIPCHK(hipMemcpyAsync(lag.p, h_lagrange, (size_t)n_ * sizeof(Aff), hipMemcpyHostToDevice, st));
        else CHK((g1_to_lagrange_dev<FRP, FPP>(d_srs, n_, ptr<Aff>(lag), st)));
        HIPCHK(hipMemcpyAsync(ptr<Aff>(lag) + n_, lag_dk_, sizeof lag_dk_, hipMemcpyHostToDevice, st));
        CHK((build_tables<FRP, FPP>(st, msm_ctx_, ptr<Aff>(lag), n_ + 3, tab_lag_, /*plain=*/true)));
        HIPCHK(hipStreamSynchronize(st));     // `lag` is released on return
        lag_ready_.store(true, std::memory_order_release);
        return APK_OK;
    }
    bool lagrange_ready() const { return lag_ready_.load(std::memory_order_acquire); }
    // can this context commit over the Lagrange SRS at all (now, or after a lazy derive)?
    bool lagrange_possible() const { return lagrange_ready() || (srs_keep_.p && !lag_failed_.load(std::memory_order_relaxed)); }
    // Best effort: true when the table is there on return.  A failed derive clears the HIP error state and is not retried.
    bool ensure_lagrange_table(hipStream_t st) {
        if (lagrange_ready()) return true;
        std::lock_guard<std::mutex> lk(lag_mu_);
        if (lagrange_ready()) return true;
        if (!srs_keep_.p || lag_failed_.load(std::memory_order_relaxed)) return false;
        const int rc = build_lagrange_table(st, ptr<Aff>(srs_keep_), nullptr);
        if (rc != APK_OK) {
            (void)hipGetLastError();
            tab_lag_.table.release();
            tab_lag_.built = false;
            lag_failed_.store(true, std::memory_order_relaxed);
            (void)hipStreamSynchronize(st);
            srs_keep_.release();
            return false;
        }
        srs_keep_.release();
        return true;
    }

    int run_msm(Slot& s, const MsmTables& T, const MsmBatchArgs& a_in) {
        // whether the scalars leave the Montgomery form in the sort is a property of the TABLE (R^-1 * P or P): derived here, so
        // that no call site can pair a table with the wrong scalar form
        MsmBatchArgs a = a_in;
        a.plain = T.plain ? 1u : 0u;
        if (!msm_knobs().graph || stats_on_) return run_msm_body(s, T, a);
        GraphKey key{};
        key.table = T.table.p; key.a = a;
        for (uint32_t b = a.batch; b < MSM_ARGS_MAX; b++) { key.a.scalars[b] = nullptr; key.a.len[b] = 0; key.a.offset[b] = 0; }
        for (size_t i = 0; i < s.graphs.size(); i++)
            if (s.graphs[i].first == key) {
                if (i) std::swap(s.graphs[i], s.graphs[0]);          // most recently used first
                HIPCHK(hipGraphLaunch(s.graphs[0].second, s.stream));
                s.pending_pts = a.batch;
                return APK_OK;
            }
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamBeginCapture(s.stream, hipStreamCaptureModeThreadLocal));
        const int rc = run_msm_body(s, T, a);
        const hipError_t e = hipStreamEndCapture(s.stream, &g);
        if (rc != APK_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
        HIPCHK(e);
        hipGraphExec_t exec = nullptr;
        HIPCHK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        // bounded: the prover's own four batches hit the same keys every proof; callers with per-call staging pointers
        // (apk_msm_g1_batch_device) would otherwise grow the list without limit.  The evicted exec may still be running on
        // this slot's stream, so the stream is drained before it is destroyed.
        constexpr size_t GRAPH_CACHE = 8;
        if (s.graphs.size() >= GRAPH_CACHE) {
            HIPCHK(hipStreamSynchronize(s.stream));
            (void)hipGraphExecDestroy(s.graphs.back().second);
            s.graphs.pop_back();
        }
        s.graphs.insert(s.graphs.begin(), std::make_pair(key, exec));
        HIPCHK(hipGraphLaunch(exec, s.stream));
        s.pending_pts = a.batch;
        return APK_OK;
    }

    // Plan (msm_plan.h: every decision about the batch), then launch (msm_run.h).  The sums land in the slot's XYZZ result area -
    // the pinned buffer itself where the kernels can write it, else the workspace's result_xyzz and a copy queued behind them;
    // sync_results() makes them affine.  The caller syncs the stream.
    int run_msm_body(Slot& s, const MsmTables& T, const MsmBatchArgs& a) {
        hipStream_t st = s.stream;
        MsmBatchIn in{};
        in.batch = a.batch; in.len = a.len; in.offset = a.offset;
        in.n_bases = T.n_bases; in.ctx_bases = msm_bases_;
        in.simds = simds_; in.slots = (uint32_t)slots_.size();
        if (slots_.size() > 2) in.others_busy = device_load_over(1, &in.others_foreign);
        in.scan_runs = APK_PHASE(32);
        in.ws_batch = ws_batch_;
        in.lt_max = MsmQuad<FPP>::LT;
        in.counts_words = s.msm.counts.bytes / 4; in.sort_tmp_bytes = s.msm.sort_tmp.bytes;
        in.has_sort_tmp = s.msm.sort_tmp.p != nullptr; in.has_ptot2 = s.msm.ptot2.p != nullptr;
        const MsmBatchPlan p = msm_plan_batch(msm_ctx_, msm_knobs(), in);
        static constexpr PathIdx PATH_OF_BIT[] = {P_UNIT_LOADED, P_SMALL_UNITS, P_SORT2, P_SORT2_LOAD, P_SORT_FUSED, P_LEAN_TAIL, P_COMBINE_QUAD, P_ROWCOL_SERIAL, P_DEVICE_LOAD, P_MSM_INPLACE};   // MsmPathBit order
        for (uint32_t i = 0; i < sizeof PATH_OF_BIT / sizeof PATH_OF_BIT[0]; i++) if (p.paths >> i & 1u) path(PATH_OF_BIT[i]);
        if (p.rc == APK_ERR_ARG) { set_error("%s", p.message); return p.rc; }
        if (p.rc == APK_OK) {    // (any other refusal comes back from msm_launch_batch, behind the records in front of the batch)
            path(P_MSM_BATCHES);
            if (s.res_write_off + a.batch > (uint32_t)MSM_ARGS_MAX) { set_error("msm: result area overflow"); return APK_ERR_STATE; }
        }
        Pt* const res_out = s.d_pinned ? pin_dev<Pt>(s.d_pinned, PIN_XYZZ) + s.res_write_off : ptr<Pt>(s.msm.result_xyzz);
        MsmEvents ev;
        if (stats_on_) { ev.before = s.ev0; ev.scanned = s.ev2; ev.accumulated = s.ev3; ev.reduced = s.ev1; }
        ev.acc = s.ev_acc; ev.mark_acc = s.mark_acc;
        CHK((msm_launch_batch<FRP, FPP>(st, msm_ctx_, s.msm, ptr<Aff>(T.table), T.n_bases, a, p, res_out, ev)));
        if (!s.d_pinned) HIPCHK(hipMemcpyAsync(pin_host<Pt>(s.h_pinned, PIN_XYZZ) + s.res_write_off, s.msm.result_xyzz.p, a.batch * sizeof(Pt), hipMemcpyDeviceToHost, st));
        s.pending_pts = a.batch;
        if (stats_on_) {
            HIPCHK(hipEventSynchronize(s.ev1));
            float tot = 0, acc = 0, srt = 0, tail = 0;
            HIPCHK(hipEventElapsedTime(&tot, s.ev0, s.ev1));
            HIPCHK(hipEventElapsedTime(&acc, s.ev2, s.ev3));
            HIPCHK(hipEventElapsedTime(&srt, s.ev0, s.ev2));
            HIPCHK(hipEventElapsedTime(&tail, s.ev3, s.ev1));
            std::lock_guard<std::mutex> g(stats_mu_);
            stats_.msm_sort_ms += srt;
            stats_.msm_tail_ms += tail;
            stats_.msm_total_ms += tot;
            stats_.msm_batches += 1;
            stats_.msm_accumulate_ms += acc;
            stats_.msm_accumulate_launches += 1;
            for (uint32_t b = 0; b < a.batch; b++) stats_.msm_pairs += a.len[b];
        }
        return APK_OK;
    }

    static Slot*& hook_slot() { static thread_local Slot* p = nullptr; return p; }

    // A commitment batch of the prover.  Without a hook: run_msm on this GPU.  With one (the
    // independent commitments of ONE proof dealt to several GPUs) the batch is parked and handed to the hook at the next
    // sync_results(), after the stream has produced the scalar vectors - the launches queued in between (coset NTTs ...) run
    // on this GPU while the other GPUs commit.
    int commit(Slot& s, const MsmTables& T, int basis, const MsmBatchArgs& a) {
        if (!hook_ && s.in_gang) {      // a merge point of the gang: ONE launch sequence for every member's batch (gang_launch)
            MsmReq mr{&T, a};
            GangReq r;
            r.kind = GANG_KIND_MSM; r.args = &mr; r.member = &s;
            const int rc = s.lead->gang.meet(s.gang_idx, r, gang_launcher_);
            if (rc != APK_OK) set_error("%s", r.err.c_str());     // (the launch ran on another member's thread)
            return rc;
        }
        if (!hook_) return run_msm(s, T, a);
        for (uint32_t b = 0; b < a.batch; b++)
            if (a.len[b] > T.n_bases || a.offset[b] > T.n_bases - a.len[b]) { set_error("msm: %u scalars exceed the %u bases", a.len[b], T.n_bases); return APK_ERR_ARG; }
        s.hook_pending = true; s.hook_basis = basis; s.hook_args = a;
        s.hook_args.plain = T.plain ? 1u : 0u;
        return APK_OK;
    }

    // stream sync + affine conversion of the MSM sums run_msm left in the pinned buffer (results land at h_pinned[0..])
    // ---- tail filling --------------------------------------------------------------------------------------------------------
    // A lone proof spends a fifth of its time in the reduction tails of its four commitment batches (combine, row/column sums,
    // bit sums + final scaling: ~210 us per batch on a few hundred waves), and the launches queued behind a batch - the 4n coset
    // transforms of the polynomials just committed - wait for the tail although they need neither its result nor its SIMDs.  When
    // this proof is the only one in flight they go to a second stream gated on an event recorded right behind the accumulate
    // kernel, so they start when the VALU-bound part of the MSM is over, not before (ungated, round 3's first attempt, they
    // only slowed the accumulate kernel down by what they gained).  With several proofs in flight other proofs fill the tails
    // and a second stream per slot costs throughput (-8 % with 16 slots), so the choice is made per proof.
    int tail_fill(Slot& s) {
        const int on = prover_knobs().tail_fill;
        const int graphs = msm_knobs().graph;
        if (!on || graphs || hook_ || wire_hook_ || stats_on_ || !qk_direct_ || sc_.on()) return 0;
        if (gate_.load() != 1) return 0;      // (the DEVICE has one proof in flight: this one)
        if (!s.side) {
            // lowest priority: the tail kernels on the main stream are the critical path, the transforms only have to be done
            // by the time the next round's challenge is known
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (hipStreamCreateWithPriority(&s.side, hipStreamNonBlocking, least) != hipSuccess) { s.side = nullptr; return 0; }
            if (hipEventCreateWithFlags(&s.ev_acc, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&s.ev_side, hipEventDisableTiming) != hipSuccess) return 0;
        }
        return s.ev_acc && s.ev_side ? on : 0;
    }
    int side_begin(Slot& s) { HIPCHK(hipStreamWaitEvent(s.side, s.ev_acc, 0)); return APK_OK; }
    int side_end(Slot& s) { HIPCHK(hipEventRecord(s.ev_side, s.side)); s.side_pending = true; return APK_OK; }

    // Wait for the slot's stream.  hipStreamSynchronize spins on the host (ROCm's default with many CPUs visible): right for a lone
    // proof (its six waits are on the critical path), wrong when 16 proving threads spin at once - on the GPU boxes of this build
    // the container's CPU quota is 16 cores for 256 visible CPUs, and N ranks of an N-GPU node share whatever the node grants.
    // With other proofs in flight the thread therefore sleeps between polls of an event (the wake-up latency hides behind the
    // other proofs).
    int wait_stream(Slot& s) {
        // mode: -1 by load (default: sleep-and-poll with other proofs in flight, spin alone), 0 always spin, 1 hipEventSynchronize on a
        // hipEventBlockingSync event, 2 always sleep-and-poll.
        // Round 6: the "blocking" event wait of rounds 3-5 does NOT give the CPU back on this runtime - a loaded context burned one
        // core per proof in flight (17.6 cores for 16 proofs: bench.py host_cpu_timed_region), i.e. the whole 16-CPU quota of the
        // boxes, and with 32 proofs in flight (gangs) the cgroup froze the process for most of every period.  So with other proofs
        // in flight the thread now polls the event and SLEEPS in between (the wake-up hides behind the other proofs).
        static const int mode = env_int("APK_SYNC_BLOCKING", -1, -1, 2);
        static const int poll_us = env_int("APK_SYNC_POLL_US", 50, 1, 10000);
        const bool loaded = slots_.size() > 2 && device_load_over(2);
        if (s.ev_sync && (mode == 2 || (mode < 0 && loaded))) {
            HIPCHK(hipEventRecord(s.ev_sync, s.stream));
            for (;;) {
                const hipError_t e = hipEventQuery(s.ev_sync);
                if (e == hipSuccess) return APK_OK;
                if (e != hipErrorNotReady) { (void)hipGetLastError(); set_error("hipEventQuery: %s", hipGetErrorString(e)); return APK_ERR_HIP; }
                struct timespec ts = {0, (long)poll_us * 1000L};
                nanosleep(&ts, nullptr);
            }
        }
        if (mode == 1 && s.ev_sync) {
            HIPCHK(hipEventRecord(s.ev_sync, s.stream));
            HIPCHK(hipEventSynchronize(s.ev_sync));
            return APK_OK;
        }
        HIPCHK(hipStreamSynchronize(s.stream));
        return APK_OK;
    }

    int sync_results(Slot& s) {
        if (s.in_gang) {     // the launches this member recorded since its last merge point go out now, with the other members'
            GangReq r;
            r.kind = GANG_KIND_FLUSH; r.member = &s;
            const int rc = s.lead->gang.meet(s.gang_idx, r, gang_launcher_);
            if (rc != APK_OK) { set_error("%s", r.err.c_str()); return rc; }
        }
        CHK(wait_stream(s));
        // whatever the main stream is handed from here on runs behind the side stream's transforms
        if (s.side_pending) { s.side_pending = false; HIPCHK(hipStreamWaitEvent(s.stream, s.ev_side, 0)); }
        if (s.hook_pending) {
            s.hook_pending = false;
            const MsmBatchArgs& a = s.hook_args;
            uint8_t pts[MSM_MAX_BATCH * sizeof(Aff)];
            // the hook's own share of the batch comes back in through apk_msm_g1_batch_device on this thread: it runs on THIS
            // slot (idle now: the stream was just synchronised and the parked batch never touched the MSM workspace) instead
            // of waiting for a free one - with one slot it would wait for itself
            hook_slot() = &s;
            const int rc = hook_(hook_user_, s.hook_basis, a.batch, a.scalars, a.len, pts);
            hook_slot() = nullptr;
            if (rc != APK_OK) { set_error("commit hook failed with %d", rc); return rc == APK_ERR_ARG ? APK_ERR_ARG : APK_ERR_STATE; }
            memcpy(pin_host<Aff>(s.h_pinned, PIN_AFF), pts, a.batch * sizeof(Aff));
            s.pending_pts = 0;
            return APK_OK;
        }
        // (a gang's merged batch left its sums in the LEAD's buffer; this proof's start at res_off)
        const Slot& from = s.lead ? *s.lead : s;
        const Pt* g = pin_host<Pt>(from.h_pinned, PIN_XYZZ) + s.res_off;
        // one shared inversion: 3 of 4 host inversions of ~5 us leave the gap between a batch's results and the next round's launches
        static_assert(MSM_MAX_BATCH <= HOST_AFFINE_BATCH, "a proof's batch of sums is one batch conversion");
        host_xyzz_batch_to_affine<FPP>(g, s.pending_pts, pin_host<Aff>(s.h_pinned, PIN_AFF));
        s.pending_pts = 0;
        return APK_OK;
    }

    int alloc_slot(Slot& s) {
        s.lead = &s;
        HIPCHK(hipEventCreate(&s.ev0));
        HIPCHK(hipEventCreate(&s.ev1));
        HIPCHK(hipEventCreate(&s.ev2));
        HIPCHK(hipEventCreate(&s.ev3));
        if (hipEventCreateWithFlags(&s.ev_sync, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); s.ev_sync = nullptr; }
        HIPCHK(hipHostMalloc(&s.h_pinned, PIN_BYTES, hipHostMallocDefault));
        memset(s.h_pinned, 0, PIN_BYTES);   // (the tail-flag word is only ever written by a failing proof)
        // MSM sums and evaluations are a few hundred bytes behind a chain of kernels: the kernel that produces them writes them
        // straight into this (coherent, device-visible) host buffer instead of a device buffer + a copy launch - one launch less
        // per batch, and under load every launch of a proof's chain waits ~0.1 ms for its turn.  APK_ZERO_COPY=0: device buffer + copy.
        static const int zero_copy = env_int("APK_ZERO_COPY", 1, 0, 1);
        if (zero_copy) {
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, s.h_pinned, 0) == hipSuccess) s.d_pinned = static_cast<uint8_t*>(dp);
            else (void)hipGetLastError();
        }
        const size_t fn = (size_t)n_ * sizeof(Fr), fn3 = (size_t)(n_ + 4) * sizeof(Fr), f4 = (size_t)n4_ * sizeof(Fr);
        if (msm_only_) {
            CHK(s.scratch_in.alloc((size_t)msm_bases_ * sizeof(Fr)));
            return s.msm.alloc(msm_ctx_, msm_knobs(), msm_bases_, 1, many_slots_);
        }
        CHK(s.wl.alloc(fn3)); CHK(s.wr.alloc(fn3)); CHK(s.wo.alloc(fn3));   // n values + the blinding scalars of a Lagrange-basis commitment
        CHK(s.cl.alloc(fn3)); CHK(s.cr.alloc(fn3)); CHK(s.co.alloc(fn3)); CHK(s.cz.alloc(fn3));
        for (DevBuf* b : {&s.cl, &s.cr, &s.co, &s.cz}) HIPCHK(hipMemset(b->p, 0, fn3));
        CHK(s.qk_lag.alloc(fn)); CHK(s.qk_can.alloc(fn));
        CHK(s.ratio.alloc(fn)); CHK(s.zlag.alloc(fn));
        CHK(s.scan_tot.alloc((size_t)(2 * (cdiv(n_ + 4, SCAN_BLOCK) + 1) + 2) * sizeof(Fr)));
        CHK(s.el.alloc(f4)); CHK(s.er.alloc(f4)); CHK(s.eo.alloc(f4)); CHK(s.ez.alloc(f4)); CHK(s.eqk.alloc(f4));
        CHK(s.quot.alloc(f4)); CHK(s.hcan.alloc(f4));
        CHK(s.pw_z.alloc(fn3)); CHK(s.pw_zi.alloc(fn3)); CHK(s.pw_zw.alloc(fn3)); CHK(s.pw_zwi.alloc(fn3));
        CHK(s.tmp2.alloc(fn3)); CHK(s.folded.alloc(fn3)); CHK(s.tmp.alloc(fn3)); CHK(s.q1.alloc(fn3)); CHK(s.q2.alloc(fn3));
        CHK(s.eval_partial.alloc((size_t)EVAL_MAX * cdiv(n_ + 4, EVAL_BLOCK) * sizeof(Fr)));
        CHK(s.eval_result.alloc(EVAL_MAX * sizeof(Fr)));
        for (uint32_t k = 0; k < nb_commit_; k++) { CHK(s.pi2_can[k].alloc(fn)); CHK(s.epi2[k].alloc(f4)); }
        CHK(s.scratch_in.alloc(f4));
        CHK(s.tail_flag.alloc(16));
        HIPCHK(hipMemset(s.tail_flag.p, 0, 16));
        CHK(s.ntt_wide.alloc((size_t)NTT_MAX_BATCH * gang_cap_ * n4_ * sizeof(FeU<FRP>)));
        return s.msm.alloc(msm_ctx_, msm_knobs(), msm_bases_, ws_batch_, many_slots_);
    }

    // ---- host-input staging sets (see InputSet) ---------------------------------------------------------------------------------
    int ensure_input_sets() {
        std::lock_guard<std::mutex> lk(mu_);
        if (!in_sets_.empty()) return APK_OK;
        // as many sets again as proving slots (callers waiting for a slot have their upload in flight), at most 64 - the most
        // callers a context proves for at a time (16 streams of four)
        static const int sets_env = env_int("APK_INPUT_SETS", 0, 0, 128);
        size_t count = sets_env ? (size_t)sets_env : 2 * slots_.size();
        if (count > 64 && !sets_env) count = 64;
        if (count < 1) count = 1;
        if (!copy_stream_) HIPCHK(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking));
        std::vector<InputSet*> made;
        int rc = APK_OK;
        for (size_t i = 0; i < count && rc == APK_OK; i++) {
            InputSet* is = new InputSet();
            is->index = i;
            made.push_back(is);
            rc = alloc_input_set(*is);
        }
        if (rc != APK_OK && made.size() > 1) {       // out of memory half way: keep the sets that were completed
            InputSet* last = made.back();
            made.pop_back();
            if (last->ready) (void)hipEventDestroy(last->ready);
            delete last;
            (void)hipGetLastError();
            rc = APK_OK;
        }
        if (rc != APK_OK) { for (InputSet* is : made) delete is; return rc; }
        in_sets_ = made;
        in_gate_.resize(in_sets_.size());
        return APK_OK;
    }
    int alloc_input_set(InputSet& is) {
        const size_t fn3 = (size_t)(n_ + 4) * sizeof(Fr);
        for (int j = 0; j < 3; j++) CHK(is.w[j].alloc(fn3));
        for (uint32_t k = 0; k < nb_commit_; k++) CHK(is.pi2[k].alloc(fn3));
        is.copy = copy_stream_;
        HIPCHK(hipEventCreateWithFlags(&is.ready, hipEventDisableTiming));
        return APK_OK;
    }
    struct InputGuard {
        CurveBackend* b; InputSet* set = nullptr; bool ok = false;
        explicit InputGuard(CurveBackend* b_) : b(b_) {}
        int take() {
            CHK(b->ensure_input_sets());
            set = b->in_sets_[b->in_gate_.acquire().slot];
            return APK_OK;
        }
        ~InputGuard() {
            if (!set) return;
            // an error return may leave copies or kernels in flight that still read the caller's buffers / this set
            if (!ok) (void)hipDeviceSynchronize();
            b->in_gate_.release(set->index);
        }
    };

    // ---- deferred launches of a gang member (gang_run.h) -------------------------------------------------------------------------
    // Every element-wise / scan / reduction kernel of the prover goes through klaunch().  Alone, it is an ordinary launch.  As a
    // gang member (with the zero-copy result buffer: nothing but kernels then touches the stream between two merge points) it is
    // RECORDED - grid, block, the arguments by value - and launched at the member's next merge point or stream wait, together with
    // the same kernel of the other members: ONE launch, blockIdx.z = member (gang_flush).
    template <class K, int BOUNDS, class... P>
    int klaunch(hipStream_t st, dim3 grid, dim3 block, size_t lds, P... p) {
        Slot* m = gang_member();
        static const int defer = env_int("APK_GANG_DEFER", 1, 0, 1);
        if (defer && m && m->in_gang && m->d_pinned && st == m->stream && grid.z == 1) {
            m->cmds.template record<K, BOUNDS, P...>(grid, block, lds, p...);
            return APK_OK;
        }
        poly1_kernel<K, BOUNDS, P...><<<grid, block, lds, st>>>(p...);
        KCHK();
        return APK_OK;
    }
    // the launcher poly_run.h's sequences take: klaunch
    struct KLaunch {
        CurveBackend* b;
        template <class K, int BOUNDS, class... P>
        int go(hipStream_t st, dim3 grid, dim3 block, size_t lds, P... p) const { return b->template klaunch<K, BOUNDS, P...>(st, grid, block, lds, p...); }
    };
    KLaunch kl() { return KLaunch{this}; }

    // ---- gangs (gang.h) ----------------------------------------------------------------------------------------------------------
    static int choose_gang(int log_n, int nslots, int max_slots) {
        const int env = env_int("APK_GANG", 0, 0, GANG_MAX);
        if (nslots <= max_slots) return 1;            // every caller gets a stream of its own
        if (env) return env;
        // Same box, 32 / 64 persistent callers with distinct witnesses (tools/sweep_gangs.sh, profiles/r06_gang_sweep.txt), proofs/s
        // alone -> gangs of 2 (32 callers) -> gangs of 4 (64 callers):
        //   BN254 2^13  2 175 -> . -> 3 846     BN254 2^15  1 499 -> 1 763 -> 1 825     BLS12-381 2^14  1 376 -> 1 604 -> 1 746 .. 1 775
        //   BN254 2^16    958 -> 1 033 -> 1 026   BN254 2^17  538 -> 539 (VALU-bound: nothing left for wider launches to fill)
        //   BLS12-381 2^15  852 -> 933 -> 961;  BLS12-381 2^16  501.6 -> 497.4 with pairs (neutral: off);  BN254 2^14  1 997 -> 2 704 -> 3 029
        return log_n <= 15 ? 4 : (log_n == 16 && FPP::N <= 8) ? 2 : 1;
    }
    static Slot*& gang_member() { static thread_local Slot* p = nullptr; return p; }
    bool gangs_allowed() const {
        const int graphs = msm_knobs().graph;
        return gang_cap_ > 1 && !hook_ && !wire_hook_ && !sc_.on() && !stats_on_ && !graphs;
    }
    // a proof's slot, alone or as a member of a gang
    struct MemberGuard {
        CurveBackend* b; Slot* s; bool ok = false;
        explicit MemberGuard(CurveBackend* b_) : b(b_) {
            const SlotGate::Ticket t = b->gate_.acquire_member(b->gangs_allowed());
            s = b->slots_[t.slot];
            Slot* lead = b->slots_[t.lead];
            s->lead = lead; s->gang_idx = t.idx; s->in_gang = t.size > 1; s->res_off = 0;
            if (lead == s) s->own_stream = b->stream_pool_[(size_t)t.stream];
            s->stream = b->stream_pool_[(size_t)t.stream];
            if (s->in_gang) { lead->gang.enter(t.gen, t.size); gang_member() = s; b->path(P_GANG_PROOFS); }
        }
        ~MemberGuard() {
            // an error return may leave this proof's launches in flight on its (or its gang's) stream: nobody may get this workspace
            // before them - and the next holder may well get ANOTHER stream, so stream order alone does not see to it
            if (!ok) b->drain(s);
            if (s->in_gang) {
                gang_member() = nullptr;
                Slot* lead = s->lead;
                lead->gang.leave(s->gang_idx);
                if (lead == s) lead->gang.wait_empty();       // the others run on this slot's stream and MSM workspace
            }
            s->lead = s; s->in_gang = false; s->res_off = 0;
            s->cmds.clear();
            b->release(s, /*ok=*/true);      // (drained above where it had to be)
        }
    };
    // The merged launches of one meeting (called once, by the last member to arrive).  gang_plan.h decides which requests share a
    // launch sequence and where every member's operands and sums sit; here the plan's groups become run_msm / run_ntt_batch_now
    // calls on the lead's stream and workspace.
    static Slot& member_of(const GangReq* r) { return *static_cast<Slot*>(r->member); }
    static const MsmReq& msm_of(const GangReq* r) { return *static_cast<const MsmReq*>(r->args); }
    static const NttReq<Fr>& ntt_of(const GangReq* r) { return *static_cast<const NttReq<Fr>*>(r->args); }
    void gang_launch(GangReq* const* reqs, int count) {
        // 1. the plan
        GangPlanReq pr[GANG_MAX];
        GangRecorder* recs[GANG_MAX];
        for (int i = 0; i < count; i++) {
            pr[i] = reqs[i]->kind == GANG_KIND_MSM ? msm_of(reqs[i]).plan_req() : reqs[i]->kind == GANG_KIND_NTT ? ntt_of(reqs[i]).plan_req() : GangPlanReq{GANG_KIND_FLUSH, 0, nullptr, GangNttShape{}};
            recs[i] = &member_of(reqs[i]).cmds;
        }
        const GangPlan plan = gang_plan_meeting(pr, count, ws_batch_, (uint32_t)(NTT_MAX_BATCH * gang_cap_));
        // 2. first what the members recorded on their way here (the kernels in front of this merge point), merged
        int merged = 0;
        const int frc = gang_flush(recs, count, member_of(reqs[0]).stream, &merged);
        for (int i = 0; i < merged; i++) path(P_GANG_KERNELS);
        if (frc != APK_OK) {
            for (int i = 0; i < count; i++) { reqs[i]->rc = frc; reqs[i]->err = apk_last_error(); }
            return;
        }
        for (int i = 0; i < count; i++) if (reqs[i]->kind == GANG_KIND_FLUSH) reqs[i]->rc = APK_OK;
        // 3. one launch sequence per group, on the lead's stream and workspace: member k's operands from first[k] on
        for (int gi = 0; gi < plan.groups; gi++) {
            const GangGroup& g = plan.group[gi];
            Slot& lead = *member_of(reqs[g.req[0]]).lead;
            int rc;
            if (g.kind == GANG_KIND_MSM) {
                MsmBatchArgs c{};
                c.batch = g.total;
                for (int k = 0; k < g.n; k++) {
                    const MsmBatchArgs& a = msm_of(reqs[g.req[k]]).a;
                    for (uint32_t b = 0; b < a.batch; b++) { c.scalars[g.first[k] + b] = a.scalars[b]; c.len[g.first[k] + b] = a.len[b]; c.offset[g.first[k] + b] = a.offset[b]; }
                    member_of(reqs[g.req[k]]).res_off = g.res_off(k);
                }
                const uint32_t lead_pending = lead.pending_pts;       // (run_msm counts the whole sequence as the workspace owner's)
                lead.res_write_off = g.res_base;
                rc = run_msm(lead, *msm_of(reqs[g.req[0]]).T, c);
                lead.res_write_off = 0;
                lead.pending_pts = lead_pending;
                if (g.n > 1) path(P_GANG_MSM);
                for (int k = 0; k < g.n; k++) member_of(reqs[g.req[k]]).pending_pts = rc == APK_OK ? msm_of(reqs[g.req[k]]).a.batch : 0;
            } else {
                const Fr* ins[NTT_ARGS_MAX]; Fr* outs[NTT_ARGS_MAX]; uint32_t lens[NTT_ARGS_MAX];
                for (int k = 0; k < g.n; k++) {
                    const NttReq<Fr>& m = ntt_of(reqs[g.req[k]]);
                    for (int t = 0; t < m.count; t++) { ins[g.first[k] + t] = m.ins[t]; outs[g.first[k] + t] = m.outs[t]; lens[g.first[k] + t] = m.in_lens[t]; }
                }
                const NttReq<Fr>& f = ntt_of(reqs[g.req[0]]);
                rc = run_ntt_batch_now(lead.own_stream, f.which, f.inverse, (int)g.total, ins, outs, lens, f.out_len, f.pre, f.post, f.scale, f.sub_log, f.semi);
                if (g.n > 1) path(P_GANG_NTT);
            }
            // 4. the group's members get its outcome (the launch ran on one member's thread: the error text travels with rc)
            for (int k = 0; k < g.n; k++) { reqs[g.req[k]]->rc = rc; if (rc != APK_OK) reqs[g.req[k]]->err = apk_last_error(); }
        }
    }

    Slot* acquire() {
        const SlotGate::Ticket t = gate_.acquire();
        Slot* s = slots_[t.slot];
        s->own_stream = s->stream = stream_pool_[(size_t)t.stream];
        return s;
    }
    // wait for whatever the slot's holder has queued: its stream and, with a fill pending, its side stream
    void drain(Slot* s) {
        if (s->stream) (void)hipStreamSynchronize(s->stream);
        if (s->side_pending && s->side) { (void)hipStreamSynchronize(s->side); s->side_pending = false; }
        (void)hipGetLastError();
    }
    // ok = false: the holder returns an error and may have launches in flight.  The slot's next holder can get a different stream
    // (ids are handed out per ticket, device-wide) and would race with them on this workspace: they are waited for here.
    void release(Slot* s, bool ok) {
        if (!ok) drain(s);
        // a side-stream launch still pending at a regular return: whoever gets the STREAM next is ordered behind it
        if (s->side_pending) { s->side_pending = false; if (s->own_stream) (void)hipStreamWaitEvent(s->own_stream, s->ev_side, 0); }
        s->own_stream = s->stream = nullptr;      // (the workspace lookup by stream must only ever find the slot that holds it now)
        gate_.release(s->index);
    }
    struct SlotGuard {
        CurveBackend* b; Slot* s; bool ok = false;     // ok: set by the holder once everything it queued has been waited for
        SlotGuard(CurveBackend* b_) : b(b_), s(b_->acquire()) {}
        ~SlotGuard() { b->release(s, ok); }
    };
    // for the calls a hook of this context makes back into it (hook_slot()): the prover's own slot, idle while its hook runs, else an acquired one
    struct MaybeGuard {
        CurveBackend* b; Slot* s; bool owned; bool ok = false;
        static Slot* own(CurveBackend* b) { return std::count(b->slots_.begin(), b->slots_.end(), hook_slot()) ? hook_slot() : nullptr; }   // the hook's slot, when the hook is THIS context's
        MaybeGuard(CurveBackend* b_) : b(b_), s(own(b_)), owned(s == nullptr) { if (owned) s = b->acquire(); }
        ~MaybeGuard() { if (owned) b->release(s, ok); }
    };
    static bool is_device_ptr(const void* p) {       // (a pointer the runtime does not know leaves an error behind: cleared)
        hipPointerAttribute_t at{};
        const bool dev = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice;
        if (!dev) (void)hipGetLastError();
        return dev;
    }

    int powers(hipStream_t st, Fr* out, uint32_t count, const Fr& w, const Fr& scale) {
        PowersBatch<FRP> pb{};
        pb.out[0] = out; pb.w[0] = w; pb.scale[0] = scale;
        return klaunch<PowersK<FRP>, 256>(st, dim3(cdiv(cdiv(count, 8), 256), 1), 256, 0, pb, count);
    }
    int powers_batch(hipStream_t st, int k, Fr* const* outs, const Fr* ws, uint32_t count) {
        PowersBatch<FRP> pb{};
        for (int i = 0; i < k; i++) { pb.out[i] = outs[i]; pb.w[i] = ws[i]; pb.scale[i] = Fr::one(); }
        return klaunch<PowersK<FRP>, 256>(st, dim3(cdiv(cdiv(count, 8), 256), k), 256, 0, pb, count);
    }

    // the context's window and sort layout: msm_plan.h (msm_plan_context) decides, from the knobs as they are now
    int choose_window(int requested, int log_size, int slots = 1) {
        msm_ctx_ = msm_plan_context(FRP::BITS, FPP::N, msm_bases_, log_size, slots, requested, msm_knobs_from_env());
        if (msm_ctx_.rc != APK_OK) { set_error("%s", msm_ctx_.message); return msm_ctx_.rc; }
        return APK_OK;
    }

    // ---------------------------------------------------------------------------------------------- init
    // MSM-only context: SRS tables + one MSM workspace per slot, no circuit (single sharded MSM, BASELINE config 4)
    int init_msm_only(int device, const void* bases, uint64_t count, int msm_window) override {
        if (!bases || count == 0 || count >= (1ull << 27)) { set_error("msm context: bad base count"); return APK_ERR_ARG; }
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0) { set_error("no HIP device available (%s); libapk has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e)); return APK_ERR_HIP; }
        if (device < 0 || device >= ndev) { set_error("device %d out of range (%d devices)", device, ndev); return APK_ERR_ARG; }
        device_ = device;
        HIPCHK(hipSetDevice(device_));
        { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_) == hipSuccess && cus > 0) simds_ = 4u * (uint32_t)cus; }
        msm_only_ = true;
        ws_batch_ = 1;             // (alloc_slot sizes an MSM-only context's workspace for one MSM at a time)
        msm_bases_ = (uint32_t)count;
        n_ = (uint32_t)count;
        int lg = 0;
        while ((1ull << lg) < count) lg++;
        CHK(choose_window(msm_window, lg));
        CHK(set_sort_lds_limits<FRP>(msm_ctx_));
        DevBuf srs;
        CHK(srs.alloc(count * sizeof(Aff)));
        HIPCHK(hipMemcpy(srs.p, bases, count * sizeof(Aff), hipMemcpyHostToDevice));
        CHK((build_tables<FRP, FPP>(nullptr, msm_ctx_, ptr<Aff>(srs), (uint32_t)count, tab_can_)));
        HIPCHK(hipDeviceSynchronize());
        Slot* s = new Slot();
        s->index = slots_.size();
        slots_.push_back(s);
        CHK(take_stream_pool(1));
        gate_.resize(slots_.size());
        CHK(alloc_slot(*s));
        return APK_OK;
    }

    // The context's view of the proving streams.  With the device-wide scheduler (the default): the device's own streams, borrowed,
    // and the gate attached to the device's scheduler.  APK_DEVICE_SCHED=0: `own_count` streams of the context's own.
    int take_stream_pool(int own_count) {
        DeviceSched* sched = device_sched_for(device_);
        if (sched) {
            void* st[64];
            int count = 0;
            CHK(device_stream_pool(device_, st, 64, &count));
            for (int i = 0; i < count; i++) stream_pool_.push_back(static_cast<hipStream_t>(st[i]));
            owns_streams_ = false;
            gate_.attach(sched);
            return APK_OK;
        }
        owns_streams_ = true;
        for (int i = 0; i < own_count; i++) {
            hipStream_t ps = nullptr;
            HIPCHK(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
            stream_pool_.push_back(ps);
        }
        return APK_OK;
    }

    int init(const apk_circuit_desc* d) override {
        if (d->n < 8 || (d->n & (d->n - 1)) || d->n > (1ull << 24)) { set_error("n=%llu must be a power of two in [8, 2^24]", (unsigned long long)d->n); return APK_ERR_ARG; }
        if (d->nb_commitments > APK_MAX_COMMITMENTS) { set_error("at most %d BSB22 commitments", APK_MAX_COMMITMENTS); return APK_ERR_ARG; }
        if (!d->srs_g1 || !d->ql || !d->qr || !d->qm || !d->qo || !d->qk || !d->perm) { set_error("null circuit pointer"); return APK_ERR_ARG; }
        if (d->nb_commitments && !d->srs_g1_lagrange) { set_error("BSB22 commitments need the Lagrange SRS"); return APK_ERR_ARG; }
        if (d->nb_public > d->n) { set_error("nb_public > n"); return APK_ERR_ARG; }
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0) { set_error("no HIP device available (%s); libapk has no CPU fallback", e == hipSuccess ? "0 devices" : hipGetErrorString(e)); return APK_ERR_HIP; }
        if (d->device < 0 || d->device >= ndev) { set_error("device %d out of range (%d devices)", d->device, ndev); return APK_ERR_ARG; }
        device_ = d->device;
        HIPCHK(hipSetDevice(device_));
        { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_) == hipSuccess && cus > 0) simds_ = 4u * (uint32_t)cus; }
        n_ = (uint32_t)d->n;
        n4_ = 4 * n_;
        log_n_ = 0;
        while ((1u << log_n_) < n_) log_n_++;
        nb_public_ = d->nb_public;
        nb_commit_ = d->nb_commitments;
        for (uint32_t k = 0; k < nb_commit_; k++) {
            cci_[k] = d->commitment_constraint_index[k];
            // the prover writes the commitment's hash into row nb_public + cci of Qk: must be a row of the domain on every path
            if ((uint64_t)nb_public_ + cci_[k] >= n_) { set_error("commitment_constraint_index[%u] = %u: row %llu is outside the domain (n = %u)", k, cci_[k], (unsigned long long)nb_public_ + cci_[k], n_); return APK_ERR_ARG; }
        }
        msm_bases_ = n_ + 3;
        CHK(choose_window(d->msm_window, (int)log_n_, d->slots));
        // domain constants on the host (gnark fft.NewDomain [UPSTREAM]; generator = VK Generator,
        // templateLogicSigBN254.go:57; shift = VK CosetShift :68)
        Fr root = root_of_unity();
        const int adicity = FRP::ADICITY;
        omega4_ = root;
        for (int i = 0; i < adicity - (int)log_n_ - 2; i++) omega4_ = Fr::sqr(omega4_);
        omega_ = Fr::sqr(Fr::sqr(omega4_));
        omega_inv_ = Fr::inv(omega_);
        omega4_inv_ = Fr::inv(omega4_);
        shift_ = fr_u64(FRP::COSET_SHIFT);
        shift_inv_ = Fr::inv(shift_);
        n_inv_ = Fr::inv(fr_u64(n_));
        n4_inv_ = Fr::inv(fr_u64(n4_));
        {   // 1/(x^n - 1) on the 4n coset takes four values: x^n = shift^n * i^k, i = omega4^n
            Fr sn = Fr::pow_u64(shift_, n_);
            Fr i4 = Fr::pow_u64(omega4_, n_);
            Fr cur = sn;
            for (int k = 0; k < 4; k++) { zh_inv_[k] = Fr::inv(cur - Fr::one()); cur = cur * i4; }
        }
        hipStream_t st = nullptr;  // default stream during setup
        const size_t fn = (size_t)n_ * sizeof(Fr), f4 = (size_t)n4_ * sizeof(Fr);
        CHK(tw_n_.alloc(fn / 2)); CHK(twi_n_.alloc(fn / 2)); CHK(tw_4n_.alloc(f4 / 2)); CHK(twi_4n_.alloc(f4 / 2));
        const Fr ru = fr_u64(32);   // R'/R = 2^5: x R -> x R'
        CHK(ntt_allow_tile_lds<FRP>());
        CHK(twu_n_.alloc(fn / 2));
        CHK(powers(st, ptr<Fr>(tw_n_), n_ / 2, omega_, Fr::one()));
        CHK(powers(st, ptr<Fr>(twu_n_), n_ / 2, omega_, ru));
        CHK(powers(st, ptr<Fr>(twi_n_), n_ / 2, omega_inv_, ru));
        CHK(powers(st, ptr<Fr>(tw_4n_), n4_ / 2, omega4_, ru));
        CHK(powers(st, ptr<Fr>(twi_4n_), n4_ / 2, omega4_inv_, ru));
        if (env_int("APK_NTT_TWU", 0, 0, 1)) {     // measured neutral (profiles/r06_ntt_twiddles.txt): off
            struct { DevBuf* in; DevBuf* out; uint32_t count; } tabs[4] = {{&twu_n_, &twu_n_x_, n_ / 2}, {&twi_n_, &twi_n_x_, n_ / 2},
                                                                            {&tw_4n_, &tw_4n_x_, n4_ / 2}, {&twi_4n_, &twi_4n_x_, n4_ / 2}};
            for (auto& t : tabs) {
                CHK(t.out->alloc((size_t)t.count * sizeof(FeU<FRP>)));
                unpack_table_kernel<FRP><<<cdiv(t.count, 256), 256, 0, st>>>(ptr<Fr>(*t.in), ptr<FeU<FRP>>(*t.out), t.count);
                KCHK();
            }
            ntt_twu_ = true;
        }
        CHK(coset_pre_.alloc((size_t)(n_ + 4) * sizeof(Fr)));
        CHK(powers(st, ptr<Fr>(coset_pre_), n_ + 4, shift_, ru));
        CHK(coset_post_inv_.alloc(f4));
        CHK(powers(st, ptr<Fr>(coset_post_inv_), n4_, shift_inv_, n4_inv_ * ru));
        CHK(scales_.alloc(2 * sizeof(Fr)));
        {
            Fr sc[2] = {n_inv_ * ru, n4_inv_ * ru};
            HIPCHK(hipMemcpy(scales_.p, sc, sizeof sc, hipMemcpyHostToDevice));
        }
        CHK(x4_.alloc(f4));
        CHK(powers(st, ptr<Fr>(x4_), n4_, omega4_, shift_));
        // MSM tables
        DevBuf srs;
        CHK(srs.alloc((size_t)(n_ + 3) * sizeof(Aff)));
        HIPCHK(hipMemcpy(srs.p, d->srs_g1, (size_t)(n_ + 3) * sizeof(Aff), hipMemcpyHostToDevice));
        CHK((build_tables<FRP, FPP>(st, msm_ctx_, ptr<Aff>(srs), n_ + 3, tab_can_)));
        wires_lag_mode_ = env_int("APK_WIRES_LAGRANGE", -1, -1, 1);
        {
            const Aff* g = reinterpret_cast<const Aff*>(d->srs_g1);
            for (int k = 0; k < 3; k++) {
                Pt p = Pt::from_affine(g[n_ + k]);
                p.madd(g[k], /*negate=*/true);
                lag_dk_[k] = p.to_affine();
            }
        }
        if (d->srs_g1_lagrange || wires_lag_mode_ == 1) {
            // the extended Lagrange table NOW: the caller's Lagrange SRS (gnark's ProvingKey.KzgLagrange; BSB22 needs it) or a forced
            // Lagrange route - derived from the canonical SRS when not given (kzg.ToLagrangeG1 as an inverse FFT in the exponent)
            CHK(build_lagrange_table(st, ptr<Aff>(srs), d->srs_g1_lagrange));
        } else if (wires_lag_mode_ != 0) {
            // automatic route, nothing given: derived on first use (ensure_lagrange_table), from the SRS kept here
            CHK(srs_keep_.alloc((size_t)(n_ + 3) * sizeof(Aff)));
            HIPCHK(hipMemcpyAsync(srs_keep_.p, srs.p, (size_t)(n_ + 3) * sizeof(Aff), hipMemcpyDeviceToDevice, st));
        }
        HIPCHK(hipDeviceSynchronize());
        srs.release();
        CHK(set_sort_lds_limits<FRP>(msm_ctx_));
        // proving slots
        int nslots = d->slots > 0 ? d->slots : 1;
        // 16 concurrently active streams are the optimum at 2^17 (round 6, sleeping waits: 12 -> 542, 16 -> 549, 20 -> 544, 24 -> 518
        // proofs/s; the collapse rounds 2-5 measured beyond 16 - 24: -25 %, 32: -40 % - was mostly the cgroup freezing a process
        // with more spinning proving threads than its 16-CPU quota); callers beyond the cap wait for a slot, which also hides
        // their host-side gaps - or, on small circuits, join a gang
        static const int max_slots = env_int("APK_MAX_SLOTS", 16, 1, 64);
        // Gangs: a context asked for more slots than it may run streams lets up to gang_cap_ proofs share a stream (gang.h).
        // APK_GANG: 1 = never, 2..4 = members per stream; default by size (choose_gang).  The operands of a merged launch must fit
        // the scan's 2^21 buckets and the sort's totals buffers.
        gang_cap_ = choose_gang((int)log_n_, nslots, max_slots);
        while (gang_cap_ > 1 && ((uint64_t)MSM_MAX_BATCH * gang_cap_ * msm_ctx_.NB > (1ull << 21) || MSM_MAX_BATCH * gang_cap_ > MSM_ARGS_MAX ||
                                 (msm_ctx_.part.P && (uint64_t)MSM_MAX_BATCH * gang_cap_ * msm_ctx_.part.P > (uint64_t)MSM_MAX_BATCH * MSM_PART_MAX)))
            gang_cap_--;
        ws_batch_ = (uint32_t)(MSM_MAX_BATCH * gang_cap_);
        const int max_streams = nslots > max_slots ? max_slots : nslots;
        if (nslots > max_slots * gang_cap_) nslots = max_slots * gang_cap_;
        many_slots_ = nslots > 2;
        CHK(take_stream_pool(max_streams));
        for (int i = 0; i < nslots; i++) {
            Slot* s = new Slot();
            s->index = slots_.size();
            slots_.push_back(s);
            CHK(alloc_slot(*s));
        }
        static const int gang_wait_us = env_int("APK_GANG_WAIT_US", 300, 0, 100000);
        gate_.configure(slots_.size(), (size_t)max_streams, gang_cap_, gang_wait_us);
        gang_launcher_ = [this](GangReq* const* reqs, int count) { gang_launch(reqs, count); };
        // the trace setup runs on slot 0 (nobody else can take a slot of this context yet), on a stream taken from the device like
        // any other holder's: another context may be proving on the others
        Slot* s0 = acquire();
        const int trc = setup_trace(d);
        release(s0, trc == APK_OK);
        return trc;
    }

    static Fr root_of_unity() {
        // primitive 2^ADICITY-th root of unity (generated constant, tools/gen_params.py)
        Fr a;
        for (int i = 0; i < Fr::N; i++) a.l[i] = FRP::root(i);
        return Fr::to_mont(a);
    }

    // ---- trace polynomials, permutation polynomials, their coset evaluations and the VK commitments ----------
    int setup_trace(const apk_circuit_desc* d);

    int get_vk(apk_vk* out) override {
        if (msm_only_) { set_error("MSM-only context has no verifying key"); return APK_ERR_STATE; }
        memset(out, 0, sizeof *out);
        uint8_t* dst[8 + APK_MAX_COMMITMENTS] = {out->ql, out->qr, out->qm, out->qo, out->qk, out->s[0], out->s[1], out->s[2], out->qcp[0], out->qcp[1]};
        for (uint32_t i = 0; i < 8 + nb_commit_; i++) memcpy(dst[i], &vk_pts_[i], sizeof(Aff));
        memcpy(out->size_inv, &n_inv_, sizeof(Fr));
        memcpy(out->generator, &omega_, sizeof(Fr));
        memcpy(out->coset_shift, &shift_, sizeof(Fr));
        return APK_OK;
    }

    // ---------------------------------------------------------------------------------------------- primitives
    // the one vector of a primitive, on the device: a host vector goes through the slot's upload staging, on its stream
    int upload_in(Slot& s, const void* v, uint64_t len, bool on_device, const Fr** d) {
        if (!on_device) HIPCHK(hipMemcpyAsync(s.scratch_in.p, v, len * sizeof(Fr), hipMemcpyHostToDevice, s.stream));
        *d = on_device ? reinterpret_cast<const Fr*>(v) : ptr<Fr>(s.scratch_in);
        return APK_OK;
    }
    // out[i] = [polys[i]] over T, affine, for i < count: as many MSMs per launch sequence as the workspace takes (an MSM-only context: one), each waited for
    int commit_chunks(Slot& s, const MsmTables& T, const Fr* const* polys, const uint32_t* lens, uint32_t count, void* out) {
        const uint32_t per = ws_batch_ < (uint32_t)MSM_MAX_BATCH ? ws_batch_ : (uint32_t)MSM_MAX_BATCH;
        for (uint32_t i0 = 0; i0 < count; i0 += per) {
            MsmBatchArgs m{};
            m.batch = count - i0 < per ? count - i0 : per;
            for (uint32_t b = 0; b < m.batch; b++) { m.scalars[b] = polys[i0 + b]; m.len[b] = lens[i0 + b]; m.offset[b] = 0; }
            CHK(run_msm(s, T, m));
            CHK(sync_results(s));
            memcpy(reinterpret_cast<uint8_t*>(out) + i0 * sizeof(Aff), pin_host<Aff>(s.h_pinned, PIN_AFF), m.batch * sizeof(Aff));
        }
        return APK_OK;
    }
    int commit_one(Slot& s, const MsmTables& T, const Fr* poly, uint32_t len, void* out) { return commit_chunks(s, T, &poly, &len, 1, out); }
    int msm(int basis, const void* scalars, uint64_t len, bool on_device, void* out) override {
        HIPCHK(hipSetDevice(device_));
        SlotGuard g(this);
        Slot& s = *g.s;
        if (basis) (void)ensure_lagrange_table(s.stream);      // the automatic mode derives the table on first use
        MsmTables& T = basis ? tab_lag_ : tab_can_;
        if (basis ? !lagrange_ready() : !T.built) { set_error("context has no %s SRS", basis ? "Lagrange" : "canonical"); return APK_ERR_STATE; }
        if (len > T.n_bases) { set_error("msm length %llu exceeds SRS size %u", (unsigned long long)len, T.n_bases); return APK_ERR_ARG; }
        const Fr* dsc = nullptr;
        CHK(upload_in(s, scalars, len, on_device, &dsc));
        CHK(commit_one(s, T, dsc, (uint32_t)len, out));
        g.ok = true;
        return APK_OK;
    }

    // `count` partial MSMs in one batch: sum over scalars[b][0 .. len) * SRS[offset + i]; scalars in device memory
    int msm_batch(int basis, uint32_t count, const void* const* d_scalars, const uint64_t* offsets, const uint64_t* lens, void* out) override {
        HIPCHK(hipSetDevice(device_));
        if (count == 0 || count > MSM_MAX_BATCH) { set_error("msm batch of %u (1..%d)", count, MSM_MAX_BATCH); return APK_ERR_ARG; }
        MaybeGuard g(this);                            // called from inside this thread's commit hook: the prover's slot
        Slot& s = *g.s;
        if (basis) (void)ensure_lagrange_table(s.stream);
        MsmTables& T = basis ? tab_lag_ : tab_can_;
        if (basis ? !lagrange_ready() : !T.built) { set_error("context has no %s SRS", basis ? "Lagrange" : "canonical"); return APK_ERR_STATE; }
        MsmBatchArgs a{};
        a.batch = count;
        a.plain = T.plain ? 1u : 0u;
        for (uint32_t b = 0; b < count; b++) {
            if (d_scalars[b] && !is_device_ptr(d_scalars[b])) { set_error("msm batch: scalars[%u] is not device memory", b); return APK_ERR_ARG; }
            if (lens[b] > T.n_bases || offsets[b] > T.n_bases - lens[b] || !d_scalars[b]) {   /* no uint64 wrap-around */ set_error("msm batch: range [%llu, +%llu) outside the %u bases", (unsigned long long)offsets[b], (unsigned long long)lens[b], T.n_bases); return APK_ERR_ARG; }
            a.scalars[b] = d_scalars[b]; a.len[b] = (uint32_t)lens[b]; a.offset[b] = (uint32_t)offsets[b];
        }
        CHK(run_msm(s, T, a));
        CHK(wait_stream(s));
        const Pt* gsum = pin_host<Pt>(s.h_pinned, PIN_XYZZ);
        Aff r[MSM_MAX_BATCH];
        host_xyzz_batch_to_affine<FPP>(gsum, count, r);
        memcpy(out, r, count * sizeof(Aff));
        s.pending_pts = 0;
        g.ok = true;
        return APK_OK;
    }
    // ---- KZG openings (include/apk.h apk_kzg_*, apk_kzg_*_lagrange) ------------------------------------------------------------------
    // Two forms (kzg_run.h: their launches) on one skeleton, kzg_open_as / kzg_batch_open_as.  Here a form adds what needs the context: the checks, its commitments' table, ready() - table, scratch, point.
    struct KzgCoef : KzgCoefForm<FRP> {      // coefficient form over the canonical SRS
        static const MsmTables& table(const CurveBackend& b) { return b.tab_can_; }
        static int check(const CurveBackend& b, uint32_t count, const void* const* polys, const uint64_t* lens, bool on_device) {
            if (!b.tab_can_.built) { set_error("context has no canonical SRS"); return APK_ERR_STATE; }
            for (uint32_t i = 0; i < count; i++) {
                if (!polys[i]) { set_error("kzg: polynomial %u is null", i); return APK_ERR_ARG; }
                if (lens[i] == 0 || lens[i] > b.tab_can_.n_bases) { set_error("kzg: polynomial %u has %llu coefficients (1..%u)", i, (unsigned long long)lens[i], b.tab_can_.n_bases); return APK_ERR_ARG; }
                if (on_device && !is_device_ptr(polys[i])) { set_error("kzg: polynomial %u is not device memory", i); return APK_ERR_ARG; }
            }
            return APK_OK;
        }
        int ready(CurveBackend& b, Slot& s, const void* point) { memcpy(&this->z, point, sizeof this->z); return s.kzg.ensure(b.tab_can_.n_bases); }
    };
    struct KzgLag : KzgLagForm<FRP> {        // evaluation form over the Lagrange SRS
        static const MsmTables& table(const CurveBackend& b) { return b.tab_lag_; }
        static int check(const CurveBackend& b, uint32_t count, const void* const* evals, const uint64_t* lens, bool on_device) {
            if (b.msm_only_) { set_error("MSM-only context has no NTT domain"); return APK_ERR_STATE; }
            for (uint32_t i = 0; i < count; i++) {
                if (lens[i] != b.n_) { set_error("kzg: %llu values, the domain has %u", (unsigned long long)lens[i], b.n_); return APK_ERR_ARG; }
                if (!evals[i]) { set_error("kzg: vector %u is null", i); return APK_ERR_ARG; }
                if (on_device && !is_device_ptr(evals[i])) { set_error("kzg: vector %u is not device memory", i); return APK_ERR_ARG; }
            }
            return APK_OK;
        }
        static int ready_table(CurveBackend& b, Slot& s) {           // (the automatic mode derives the Lagrange table now)
            (void)b.ensure_lagrange_table(s.stream);
            if (!b.lagrange_ready()) { set_error("context has no Lagrange SRS"); return APK_ERR_STATE; }
            if (!s.kzg.fits(b.tab_can_.n_bases, b.n_)) { set_error("kzg: the slot's scratch does not hold an opening in evaluation form"); return APK_ERR_STATE; }
            return APK_OK;
        }
        int ready(CurveBackend& b, Slot& s, const void* point) {
            CHK(ready_table(b, s));
            this->pt = kzg_lag_point<FRP>(point, b.log_n_, b.n_inv_); this->tw = ptr<Fr>(b.tw_n_); this->n = b.n_;
            return s.kzg.ensure(b.tab_can_.n_bases);
        }
    };
    static Fr* kzg_h_values(const Slot& s) { return pin_host<Fr>(s.h_pinned, PIN_FR); }   // where an opening's values reach the host
    static Fr* kzg_d_values(const Slot& s) { return pin_dev<Fr>(s.d_pinned, PIN_FR); }   // the device's view of it, if any
    // The fold divided and its quotient committed to out_h; returns with everything waited for.  out_value may be null.
    template <class Form>
    int kzg_divide_commit(Form& f, Slot& s, const KzgPolys<FRP>& a, const Fr* vals, void* out_h, void* out_value) {
        CHK(f.divide(s.stream, s.kzg, a, vals, kzg_h_values(s)));
        if (const uint32_t len = f.quot_len(a)) CHK(commit_one(s, f.table(*this), s.kzg.quot(), len, out_h));
        else {             // (coefficient form) a constant: the quotient is the zero polynomial
            CHK(wait_stream(s));
            const Aff inf = Aff::inf(); memcpy(out_h, &inf, sizeof inf);
        }
        if (out_value) memcpy(out_value, kzg_h_values(s), sizeof(Fr));
        return APK_OK;
    }
    template <class Form>
    int kzg_open_as(Form f, const void* vec, uint64_t len, bool on_device, const void* point, void* out_h, void* out_value) {
        HIPCHK(hipSetDevice(device_));
        CHK(f.check(*this, 1, &vec, &len, on_device));
        SlotGuard g(this);
        Slot& s = *g.s;
        CHK(f.ready(*this, s, point));
        KzgPolys<FRP> a{};
        a.count = 1; a.max_len = (uint32_t)len; a.len[0] = (uint32_t)len;
        CHK(upload_in(s, vec, len, on_device, &a.f[0]));
        if (f.VALUES_FIRST) CHK(f.evaluate(s.stream, s.kzg, a, kzg_d_values(s), kzg_h_values(s)));
        CHK(kzg_divide_commit(f, s, a, nullptr, out_h, out_value));
        g.ok = true;
        return APK_OK;
    }
    template <class Form>
    int kzg_batch_open_as(Form f, uint32_t count, const void* const* vecs, const uint64_t* lens, bool on_device, const void* digests,
                          const void* point, const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) {
        HIPCHK(hipSetDevice(device_));
        if (count == 0 || count > (uint32_t)KZG_MAX_POLYS) { set_error("kzg: %u %s (1..%d)", count, f.NOUN, KZG_MAX_POLYS); return APK_ERR_ARG; }
        CHK(f.check(*this, count, vecs, lens, on_device));
        std::vector<DevBuf> staged(on_device ? 0 : count);
        KzgPolys<FRP> a{};
        CHK(kzg_stage<FRP>(count, vecs, lens, on_device, staged, a));
        SlotGuard g(this);
        Slot& s = *g.s;
        CHK(f.ready(*this, s, point));
        // the values first: the commitments (when the caller has none) queue behind them
        CHK(f.evaluate(s.stream, s.kzg, a, kzg_d_values(s), kzg_h_values(s)));
        std::vector<Aff> digs(count);
        if (digests) memcpy(digs.data(), digests, count * sizeof(Aff));
        else CHK(commit_chunks(s, f.table(*this), a.f, a.len, count, digs.data()));
        CHK(wait_stream(s));      // the one synchronisation between the values and the fold (already over when the digests were committed)
        const std::vector<Fr> vals(kzg_h_values(s), kzg_h_values(s) + count);
        Fr gamma;
        CHK(apk_kzg_fold_challenge(CURVE_ID, count, digs.data(), vals.data(), &f.point(), extra, extra_len, &gamma));
        a.coef[0] = Fr::one(); for (uint32_t i = 1; i < count; i++) a.coef[i] = a.coef[i - 1] * gamma;     // the fold's weights
        CHK(kzg_divide_commit(f, s, a, vals.data(), out_h, nullptr));
        memcpy(out_values, vals.data(), count * sizeof(Fr));
        if (out_gamma) memcpy(out_gamma, &gamma, sizeof gamma);
        g.ok = true;
        return APK_OK;
    }
    int kzg_open(const void* poly, uint64_t len, bool on_device, const void* point, void* out_h, void* out_value) override {
        return kzg_open_as(KzgCoef{}, poly, len, on_device, point, out_h, out_value);
    }
    int kzg_batch_open(uint32_t count, const void* const* polys, const uint64_t* lens, bool on_device, const void* digests,
                       const void* point, const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) override {
        return kzg_batch_open_as(KzgCoef{}, count, polys, lens, on_device, digests, point, extra, extra_len, out_h, out_values, out_gamma);
    }
    int kzg_open_lagrange(const void* evals, uint64_t len, bool on_device, const void* point, void* out_h, void* out_value) override {
        return kzg_open_as(KzgLag{}, evals, len, on_device, point, out_h, out_value);
    }
    int kzg_batch_open_lagrange(uint32_t count, const void* const* evals, bool on_device, const void* digests, const void* point,
                                const uint8_t* extra, size_t extra_len, void* out_h, void* out_values, void* out_gamma) override {
        const std::vector<uint64_t> lens(KZG_MAX_POLYS, n_);
        return kzg_batch_open_as(KzgLag{}, count, evals, lens.data(), on_device, digests, point, extra, extra_len, out_h, out_values, out_gamma);
    }
    // `count` openings, each a polynomial at its own point (kzg_run.h kzg_group_divide), in call order and in groups as wide as
    // commit_chunks': per group three launches, ONE MSM batch over the quotients of its rows and one synchronisation.
    int kzg_open_multi(uint32_t count, const void* const* polys, const uint64_t* lens, bool on_device, const void* points, void* out_h,
                       void* out_values) override {
        HIPCHK(hipSetDevice(device_));
        if (count == 0 || count > (uint32_t)KZG_MAX_POLYS) { set_error("kzg: %u openings (1..%d)", count, KZG_MAX_POLYS); return APK_ERR_ARG; }
        CHK(KzgCoef::check(*this, count, polys, lens, on_device));
        std::vector<DevBuf> staged(on_device ? 0 : count);
        const Fr* d_poly[KZG_MAX_POLYS];
        CHK(kzg_stage_pairs<FRP>(count, polys, lens, on_device, staged, d_poly));
        SlotGuard g(this);
        Slot& s = *g.s;
        static_assert(KZG_GROUP == MSM_MAX_BATCH, "a group's quotients are one MSM batch");
        const uint32_t per = ws_batch_ < (uint32_t)KZG_GROUP ? ws_batch_ : (uint32_t)KZG_GROUP;
        CHK(s.kzg.ensure_multi(tab_can_.n_bases, per));
        const Fr* z = reinterpret_cast<const Fr*>(points);
        const Aff inf = Aff::inf();
        for (uint32_t i0 = 0; i0 < count; i0 += per) {
            const uint32_t rows = count - i0 < per ? count - i0 : per;
            KzgGroup<FRP> grp{};
            for (uint32_t r = 0; r < rows; r++) { grp.f[r] = d_poly[i0 + r]; grp.len[r] = (uint32_t)lens[i0 + r]; memcpy(&grp.z[r], &z[i0 + r], sizeof(Fr)); }
            CHK(kzg_group_divide<FRP>(s.stream, s.kzg, grp, rows, kzg_h_values(s)));
            // the rows with a quotient are the operands of the batch (a constant's H is the point at infinity)
            MsmBatchArgs m{};
            uint32_t row_of[KZG_GROUP];
            for (uint32_t r = 0; r < rows; r++) {
                if (grp.len[r] < 2) continue;
                m.scalars[m.batch] = grp.q[r]; m.len[m.batch] = grp.len[r] - 1; m.offset[m.batch] = 0;
                row_of[m.batch++] = r;
            }
            if (m.batch) { CHK(run_msm(s, tab_can_, m)); CHK(sync_results(s)); }
            else CHK(wait_stream(s));
            uint8_t* h = reinterpret_cast<uint8_t*>(out_h) + (size_t)i0 * sizeof(Aff);
            for (uint32_t r = 0; r < rows; r++) memcpy(h + r * sizeof(Aff), &inf, sizeof inf);
            for (uint32_t b = 0; b < m.batch; b++) memcpy(h + row_of[b] * sizeof(Aff), pin_host<Aff>(s.h_pinned, PIN_AFF) + b, sizeof(Aff));
            memcpy(reinterpret_cast<uint8_t*>(out_values) + (size_t)i0 * sizeof(Fr), kzg_h_values(s), rows * sizeof(Fr));
        }
        g.ok = true;
        return APK_OK;
    }
    // The same in evaluation form (kzg_run.h kzg_lag_group_open): `count` vectors of n values, each at its own point, in call order
    // and in groups as wide as commit_chunks': per group at most six launches, ONE MSM batch over the Lagrange SRS whose operand r
    // is row r's n quotient values (a zero or constant vector reaches the point at infinity through the MSM, as in the single
    // form) and one synchronisation.
    int kzg_open_multi_lagrange(uint32_t count, const void* const* evals, bool on_device, const void* points, void* out_h,
                                void* out_values) override {
        HIPCHK(hipSetDevice(device_));
        if (count == 0 || count > (uint32_t)KZG_MAX_POLYS) { set_error("kzg: %u openings (1..%d)", count, KZG_MAX_POLYS); return APK_ERR_ARG; }
        const std::vector<uint64_t> lens(KZG_MAX_POLYS, n_);
        CHK(KzgLag::check(*this, count, evals, lens.data(), on_device));
        std::vector<DevBuf> staged(on_device ? 0 : count);
        const Fr* d_vec[KZG_MAX_POLYS];
        CHK(kzg_stage_pairs<FRP>(count, evals, lens.data(), on_device, staged, d_vec));
        SlotGuard g(this);
        Slot& s = *g.s;
        CHK(KzgLag::ready_table(*this, s));
        const uint32_t per = ws_batch_ < (uint32_t)KZG_GROUP ? ws_batch_ : (uint32_t)KZG_GROUP;
        CHK(s.kzg.ensure_multi(tab_can_.n_bases, per));
        const uint8_t* z = reinterpret_cast<const uint8_t*>(points);
        for (uint32_t i0 = 0; i0 < count; i0 += per) {
            const uint32_t rows = count - i0 < per ? count - i0 : per;
            KzgLagGroup<FRP> grp{};
            for (uint32_t r = 0; r < rows; r++) {
                const KzgLagPoint<FRP> pt = kzg_lag_point<FRP>(z + (size_t)(i0 + r) * sizeof(Fr), log_n_, n_inv_);
                grp.f[r] = d_vec[i0 + r]; grp.z[r] = pt.z; grp.scale[r] = pt.scale; grp.whole[r] = pt.whole; grp.on_domain[r] = pt.on_domain;
            }
            CHK(kzg_lag_group_open<FRP>(s.stream, s.kzg, grp, rows, n_, ptr<Fr>(tw_n_), kzg_h_values(s)));
            MsmBatchArgs m{};
            m.batch = rows;
            for (uint32_t r = 0; r < rows; r++) { m.scalars[r] = grp.q[r]; m.len[r] = n_; m.offset[r] = 0; }
            CHK(run_msm(s, tab_lag_, m));
            CHK(sync_results(s));
            memcpy(reinterpret_cast<uint8_t*>(out_h) + (size_t)i0 * sizeof(Aff), pin_host<Aff>(s.h_pinned, PIN_AFF), rows * sizeof(Aff));
            memcpy(reinterpret_cast<uint8_t*>(out_values) + (size_t)i0 * sizeof(Fr), kzg_h_values(s), rows * sizeof(Fr));
        }
        g.ok = true;
        return APK_OK;
    }
    // ---- the FK20 openings: at every point of the domain (include/apk.h apk_kzg_all_prepare, apk_kzg_open_all; kzg_all_run.h) and on
    // every coset of it (apk_kzg_cosets_prepare, apk_kzg_open_cosets; kzg_cosets_run.h) --------------------------------------------------
    // ONE computation - the whole domain is the coset size l = 1 - whose integer rules are kzg_fk20_plan.h's.  What the two pairs of
    // calls share stands once (kzg_fk20_build, kzg_fk20_unbuild, kzg_fk20_open); each call supplies what is its own.
    int kzg_refused(const Fk20Verdict& v) { if (v.rc != APK_OK) set_error("%s", v.message); return v.rc; }
    // Once per context, under all_mu_: T^ = DFT_2n of the reversed SRS, the twiddles of the chosen stage form (APK_KZG_ALL_GLV), the
    // powers of w_2n and 1 / (2n) for the NTTs that make A^.
    int kzg_all_prepare(const void* srs, uint64_t count) override {
        if (msm_only_) { set_error("MSM-only context has no NTT domain"); return APK_ERR_STATE; }
        CHK(kzg_refused(fk20_check_srs(n_, 1, count)));
        HIPCHK(hipSetDevice(device_));
        std::lock_guard<std::mutex> lk(all_mu_);
        if (all_ready_.load(std::memory_order_acquire)) return APK_OK;
        KzgAllTables<FRP, FPP>& T = all_tab_;
        const Fr sc = Fr::inv(fr_u64(2 * n_)) * fr_u64(32);      // 1 / (2n) in the NTT's radix
        const int rc = kzg_fk20_build(reinterpret_cast<const Aff*>(srs), fk20_shape((int)log_n_, 1), T.that, (size_t)2 * n_ * sizeof(Aff), T.pre, T.scale, sc,
                                      T.tw_inv, nullptr, [&](Slot& s, const Aff* d_t, const Fr* tw_fwd) {
                                          return kzg_all_build_that<FRP, FPP>(s.stream, T, d_t, n_, (int)log_n_, s.kzg_all.points(), tw_fwd);
                                      });
        if (rc != APK_OK) return kzg_fk20_unbuild(rc, false);
        all_ready_.store(true, std::memory_order_release);
        return APK_OK;
    }
    // a failed build leaves nothing of its own behind; the twiddle records stay when an earlier prepare made them
    int kzg_fk20_unbuild(int rc, bool cosets) {
        if (cosets) cos_tab_.release();
        else { all_tab_.that.release(); all_tab_.tw_inv.release(); all_tab_.pre.release(); all_tab_.scale.release(); }
        if (!tw_ready_) all_tab_.glv.release();
        return rc;
    }
    // The stage form (APK_KZG_ALL_GLV) and, for the split form, the twiddle records of the size-2n domain: what the stages in the
    // exponent of BOTH calls read (kzg_all_stages), built by whichever prepare runs first, under all_mu_.  The copy is queued on the
    // slot's stream from `split`, which the caller keeps until it has waited; it sets tw_ready_ then.
    int kzg_twiddles_build(Slot& s, std::vector<KzgAllTwiddle>& split) {
        if (tw_ready_) return APK_OK;
        const int want_glv = env_int("APK_KZG_ALL_GLV", 1, 0, 1);      // read per context, here: tools/kzg_probe.py holds one of each side by side
        KzgAllTables<FRP, FPP>& T = all_tab_;
        T.use_glv = want_glv && GlvParams<FPP>::available && kzg_all_split_table<FRP, FPP>(n_, Fr::sqr(omega4_), split);
        {
            Fp b;
            for (int i = 0; i < Fp::N; i++) b.l[i] = GlvParams<FPP>::beta[i];
            T.beta = Fp::to_mont(b);
        }
        if (T.use_glv) {
            CHK(T.glv.alloc((size_t)n_ * sizeof(KzgAllTwiddle)));
            HIPCHK(hipMemcpyAsync(T.glv.p, split.data(), (size_t)n_ * sizeof(KzgAllTwiddle), hipMemcpyHostToDevice, s.stream));
        }
        return APK_OK;
    }
    // What both prepare calls do around their table launch, on a slot like any other call and in that slot's KzgAllScratch (2n
    // points): t from the planner's source rule, the scale word `sc`, the `pre` powers (w_2n'^u, u < n', in the NTT's radix), the
    // stage twiddles unless an earlier prepare made them, the plain form's tables (tw_inv: w_2n'^(-j), j < n'; tw_small, where the
    // caller keeps one: (w^l)^j, j < n' / 2; tw_fwd: w_2n^j, j < n, for `launch` alone; all Montgomery), then `launch` - the
    // transform of t into `table` - and the wait.
    // The host data (t, split, sc) and the device temporaries (d_t, tw_fwd) feed copies and launches queued on the slot's stream,
    // and on an error return the SlotGuard drains that stream in its destructor.  They are declared BEFORE the guard and so
    // destroyed after it: the slot is taken in this frame, not in a helper that hands it back, and `launch` runs inside it.
    template <class Launch>
    int kzg_fk20_build(const Aff* srs, const Fk20Shape& sh, DevBuf& table, size_t table_bytes, DevBuf& pre, DevBuf& scale, const Fr sc,
                       DevBuf& tw_inv, DevBuf* tw_small, Launch&& launch) {
        const uint32_t n = sh.n, n2 = 2 * sh.n, np = sh.np;
        const Fr w2n = Fr::sqr(omega4_), ru = fr_u64(32);     // (ru: x R -> x R', the radix of every NTT table)
        const Fr w2np = Fr::pow_u64(w2n, (uint64_t)sh.l);
        std::vector<KzgAllTwiddle> split;
        std::vector<Aff> t(n2, Aff::inf());
        for (uint32_t i = 0; i < n2; i++)
            if (const int64_t j = fk20_t_source(sh, i); j != FK20_T_INFINITY) t[i] = srs[j];
        DevBuf d_t, tw_fwd;
        CHK(d_t.alloc((size_t)n2 * sizeof(Aff)));
        CHK(table.alloc(table_bytes));
        CHK(pre.alloc((size_t)np * sizeof(Fr)));
        CHK(scale.alloc(sizeof(Fr)));
        SlotGuard g(this);
        Slot& s = *g.s;
        CHK(s.kzg_all.ensure(n));
        HIPCHK(hipMemcpyAsync(d_t.p, t.data(), (size_t)n2 * sizeof(Aff), hipMemcpyHostToDevice, s.stream));
        HIPCHK(hipMemcpyAsync(scale.p, &sc, sizeof sc, hipMemcpyHostToDevice, s.stream));
        CHK(powers(s.stream, ptr<Fr>(pre), np, w2np, ru));
        CHK(kzg_twiddles_build(s, split));
        if (!all_tab_.use_glv) {
            CHK(tw_inv.alloc((size_t)np * sizeof(Fr)));
            if (tw_small) CHK(tw_small->alloc((size_t)(np / 2) * sizeof(Fr)));
            CHK(tw_fwd.alloc((size_t)n * sizeof(Fr)));
            CHK(powers(s.stream, ptr<Fr>(tw_inv), np, Fr::inv(w2np), Fr::one()));
            if (tw_small) CHK(powers(s.stream, ptr<Fr>(*tw_small), np / 2, Fr::sqr(w2np), Fr::one()));
            CHK(powers(s.stream, ptr<Fr>(tw_fwd), n, w2n, Fr::one()));
        }
        CHK(launch(s, ptr<Aff>(d_t), ptr<Fr>(tw_fwd)));
        CHK(wait_stream(s));      // (t, split, sc and the temporaries are released on return)
        g.ok = true;
        tw_ready_ = true;
        return APK_OK;
    }
    // What a slot's scratch offers an open call: where the size-n NTT of f goes, the values the call returns, the affine results
    struct KzgFk20Areas { Fr* ntt; const Fr* values; const Aff* result; };
    // The frame of both open calls.  l: the coset size the context is prepared for, 0 = `prepare` has not run.  The checks in the
    // order of include/apk.h, a slot, its scratch (`scratch` allocates it and names its areas), the upload, the size-n NTT of f,
    // `middle` - which queues what leads from f to the n' results, and when f has no quotient (fk20_has_quotient: every H is
    // infinity) nothing but what the values need - one copy of each result and one wait.
    template <class Scratch, class Middle>
    int kzg_fk20_open(uint32_t l, const char* prepare, const void* poly, uint64_t len, bool on_device, void* out_h, void* out_values,
                      Scratch&& scratch, Middle&& middle) {
        if (msm_only_) { set_error("MSM-only context has no NTT domain"); return APK_ERR_STATE; }
        if (!l) { set_error("kzg: %s has not run on this context", prepare); return APK_ERR_STATE; }
        const Fk20Shape sh = fk20_shape((int)log_n_, l);
        CHK(kzg_refused(fk20_check_len(sh.n, sh.l, len)));
        HIPCHK(hipSetDevice(device_));
        if (on_device && !is_device_ptr(poly)) { set_error("kzg: the polynomial is not device memory"); return APK_ERR_ARG; }
        SlotGuard g(this);
        Slot& s = *g.s;
        KzgFk20Areas a{};
        CHK(scratch(s, sh, a));
        const Fr* f = nullptr;
        CHK(upload_in(s, poly, len, on_device, &f));
        CHK(run_ntt(s.stream, 0, false, f, a.ntt, (uint32_t)len, n_, nullptr, nullptr, nullptr));
        const bool quotient = fk20_has_quotient(sh, len);
        CHK(middle(s, sh, f, quotient));
        if (quotient) HIPCHK(hipMemcpyAsync(out_h, a.result, (size_t)sh.np * sizeof(Aff), hipMemcpyDeviceToHost, s.stream));
        else memset(out_h, 0, (size_t)sh.np * sizeof(Aff));
        if (out_values) HIPCHK(hipMemcpyAsync(out_values, a.values, (size_t)n_ * sizeof(Fr), hipMemcpyDeviceToHost, s.stream));
        CHK(wait_stream(s));
        g.ok = true;
        return APK_OK;
    }
    // out_h[i], out_values[i] = the opening at w^i, i < n: three size-n NTTs (the values; the even and the odd half of A^, scaled by
    // 1 / (2n)), then kzg_all_open's launches.
    int kzg_open_all(const void* poly, uint64_t len, bool on_device, void* out_h, void* out_values) override {
        return kzg_fk20_open(
            all_ready_.load(std::memory_order_acquire) ? 1u : 0u, "apk_kzg_all_prepare", poly, len, on_device, out_h, out_values,
            [&](Slot& s, const Fk20Shape& sh, KzgFk20Areas& a) {
                CHK(s.kzg_all.ensure(sh.n));
                a = {s.kzg_all.values(), s.kzg_all.values(), s.kzg_all.result()};
                return APK_OK;
            },
            [&](Slot& s, const Fk20Shape&, const Fr* f, bool quotient) {
                if (!quotient) return APK_OK;
                const KzgAllScratch<FRP, FPP>& ks = s.kzg_all;
                // a_m = f_(m+1): A^_(2i) = NTT_n(a)_i, A^_(2i+1) = NTT_n(a_m w_2n^m)_i
                CHK(run_ntt(s.stream, 0, false, f + 1, ks.a_even(), (uint32_t)len - 1, n_, nullptr, nullptr, ptr<Fr>(all_tab_.scale)));
                CHK(run_ntt(s.stream, 0, false, f + 1, ks.a_odd(), (uint32_t)len - 1, n_, ptr<Fr>(all_tab_.pre), nullptr, ptr<Fr>(all_tab_.scale)));
                return kzg_all_open<FRP, FPP>(s.stream, all_tab_, ks, n_, (int)log_n_, ptr<Fr>(tw_n_));
            });
    }
    // Once per context, under all_mu_ (one coset size per context): the table of the l transforms T^_c = DFT_2n'(t_c) and their
    // multiples by 2^64, 2^128, 2^192, the powers of w_2n' and 1 / (2n') for the NTTs that make A^, the plain form's tables of the
    // two small transforms - and the stage twiddles, unless apk_kzg_all_prepare has made them.
    int kzg_cosets_prepare(const void* srs, uint64_t count, uint32_t l) override {
        if (msm_only_) { set_error("MSM-only context has no NTT domain"); return APK_ERR_STATE; }
        CHK(kzg_refused(fk20_check_coset_size(n_, l)));
        CHK(kzg_refused(fk20_check_srs(n_, l, count)));
        HIPCHK(hipSetDevice(device_));
        std::lock_guard<std::mutex> lk(all_mu_);
        if (const uint32_t have = cos_l_.load(std::memory_order_acquire)) {
            if (have == l) return APK_OK;
            set_error("kzg: the context is prepared for cosets of %u points (one coset size per context)", have);
            return APK_ERR_STATE;
        }
        KzgCosetsTables& C = cos_tab_;
        const Fk20Shape sh = fk20_shape((int)log_n_, l);
        C.l = sh.l; C.log_l = sh.log_l;
        // 1 / (2n') / R in the NTT's radix: the stored limbs of x R' with x = 1 / (2n' R) are the plain integer 32 / (2n')
        const Fr sc = Fr::from_mont(Fr::inv(fr_u64(2 * sh.np)) * fr_u64(32));
        const int rc = kzg_fk20_build(reinterpret_cast<const Aff*>(srs), sh, C.tab, (size_t)2 * n_ * KZG_COSETS_WINDOWS * sizeof(Aff), C.pre, C.scale, sc,
                                      C.tw_inv, &C.tw_fwd, [&](Slot& s, const Aff* d_t, const Fr* tw_fwd) {
                                          return kzg_cosets_build_table<FRP, FPP>(s.stream, all_tab_, C, d_t, n_, (int)log_n_, s.kzg_all.points(), tw_fwd);
                                      });
        if (rc != APK_OK) return kzg_fk20_unbuild(rc, true);
        cos_l_.store(l, std::memory_order_release);
        return APK_OK;
    }
    // out_h[i] = the proof of coset i < n', out_values[i l + j] = f(w^(i + n' j)): the size-n NTT of the values and their
    // permutation; the gather of the l strided sequences and their 2l size-n' NTTs (the even and the odd half of every A^_c, scaled
    // by 1 / (2n'), in the planner's chunks of up to NTT_ARGS_MAX per launch sequence); kzg_cosets_open's launches.
    int kzg_open_cosets(const void* poly, uint64_t len, bool on_device, void* out_h, void* out_values) override {
        const KzgCosetsTables& C = cos_tab_;
        return kzg_fk20_open(
            cos_l_.load(std::memory_order_acquire), "apk_kzg_cosets_prepare", poly, len, on_device, out_h, out_values,
            [&](Slot& s, const Fk20Shape& sh, KzgFk20Areas& a) {
                CHK(s.kzg_cosets.ensure(sh.n, sh.np));
                a = {s.kzg_cosets.values(), s.kzg_cosets.values_by_coset(), s.kzg_cosets.result()};
                return APK_OK;
            },
            [&](Slot& s, const Fk20Shape& sh, const Fr* f, bool quotient) {
                const KzgCosetsScratch<FRP, FPP>& ks = s.kzg_cosets;
                CHK((kzg_cosets_values<FRP, FPP>(s.stream, C, ks, n_, (int)log_n_)));
                if (!quotient) return APK_OK;
                CHK((kzg_cosets_split<FRP, FPP>(s.stream, C, ks, f, (uint32_t)len, n_, (int)log_n_)));
                // A^_c[2i] = NTT_n'(a_c)_i, A^_c[2i+1] = NTT_n'(a_c[u] w_2n'^u)_i: size-n' transforms on the size-n table
                for (uint32_t i = 0; i < fk20_chunks(sh.l); i++) {
                    const Fk20Chunk ch = fk20_chunk(sh.l, i);
                    const Fr* ins[NTT_ARGS_MAX]; Fr* outs[NTT_ARGS_MAX]; uint32_t lens[NTT_ARGS_MAX];
                    for (int k = 0; k < ch.cnt; k++) {
                        ins[k] = ks.gathered() + (size_t)(ch.c0 + k) * sh.np;
                        outs[k] = (ch.odd ? ks.a_odd() : ks.a_even()) + (size_t)(ch.c0 + k) * sh.np;
                        lens[k] = sh.np;
                    }
                    CHK(run_ntt_batch(s.stream, 0, false, ch.cnt, ins, outs, lens, sh.np, ch.odd ? ptr<Fr>(C.pre) : nullptr, nullptr, ptr<Fr>(C.scale), sh.sub_log()));
                }
                return kzg_cosets_open<FRP, FPP>(s.stream, all_tab_, C, ks, n_, (int)log_n_);
            });
    }
    // ---- `count` polynomials on every coset in ONE call (include/apk.h apk_kzg_open_cosets_multi; kzg_cosets_multi_run.h) --------------
    // out_h[b n' + i], out_values[b n + i l + j] = what kzg_open_cosets(polys[b], lens[b]) returns.  The rules, the groups and every
    // index are the planner's (fk20_multi_check, fk20_multi_group, Fk20Multi).  One slot; the scratch for the call's largest group
    // before anything is queued; then per group the uploads (host form), G size-n NTTs in one launch sequence, the permutation of
    // the values, the split, the 2 G l size-n' NTTs in the planner's chunks, kzg_cosets_multi_open's launches and one copy of each
    // result - the next group's launches follow the copies on the same stream - and ONE wait, at the end.  On an error return the
    // SlotGuard drains the stream before the slot is released, as in kzg_fk20_open.
    int kzg_open_cosets_multi(uint32_t count, const void* const* polys, const uint64_t* lens, bool on_device, void* out_h, void* out_values) override {
        const uint32_t l = cos_l_.load(std::memory_order_acquire);
        CHK(kzg_refused(fk20_multi_check(msm_only_, l, n_, count, polys, lens, out_h)));
        HIPCHK(hipSetDevice(device_));
        if (on_device)
            for (uint32_t b = 0; b < count; b++)
                if (!is_device_ptr(polys[b])) return kzg_refused(fk20_multi_not_device(b));
        const KzgCosetsTables& C = cos_tab_;
        SlotGuard g(this);
        Slot& s = *g.s;
        KzgCosetsMultiScratch<FRP, FPP>& ks = s.kzg_cosets_multi;
        CHK(ks.ensure(fk20_multi((int)log_n_, l, fk20_multi_largest_group(count))));
        for (uint32_t gi = 0; gi < fk20_multi_groups(count); gi++) {
            const Fk20Group grp = fk20_multi_group(count, gi);
            const Fk20Multi m = fk20_multi((int)log_n_, l, grp.size);
            const Fk20Shape& sh = m.s;
            CHK(ks.ensure(m));      // (lays the areas out for this group; it is no larger than the first)
            KzgCosetsMultiSrc<FRP> src{};
            const Fr* ins[NTT_ARGS_MAX]; Fr* outs[NTT_ARGS_MAX]; uint32_t in_lens[NTT_ARGS_MAX];
            for (uint32_t b = 0; b < m.G; b++) {
                const uint64_t len = lens[grp.b0 + b];
                // host form: a (pointer, length) that an earlier row of the group brought is uploaded once, and read from there
                uint32_t first = b;
                if (!on_device)
                    for (uint32_t a = 0; a < b && first == b; a++)
                        if (polys[grp.b0 + a] == polys[grp.b0 + b] && lens[grp.b0 + a] == len) first = a;
                if (!on_device && first == b) HIPCHK(hipMemcpyAsync(ks.upload(b), polys[grp.b0 + b], len * sizeof(Fr), hipMemcpyHostToDevice, s.stream));
                src.f[b] = on_device ? reinterpret_cast<const Fr*>(polys[grp.b0 + b]) : ks.upload(first);
                src.len[b] = (uint32_t)len;
                ins[b] = src.f[b]; outs[b] = ks.values() + m.value(b, 0); in_lens[b] = (uint32_t)len;
            }
            CHK(run_ntt_batch(s.stream, 0, false, (int)m.G, ins, outs, in_lens, n_, nullptr, nullptr, nullptr));
            CHK((kzg_cosets_multi_values<FRP, FPP>(s.stream, m, ks)));
            CHK((kzg_cosets_multi_split<FRP, FPP>(s.stream, m, ks, src)));
            // A^_(b,c)[2i] = NTT_n'(a_(b,c))_i, A^_(b,c)[2i+1] = NTT_n'(a_(b,c)[u] w_2n'^u)_i: the single call's operands, over G l rows
            for (uint32_t i = 0; i < fk20_chunks(m.rows()); i++) {
                const Fk20Chunk ch = fk20_chunk(m.rows(), i);
                for (int k = 0; k < ch.cnt; k++) {
                    ins[k] = ks.gathered() + (size_t)(ch.c0 + k) * sh.np;
                    outs[k] = (ch.odd ? ks.a_odd() : ks.a_even()) + (size_t)(ch.c0 + k) * sh.np;
                    in_lens[k] = sh.np;
                }
                CHK(run_ntt_batch(s.stream, 0, false, ch.cnt, ins, outs, in_lens, sh.np, ch.odd ? ptr<Fr>(C.pre) : nullptr, nullptr, ptr<Fr>(C.scale), sh.sub_log()));
            }
            CHK((kzg_cosets_multi_open<FRP, FPP>(s.stream, all_tab_, C, m, ks)));
            HIPCHK(hipMemcpyAsync(reinterpret_cast<Aff*>(out_h) + m.result(grp.b0, 0), ks.result(), (size_t)m.G * sh.np * sizeof(Aff), hipMemcpyDeviceToHost, s.stream));
            if (out_values)
                HIPCHK(hipMemcpyAsync(reinterpret_cast<Fr*>(out_values) + m.value(grp.b0, 0), ks.values_by_coset(), (size_t)m.G * n_ * sizeof(Fr), hipMemcpyDeviceToHost, s.stream));
        }
        CHK(wait_stream(s));
        g.ok = true;
        return APK_OK;
    }
    // ---- the polynomial back from `count` of its cells (include/apk.h apk_kzg_recover_cosets; kzg_recover_run.h) -------------------
    // The integer rules are kzg_recover_plan.h's.  No prepare call and no SRS table: the one piece of state is the `post` table of
    // the last transform, built here by the first call (waited for under its mutex: another slot's stream may read it next).
    int kzg_recover_table(Slot& s) {
        if (recover_ready_.load(std::memory_order_acquire)) return APK_OK;
        std::lock_guard<std::mutex> lk(recover_mu_);
        if (recover_ready_.load(std::memory_order_acquire)) return APK_OK;
        CHK(recover_post_.alloc((size_t)n_ * sizeof(Fr)));
        int rc = powers(s.stream, ptr<Fr>(recover_post_), n_, shift_inv_, n_inv_ * fr_u64(32));     // g^(-c) / n in the NTT's radix
        if (rc == APK_OK && hipStreamSynchronize(s.stream) != hipSuccess) { set_error("kzg: the recovery table"); rc = APK_ERR_HIP; }
        if (rc != APK_OK) { recover_post_.release(); return rc; }
        recover_ready_.store(true, std::memory_order_release);
        return APK_OK;
    }
    // The checks in the order of include/apk.h, a slot, its scratch, the upload of the rows, steps (1) - (6) of
    // kernels_kzg_recover.h - three size-n transforms between the runner's launches, none reading what it writes - the check of
    // the coefficients in [len, count l), one copy of the len coefficients and one wait.  A host destination gets its copy through
    // `staged` once the verdict is known; a device destination from kzg_recover_emit_kernel, which reads the verdict itself.
    // The plan, `staged` and the flag word feed copies queued on the slot's stream, and on an error return the SlotGuard drains that
    // stream in its destructor: they are declared BEFORE the guard and so destroyed after it (as in kzg_fk20_build).
    int kzg_recover_cosets(uint32_t l, uint32_t count, const uint64_t* indices, const void* values, uint64_t len, bool on_device,
                           void* out_poly) override {
        if (msm_only_) { set_error("MSM-only context has no NTT domain"); return APK_ERR_STATE; }
        const RecoverPlan plan = recover_plan(n_, l, count, indices, len);
        if (plan.verdict.rc != APK_OK) { set_error("%s", plan.verdict.message); return plan.verdict.rc; }
        HIPCHK(hipSetDevice(device_));
        if (on_device && !is_device_ptr(values)) { set_error("kzg: the cells are not device memory"); return APK_ERR_ARG; }
        if (on_device && !is_device_ptr(out_poly)) { set_error("kzg: the destination is not device memory"); return APK_ERR_ARG; }
        std::vector<Fr> staged(on_device ? 0 : (size_t)len);
        uint32_t flag = 0;
        SlotGuard g(this);
        Slot& s = *g.s;
        KzgRecoverScratch<FRP>& ks = s.kzg_recover;
        CHK(ks.ensure(s.stream, n_, plan.np));
        CHK(kzg_recover_table(s));
        const Fr* rows = nullptr;
        CHK(upload_in(s, values, (uint64_t)count * l, on_device, &rows));
        CHK((kzg_recover_scatter<FRP>(s.stream, plan, ks, rows, ptr<Fr>(tw_n_), Fr::pow_u64(shift_, l))));
        CHK(run_ntt(s.stream, 0, true, ks.a(), ks.b(), n_, n_, nullptr, nullptr, ptr<Fr>(scales_)));            // P = f Z
        CHK(run_ntt(s.stream, 0, false, ks.b(), ks.a(), n_, n_, ptr<Fr>(coset_pre_), nullptr, nullptr));         // P on the coset g <w>
        CHK((kzg_recover_divide<FRP>(s.stream, plan, ks)));
        CHK(run_ntt(s.stream, 0, true, ks.a(), ks.b(), n_, n_, nullptr, ptr<Fr>(recover_post_), nullptr));       // f
        CHK((kzg_recover_finish<FRP>(s.stream, plan, ks, on_device ? reinterpret_cast<Fr*>(out_poly) : nullptr, &flag)));
        if (!on_device) HIPCHK(hipMemcpyAsync(staged.data(), ks.b(), (size_t)len * sizeof(Fr), hipMemcpyDeviceToHost, s.stream));
        CHK(wait_stream(s));
        g.ok = true;
        if (flag == ks.epoch) {
            set_error("kzg: the cells are not those of one polynomial of %llu coefficients (a non-zero coefficient in [%llu, %llu))",
                      (unsigned long long)len, (unsigned long long)plan.check_lo, (unsigned long long)plan.check_hi);
            return APK_ERR_VERIFY;
        }
        if (!on_device) memcpy(out_poly, staged.data(), (size_t)len * sizeof(Fr));
        return APK_OK;
    }
    int set_commit_hook(apk_commit_hook fn, void* user) override { hook_ = fn; hook_user_ = user; return APK_OK; }
    int set_wire_hook(apk_wire_hook fn, void* user) override { wire_hook_ = fn; wire_hook_user_ = user; return APK_OK; }
    int set_subcoset(int k, int G, apk_gather_hook fn, void* user) override {
        if (msm_only_) { set_error("MSM-only context has no quotient to split"); return APK_ERR_STATE; }
        HIPCHK(hipSetDevice(device_));
        if (G <= 1 || !fn) { sc_.G = 1; sc_.glog = 0; sc_.hook = nullptr; sc_.user = nullptr; return APK_OK; }
        if ((G != 2 && G != 4 && G != 8) || k < 0 || k >= G) { set_error("sub-coset split: rank %d of %d (2, 4 or 8 ranks)", k, G); return APK_ERR_ARG; }
        if (!qk_direct_) { set_error("sub-coset split needs Qk completed inside the quotient kernel (at most %d written rows)", QK_INJECT_MAX); return APK_ERR_STATE; }
        if ((n4_ >> (G == 2 ? 1 : G == 4 ? 2 : 3)) < 16u) { set_error("sub-coset split: the domain is too small"); return APK_ERR_STATE; }
        for (hipStream_t ps : stream_pool_) HIPCHK(hipStreamSynchronize(ps));
        const int glog = G == 2 ? 1 : G == 4 ? 2 : 3;
        const uint32_t m = n4_ >> glog;
        const Fr ru = fr_u64(32);   // x R -> x R'
        hipStream_t st = nullptr;
        const Fr wk = Fr::pow_u64(omega4_, (uint64_t)k), wk_inv = Fr::pow_u64(omega4_inv_, (uint64_t)k);
        CHK(sc_.pre[0].alloc((size_t)(n_ + 4) * sizeof(Fr)));
        CHK(powers(st, ptr<Fr>(sc_.pre[0]), n_ + 4, shift_ * wk, ru));
        CHK(sc_.pre[1].alloc((size_t)(n_ + 4) * sizeof(Fr)));
        CHK(powers(st, ptr<Fr>(sc_.pre[1]), n_ + 4, shift_ * Fr::pow_u64(omega4_, (uint64_t)((k + 4) % 8)), ru));
        CHK(sc_.post.alloc((size_t)m * sizeof(Fr)));
        CHK(powers(st, ptr<Fr>(sc_.post), m, wk_inv, ru));
        const Fr rho_inv = Fr::pow_u64(omega4_inv_, (uint64_t)m);
        Fr cur = ru;
        for (int e = 0; e < 8; e++) { sc_.rho_inv[e] = cur; cur = cur * rho_inv; }
        for (Slot* s : slots_) CHK(s->sc_gather.alloc((size_t)n4_ * sizeof(Fr)));
        HIPCHK(hipDeviceSynchronize());
        sc_.k = k; sc_.G = G; sc_.glog = glog; sc_.hook = fn; sc_.user = user;
        return APK_OK;
    }
    int device_ordinal() override { return device_; }
    int msm_window() override { return msm_ctx_.c; }
    uint64_t domain_size() override { return msm_only_ ? 0 : n_; }
    // 4n coset evaluations of a canonical polynomial, device memory in and out; COMPLETE when the call returns.  Inside a hook of
    // this context it runs on the prover's own stream (see msm_batch), otherwise on a free slot.
    int coset_ntt_dev(const void* d_in, uint64_t len, void* d_out) override {
        if (msm_only_) { set_error("MSM-only context has no NTT domain"); return APK_ERR_STATE; }
        if (!d_in || !d_out || len == 0 || len > n4_) { set_error("coset ntt: 1..4n coefficients"); return APK_ERR_ARG; }
        HIPCHK(hipSetDevice(device_));
        MaybeGuard g(this);
        CHK(coset_ntt_4n(g.s->stream, reinterpret_cast<const Fr*>(d_in), (uint32_t)len, reinterpret_cast<Fr*>(d_out)));
        HIPCHK(hipStreamSynchronize(g.s->stream));
        g.ok = true;
        return APK_OK;
    }
    // device-to-device copy that has COMPLETED when the call returns (hipMemcpy D2D returns early, and the proving streams are
    // non-blocking streams: they do not order themselves behind the null stream)
    int dev_copy(void* dd, const void* ss, size_t bytes) override {
        HIPCHK(hipSetDevice(device_));
        if (!is_device_ptr(dd)) { set_error("apk_device_copy: destination is not device memory"); return APK_ERR_ARG; }
        if (!is_device_ptr(ss)) { set_error("apk_device_copy: source is not device memory"); return APK_ERR_ARG; }
        Slot* own = MaybeGuard::own(this);             // the prover's stream only when the hook belongs to THIS context
        hipStream_t st = own ? own->stream : nullptr;
        HIPCHK(hipMemcpyAsync(dd, ss, bytes, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        return APK_OK;
    }

    int ntt(int which, int inverse, int coset, void* data) override {
        if (msm_only_) { set_error("MSM-only context has no NTT domain"); return APK_ERR_STATE; }
        HIPCHK(hipSetDevice(device_));
        SlotGuard g(this);
        Slot& s = *g.s;
        const uint32_t N = which ? n4_ : n_;
        if (coset && !which) { set_error("coset transforms are provided on the 4n domain"); return APK_ERR_ARG; }
        Fr* din = ptr<Fr>(s.scratch_in);
        Fr* dout = ptr<Fr>(s.quot);
        HIPCHK(hipMemcpyAsync(din, data, (size_t)N * sizeof(Fr), hipMemcpyHostToDevice, s.stream));
        if (coset == 2 && inverse) { set_error("the semi-canonical form exists for forward coset transforms only"); return APK_ERR_ARG; }
        if (!coset) {
            CHK(run_ntt(s.stream, which, inverse != 0, din, dout, N, N, nullptr, nullptr,
                        inverse ? ptr<Fr>(scales_) + (which ? 1 : 0) : nullptr));
        } else if (!inverse) {
            // forward coset needs shift^i for all i < 4n: build it in hcan for this call
            CHK(powers(s.stream, ptr<Fr>(s.hcan), N, shift_, fr_u64(32)));   // R' form, like every NTT table
            // (coset == 2: the last pass as the prover's own coset evaluations end it - outputs below 2r, NttPassArgs::semi)
            CHK(run_ntt(s.stream, 1, false, din, dout, N, N, ptr<Fr>(s.hcan), nullptr, nullptr, 0, coset == 2));
        } else {
            CHK(run_ntt(s.stream, 1, true, din, dout, N, N, nullptr, ptr<Fr>(coset_post_inv_), nullptr));
        }
        HIPCHK(hipMemcpyAsync(data, dout, (size_t)N * sizeof(Fr), hipMemcpyDeviceToHost, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
        g.ok = true;
        return APK_OK;
    }

    int dev_alloc(size_t bytes, void** p) override { HIPCHK(hipSetDevice(device_)); HIPCHK(hipMalloc(p, bytes)); return APK_OK; }
    int dev_free(void* p) override { HIPCHK(hipSetDevice(device_)); HIPCHK(hipFree(p)); return APK_OK; }
    int dev_upload(void* dd, const void* s, size_t bytes) override { HIPCHK(hipSetDevice(device_)); HIPCHK(hipMemcpy(dd, s, bytes, hipMemcpyHostToDevice)); return APK_OK; }
    int dev_download(void* dd, const void* s, size_t bytes) override { HIPCHK(hipSetDevice(device_)); HIPCHK(hipMemcpy(dd, s, bytes, hipMemcpyDeviceToHost)); return APK_OK; }
    int stats_enable(int en) override { stats_on_ = en != 0; return APK_OK; }
    int stats_read(apk_stats* out, int reset) override {
        std::lock_guard<std::mutex> g(stats_mu_);
        *out = stats_;
        if (reset) stats_ = apk_stats{};
        return APK_OK;
    }

    // ---------------------------------------------------------------------------------------------- helpers
    // q = (f - f(z)) / (X - z) for f of `len` coefficients; pw = z^i, pwi = z^-i tables
    int kzg_quotient(Slot& s, const Fr* f, uint32_t len, const Fr* pw, const Fr* pwi, bool z_is_zero, Fr* q) {
        return poly_kzg_quotient<FRP>(kl(), s.stream, f, len, pw, pwi, z_is_zero, ptr<Fr>(s.tmp), ptr<Fr>(s.scan_tot), q);
    }

    int eval_many(Slot& s, const EvalArgs<FRP>& ea, const Fr* pw, Fr* h_out) {
        hipStream_t st = s.stream;
        // (h_out lies in the slot's pinned buffer: with the zero-copy view the kernel writes the values there itself)
        Fr* const twin = pin_dev_of(s.h_pinned, s.d_pinned, h_out, ea.count * sizeof(Fr));
        const bool direct = twin != nullptr;
        Fr* const ev_out = direct ? twin : ptr<Fr>(s.eval_result);
        CHK(poly_eval_many<FRP>(kl(), st, ea, pw, ptr<Fr>(s.eval_partial), ev_out));
        if (!direct) HIPCHK(hipMemcpyAsync(h_out, s.eval_result.p, ea.count * sizeof(Fr), hipMemcpyDeviceToHost, st));
        return APK_OK;
    }

    typename Proto::KeyPoints key_points() const {
        typename Proto::KeyPoints key{vk_pts_[VK_QL], vk_pts_[VK_QR], vk_pts_[VK_QM], vk_pts_[VK_QO], vk_pts_[VK_QK],
                                      vk_pts_[VK_S1], vk_pts_[VK_S2], vk_pts_[VK_S3], {}, nb_commit_};
        for (uint32_t k = 0; k < nb_commit_; k++) key.qcp[k] = vk_pts_[VK_QCP + k];
        return key;
    }

    static void store_pt(uint8_t* slot, const Aff& p) { memset(slot, 0, APK_G1_MAX_BYTES); memcpy(slot, &p, sizeof(Aff)); }

    // ---------------------------------------------------------------------------------------------- the prover
    // What one apk_prove call carries from round to round.  prove() fills the head, derives the challenges between the rounds
    // (Proto::gamma .. zeta) and takes the phase marks; a round ends where its commitments have reached the host.
    struct ProofRun {
        Slot& s;
        InputSet* in;                      // the host inputs' staging set, or null: the caller's vectors are on the device
        hipStream_t st;
        const Fr *dL, *dR, *dO;            // the wires' values, on the device
        const Fr *pubv, *bl;               // public inputs and blinding scalars, on the host
        const Fr* pi2[APK_MAX_COMMITMENTS];   // the BSB22 columns, on the device (only read)
        apk_proof* out;
        Aff bsb[APK_MAX_COMMITMENTS];
        Fr cval[APK_MAX_COMMITMENTS];      // hash_fr([Bsb_k]): what the prover writes into Qk
        Aff lro[3], zcom, hcom[3];
        Fr gamma, beta, beta_u, beta_u2, alpha, zeta, gk;
        uint8_t gamma_raw[32], beta_raw[32], alpha_raw[32], zeta_raw[32], gk_raw[32];
        typename Proto::KeyPoints key;
        int fill = 0;                      // tail_fill() of this proof
        bool use_lag = false, measuring = false;   // wire_route(): [L][R][O] over the Lagrange SRS; this proof counts its wires' digits
        // R1..R4 of SURVEY.md section 3.3, host wall clock (stats only)
        std::chrono::steady_clock::time_point t_start, t_phase;
        double phase_ms[4] = {0, 0, 0, 0}, lincomb_ms = 0;
    };
    void mark(ProofRun& run, int r) {
        if (!stats_on_) return;
        const auto now = std::chrono::steady_clock::now();
        run.phase_ms[r] = std::chrono::duration<double, std::milli>(now - run.t_phase).count();
        run.t_phase = now;
    }
    // terms of the linearised polynomial: the polynomial (device), its commitment (host), its coefficient (Proto::lin_coefs)
    struct LinTerm { const Fr* poly; uint32_t len; Aff com; Fr coef; };
    enum { LT_QL, LT_QR, LT_QM, LT_QO, LT_QK, LT_S3, LT_Z, LT_H1, LT_H2, LT_H3, LT_BSB, LT_MAX = LT_BSB + APK_MAX_COMMITMENTS };   // positions in a proof's term table
    using HostSum = XYZZ<FPP, Fe64<FPP>>;

    int prove(const void* L, const void* R, const void* O, bool on_device, const void* pub, const void* blinding,
              const void* const* pi2, apk_proof* out) override;
    int round1_wires(ProofRun& run);
    int round2_grand_product(ProofRun& run);
    int round3_quotient(ProofRun& run);
    int round4_openings(ProofRun& run);
    int wire_route(ProofRun& run);
    uint32_t wire_route_finish(ProofRun& run);
    QuotientArgs<FRP> quotient_args(const ProofRun& run);
    int zeta_powers(ProofRun& run);
    Aff lin_commitment(ProofRun& run, const LinTerm* terms, int count, HostPool* pool, const HostSum* lin_h);
};

// =====================================================================================================================
template <class FRP, class FPP, int CURVE_ID>
int CurveBackend<FRP, FPP, CURVE_ID>::setup_trace(const apk_circuit_desc* d) {
    Slot& s = *slots_[0];
    hipStream_t st = s.stream;
    const size_t fn = (size_t)n_ * sizeof(Fr), f4 = (size_t)n4_ * sizeof(Fr);
    // L_0 on the coset: (x^n - 1) / (n (x - 1)).  x^n - 1 = 1/zh_inv[i&3]; computed on the host side as a
    // canonical polynomial (1/n) * sum X^i and pushed through the coset NTT - no per-point inversion.
    {
        std::vector<Fr> l0(n_, n_inv_);
        HIPCHK(hipMemcpyAsync(s.tmp.p, l0.data(), fn, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        CHK(l0_4_.alloc(f4));
        CHK(coset_ntt_4n(st, ptr<Fr>(s.tmp), n_, ptr<Fr>(l0_4_)));
    }
    // selector columns: Lagrange -> canonical -> coset
    const void* cols[5] = {d->ql, d->qr, d->qm, d->qo, d->qk};
    DevBuf* can[5] = {&ql_c_, &qr_c_, &qm_c_, &qo_c_, &qk_c_};
    DevBuf* cos[4] = {&eql_, &eqr_, &eqm_, &eqo_};
    for (int i = 0; i < 5; i++) {
        CHK(can[i]->alloc(fn));
        HIPCHK(hipMemcpyAsync(s.wl.p, cols[i], fn, hipMemcpyHostToDevice, st));
        if (i == 4) { CHK(qk_lag_trace_.alloc(fn)); HIPCHK(hipMemcpyAsync(qk_lag_trace_.p, s.wl.p, fn, hipMemcpyDeviceToDevice, st)); }
        CHK(inv_ntt_n(st, ptr<Fr>(s.wl), ptr<Fr>(*can[i])));
        if (i < 4) {
            CHK(cos[i]->alloc(f4));
            CHK(coset_ntt_4n(st, ptr<Fr>(*can[i]), n_, ptr<Fr>(*cos[i])));
            // into the quotient kernel's radix (kernels_poly.h): 32 q, and 1024 q for qm
            scale_kernel<FRP><<<cdiv(n4_, POLY_THREADS), POLY_THREADS, 0, st>>>(ptr<Fr>(*cos[i]), fr_u64(i == 2 ? 1u << 10 : 1u << 5), n4_); KCHK();
        }
        HIPCHK(hipStreamSynchronize(st));
    }
    // rows of Qk the prover writes per proof: public inputs 0..nb_public-1 and the commitment rows.  With few of them the
    // completed column never goes through iNTT + coset NTT again: the quotient kernel adds delta_j * L_row_j(x) instead.
    inj_row_.clear(); inj_trace_val_.clear();
    for (uint32_t i = 0; i < nb_public_; i++) inj_row_.push_back(i);
    for (uint32_t k = 0; k < nb_commit_; k++) inj_row_.push_back(nb_public_ + cci_[k]);
    qk_direct_ = inj_row_.size() <= (size_t)QK_INJECT_MAX && !getenv("APK_QK_NTT");
    if (qk_direct_) {
        CHK(eqk_trace_.alloc(f4));
        CHK(coset_ntt_4n(st, ptr<Fr>(qk_c_), n_, ptr<Fr>(eqk_trace_)));
        for (size_t j = 0; j < inj_row_.size(); j++) {
            const uint32_t row = inj_row_[j];
            if (row >= n_) { set_error("Qk row %u out of range", row); return APK_ERR_ARG; }
            inj_trace_val_.push_back(reinterpret_cast<const Fr*>(d->qk)[row]);
            if (row == 0) continue;   // L_0 is l0_4_
            // L_row(X) = (1/n) sum_i omega^(-row i) X^i
            CHK(inj_tab_[j].alloc(f4));
            CHK(powers(st, ptr<Fr>(s.tmp), n_, Fr::pow_u64(omega_inv_, row), n_inv_));
            CHK(coset_ntt_4n(st, ptr<Fr>(s.tmp), n_, ptr<Fr>(inj_tab_[j])));
        }
        HIPCHK(hipStreamSynchronize(st));
    }
    for (uint32_t k = 0; k < nb_commit_; k++) {
        CHK(qcp_c_[k].alloc(fn)); CHK(eqcp_[k].alloc(f4));
        HIPCHK(hipMemcpyAsync(s.wl.p, d->qcp[k], fn, hipMemcpyHostToDevice, st));
        CHK(inv_ntt_n(st, ptr<Fr>(s.wl), ptr<Fr>(qcp_c_[k])));
        CHK(coset_ntt_4n(st, ptr<Fr>(qcp_c_[k]), n_, ptr<Fr>(eqcp_[k])));
        scale_kernel<FRP><<<cdiv(n4_, POLY_THREADS), POLY_THREADS, 0, st>>>(ptr<Fr>(eqcp_[k]), fr_u64(1u << 5), n4_); KCHK();
        HIPCHK(hipStreamSynchronize(st));
    }
    // permutation polynomials: S_j[i] = u^(p/n) * omega^(p mod n), p = perm[j n + i]   (gnark trace.S)
    {
        std::vector<Fr> wpow(n_);
        {
            std::vector<Fr> half(n_ / 2);
            HIPCHK(hipMemcpy(half.data(), tw_n_.p, fn / 2, hipMemcpyDeviceToHost));
            for (uint32_t i = 0; i < n_ / 2; i++) { wpow[i] = half[i]; wpow[i + n_ / 2] = Fr::neg(half[i]); }
        }
        Fr us[3] = {Fr::one(), shift_, shift_ * shift_};
        std::vector<Fr> col(n_);
        for (int j = 0; j < 3; j++) {
            for (uint32_t i = 0; i < n_; i++) {
                int64_t p = d->perm[(size_t)j * n_ + i];
                if (p < 0 || p >= (int64_t)3 * n_) { set_error("perm[%zu]=%lld out of range", (size_t)j * n_ + i, (long long)p); return APK_ERR_ARG; }
                uint32_t blk = (uint32_t)(p / n_), pos = (uint32_t)(p % n_);
                col[i] = blk == 0 ? wpow[pos] : us[blk] * wpow[pos];
            }
            CHK(s_lag_[j].alloc(fn)); CHK(s_c_[j].alloc(fn)); CHK(es_[j].alloc(f4));
            HIPCHK(hipMemcpy(s_lag_[j].p, col.data(), fn, hipMemcpyHostToDevice));
            CHK(inv_ntt_n(st, ptr<Fr>(s_lag_[j]), ptr<Fr>(s_c_[j])));
            CHK(coset_ntt_4n(st, ptr<Fr>(s_c_[j]), n_, ptr<Fr>(es_[j])));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    // VK commitments: the 8+k MSMs of plonk.Setup (setup/setup.go:107,149), canonical basis
    const Fr* polys[8 + APK_MAX_COMMITMENTS] = {ptr<Fr>(ql_c_), ptr<Fr>(qr_c_), ptr<Fr>(qm_c_), ptr<Fr>(qo_c_), ptr<Fr>(qk_c_),
                                                ptr<Fr>(s_c_[0]), ptr<Fr>(s_c_[1]), ptr<Fr>(s_c_[2]), ptr<Fr>(qcp_c_[0]), ptr<Fr>(qcp_c_[1])};
    uint32_t lens[8 + APK_MAX_COMMITMENTS];
    for (uint32_t& l : lens) l = n_;
    CHK(commit_chunks(s, tab_can_, polys, lens, 8 + nb_commit_, vk_pts_));
    {   // the five of them that enter every proof's [lin] with a fresh coefficient: fixed-base tables on the host (a few ms)
        const Aff fixed[5] = {vk_pts_[VK_QL], vk_pts_[VK_QR], vk_pts_[VK_QM], vk_pts_[VK_QO], vk_pts_[VK_S3]};
        vk_fixed_.build(fixed, 5);
    }
    return APK_OK;
}

// =====================================================================================================================
// The driver: inputs on their way, a slot, then the four rounds with the transcript's challenges derived between them.
template <class FRP, class FPP, int CURVE_ID>
int CurveBackend<FRP, FPP, CURVE_ID>::prove(const void* L, const void* R, const void* O, bool on_device, const void* pub,
                                            const void* blinding, const void* const* pi2, apk_proof* out) {
    if (msm_only_) { set_error("MSM-only context cannot prove"); return APK_ERR_STATE; }
    HIPCHK(hipSetDevice(device_));
    const auto t_start = std::chrono::steady_clock::now();
    if (!L || !R || !O || !blinding || !out || (nb_public_ && !pub) || (nb_commit_ && !pi2)) { set_error("null argument to apk_prove"); return APK_ERR_ARG; }
    const size_t fn = (size_t)n_ * sizeof(Fr);
    // host inputs: on their way to the device on a copy stream BEFORE this caller queues for a proving slot (InputSet)
    InputGuard in(this);
    if (!on_device) {
        CHK(in.take());
        const void* src[3] = {L, R, O};
        for (int j = 0; j < 3; j++) HIPCHK(hipMemcpyAsync(in.set->w[j].p, src[j], fn, hipMemcpyHostToDevice, in.set->copy));
        for (uint32_t k = 0; k < nb_commit_; k++) {
            if (!pi2[k]) { set_error("null BSB22 column"); return APK_ERR_ARG; }
            HIPCHK(hipMemcpyAsync(in.set->pi2[k].p, pi2[k], fn, hipMemcpyHostToDevice, in.set->copy));
        }
        HIPCHK(hipEventRecord(in.set->ready, in.set->copy));
    }
    MemberGuard guard(this);
    ProofRun run{*guard.s, in.set, guard.s->stream};
    run.t_start = run.t_phase = t_start;
    run.bl = reinterpret_cast<const Fr*>(blinding);
    run.pubv = reinterpret_cast<const Fr*>(pub);
    run.out = out;
    memset(out, 0, sizeof *out);
    out->curve = CURVE_ID;
    out->nb_commitments = nb_commit_;
    run.dL = reinterpret_cast<const Fr*>(L);
    run.dR = reinterpret_cast<const Fr*>(R);
    run.dO = reinterpret_cast<const Fr*>(O);
    if (!on_device) {
        HIPCHK(hipStreamWaitEvent(run.st, in.set->ready, 0));
        run.dL = ptr<Fr>(in.set->w[0]); run.dR = ptr<Fr>(in.set->w[1]); run.dO = ptr<Fr>(in.set->w[2]);
        path(P_HOST_INPUTS);
    }
    // (a committed column is only read: the caller's device buffer, or the input set's copy of the caller's host buffer)
    for (uint32_t k = 0; k < nb_commit_; k++) run.pi2[k] = on_device ? reinterpret_cast<const Fr*>(pi2[k]) : ptr<Fr>(in.set->pi2[k]);

    CHK(round1_wires(run));
    mark(run, 0);
    // gamma, beta (templateLogicSigBN254.go:131-133)
    run.key = key_points();
    run.gamma = Proto::gamma(run.key, run.pubv, nb_public_, run.lro[0], run.lro[1], run.lro[2], run.gamma_raw);
    run.beta = Proto::beta(run.gamma_raw, run.beta_raw);
    run.beta_u = run.beta * shift_; run.beta_u2 = run.beta_u * shift_;
    CHK(round2_grand_product(run));
    mark(run, 1);
    run.alpha = Proto::alpha(run.beta_raw, run.bsb, nb_commit_, run.zcom, run.alpha_raw);
    const int rc3 = round3_quotient(run);
    // (the witness does not satisfy the circuit: round 3 had just drained the stream, nothing of this proof is still reading its inputs)
    if (rc3 == APK_ERR_WITNESS) in.ok = guard.ok = true;
    if (rc3 != APK_OK) return rc3;
    mark(run, 2);
    run.zeta = Proto::zeta(run.alpha_raw, run.hcom, run.zeta_raw);
    CHK(round4_openings(run));
    memcpy(out->gamma, &run.gamma, sizeof(Fr)); memcpy(out->beta, &run.beta, sizeof(Fr)); memcpy(out->alpha, &run.alpha, sizeof(Fr));
    memcpy(out->zeta, &run.zeta, sizeof(Fr)); memcpy(out->gamma_kzg, &run.gk, sizeof(Fr));
    mark(run, 3);
    in.ok = true;
    guard.ok = true;
    path(P_PROOFS);
    if (stats_on_) {
        double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        std::lock_guard<std::mutex> g(stats_mu_);
        stats_.prove_ms += ms;
        stats_.proofs += 1;
        for (int r = 0; r < 4; r++) stats_.round_ms[r] += run.phase_ms[r];
        stats_.host_lincomb_ms += run.lincomb_ms;
    }
    return APK_OK;
}

// [L][R][O] over the Lagrange SRS (gnark's way) or over the canonical one: the same group elements, so the choice is about
// work only.  Over the Lagrange SRS the scalars are the witness values - in real circuits mostly 0, 1 or small, i.e. few
// non-zero digits on the plain table - over the canonical SRS they are the uniform coefficients of the blinded polynomial.
// auto: the Lagrange route when the wires' non-zero digits (msm_density_kernel, every 16th proof of the context; the first
// proof waits for its own count) are below 90 % of what uniform scalars have.  Never with a commit hook installed (the
// multi-GPU schedules deal canonical batches).  Sets run.use_lag; run.measuring says that a count is on its way to the host:
// wire_route_finish() takes it once the stream has been waited for.
template <class FRP, class FPP, int CURVE_ID>
int CurveBackend<FRP, FPP, CURVE_ID>::wire_route(ProofRun& run) {
    Slot& s = run.s;
    hipStream_t st = run.st;
    const uint32_t n = n_;
    constexpr uint32_t DENSITY_UNKNOWN = 0xffffffffu;
    run.use_lag = run.measuring = false;
    if (!lagrange_possible() || hook_ || wires_lag_mode_ == 0) return APK_OK;
    const uint32_t seq = proof_seq_.fetch_add(1, std::memory_order_relaxed);
    uint32_t pm = wire_density_pm_.load(std::memory_order_relaxed);
    if (wires_lag_mode_ == 1) run.use_lag = true;
    else {
        run.measuring = pm == DENSITY_UNKNOWN || (seq & 15u) == 0;
        if (run.measuring) {
            uint32_t* d_cnt = ptr<uint32_t>(s.tail_flag) + 2;
            HIPCHK(hipMemsetAsync(d_cnt, 0, 4, st));
            MsmBatchArgs da{};
            da.batch = 3;
            const Fr* wires[3] = {run.dL, run.dR, run.dO};
            for (int j = 0; j < 3; j++) { da.scalars[j] = wires[j]; da.len[j] = n; }
            msm_density_kernel<FRP><<<dim3(cdiv(n, 256) < 512 ? cdiv(n, 256) : 512, 3), 256, 0, st>>>(da, msm_ctx_.win, d_cnt); KCHK();
            HIPCHK(hipMemcpyAsync(pin_host<uint32_t>(s.h_pinned, PIN_DENSITY), d_cnt, 4, hipMemcpyDeviceToHost, st));
        }
        if (pm == DENSITY_UNKNOWN) {        // the context's first proof: wait for the count
            HIPCHK(hipStreamSynchronize(st));
            pm = wire_route_finish(run);
        }
        run.use_lag = pm < 900u;
    }
    // (automatic mode without a caller's Lagrange SRS: the table is derived now, once, on this proof's stream - or not at all)
    if (run.use_lag && !lagrange_ready()) run.use_lag = ensure_lagrange_table(st);
    return APK_OK;
}
// the count has reached the host: the wires' non-zero digits per mille of what uniform scalars have, kept for the proofs to come
template <class FRP, class FPP, int CURVE_ID>
uint32_t CurveBackend<FRP, FPP, CURVE_ID>::wire_route_finish(ProofRun& run) {
    const uint32_t count = *pin_host<const volatile uint32_t>(run.s.h_pinned, PIN_DENSITY);
    const uint32_t pm = (uint32_t)((uint64_t)count * 1000u / ((uint64_t)3 * n_ * msm_ctx_.W));
    wire_density_pm_.store(pm, std::memory_order_relaxed);
    run.measuring = false;
    return pm;
}

// ---------------- round 1: wire polynomials, BSB22 commitments, completed Qk -----------------------------------------
template <class FRP, class FPP, int CURVE_ID>
int CurveBackend<FRP, FPP, CURVE_ID>::round1_wires(ProofRun& run) {
    Slot& s = run.s;
    hipStream_t st = run.st;
    const uint32_t n = n_;
    const size_t fn = (size_t)n_ * sizeof(Fr);
    const Aff* hp = pin_host<Aff>(s.h_pinned, PIN_AFF);
    for (uint32_t k = 0; k < nb_commit_; k++) {
        // kzg.Commit(pi2, Lagrange SRS) then hash_to_field (templateLogicSigBN254.go:386-397)
        const Fr* col = run.pi2[k];
        MsmBatchArgs a{};
        a.batch = 1; a.scalars[0] = col; a.len[0] = n; a.offset[0] = 0;
        CHK(commit(s, tab_lag_, 1, a));
        CHK(inv_ntt_n(st, col, ptr<Fr>(s.pi2_can[k])));
        {
            const Fr* cin = ptr<Fr>(s.pi2_can[k]); Fr* eout = ptr<Fr>(s.epi2[k]);
            CHK(coset_eval(st, 1, &cin, &n, &eout));
        }
        CHK(sync_results(s));
        run.bsb[k] = hp[0];
        run.cval[k] = Proto::hash_fr(run.bsb[k]);
        store_pt(run.out->bsb22[k], run.bsb[k]);
    }
    Fr* canon[3] = {ptr<Fr>(s.cl), ptr<Fr>(s.cr), ptr<Fr>(s.co)};
    const Fr* wires[3] = {run.dL, run.dR, run.dO};
    CHK(wire_route(run));
    const bool use_lag = run.use_lag;
    Fr* lagv[3] = {ptr<Fr>(s.wl), ptr<Fr>(s.wr), ptr<Fr>(s.wo)};
    if (use_lag)
        for (int j = 0; j < 3; j++) HIPCHK(hipMemcpyAsync(lagv[j], wires[j], fn, hipMemcpyDeviceToDevice, st));
    // (no zero-fill of the tails: blind_kernel assigns the coefficients n .. n+d-1 and nothing reads beyond them)
    {
        const uint32_t lens[3] = {n, n, n};
        CHK(run_ntt_batch(st, 0, true, 3, wires, canon, lens, n, nullptr, nullptr, ptr<Fr>(scales_)));
    }
    {
        Blind3<FRP> b3{};
        for (int j = 0; j < 3; j++) {
            b3.p[j] = canon[j]; b3.b[j].v[0] = run.bl[2 * j]; b3.b[j].v[1] = run.bl[2 * j + 1];
            b3.lag[j] = use_lag ? lagv[j] : nullptr;     // the blinding scalars behind the n witness values: the scalars of D_0, D_1
        }
        CHK((klaunch<Blind3K<FRP>, 256>(st, 3, 64, 0, b3, n, 2)));
    }
    const int fill = run.fill = tail_fill(s);
    if (fill) path(P_TAIL_FILL);
    {
        MsmBatchArgs a{};
        a.batch = 3;
        for (int j = 0; j < 3; j++) { a.scalars[j] = use_lag ? lagv[j] : canon[j]; a.len[j] = n + 2; a.offset[j] = 0; }
        a.plain = use_lag ? 1u : 0u;
        if (use_lag) path(P_LAGRANGE_WIRES);
        s.mark_acc = fill;
        const int rc = use_lag ? commit(s, tab_lag_, 1, a) : commit(s, tab_can_, 0, a);
        s.mark_acc = 0;
        CHK(rc);
    }
    // completed Qk: public inputs and commitment values written into the Lagrange column, then iNTT
    if (!qk_direct_) {
        HIPCHK(hipMemcpyAsync(s.qk_lag.p, qk_lag_trace_.p, fn, hipMemcpyDeviceToDevice, st));
        if (nb_public_) HIPCHK(hipMemcpyAsync(s.qk_lag.p, run.pubv, (size_t)nb_public_ * sizeof(Fr), hipMemcpyHostToDevice, st));
        for (uint32_t k = 0; k < nb_commit_; k++)
            HIPCHK(hipMemcpyAsync(ptr<Fr>(s.qk_lag) + nb_public_ + cci_[k], &run.cval[k], sizeof(Fr), hipMemcpyHostToDevice, st));
        CHK(inv_ntt_n(st, ptr<Fr>(s.qk_lag), ptr<Fr>(s.qk_can)));
        CHK(coset_ntt_4n(st, ptr<Fr>(s.qk_can), n, ptr<Fr>(s.eqk)));
    }
    {
        Fr* ev[3] = {ptr<Fr>(s.el), ptr<Fr>(s.er), ptr<Fr>(s.eo)};
        const uint32_t lens[3] = {n + 2, n + 2, n + 2};
        if (wire_hook_ && !sc_.on()) {
            // per-wire transforms dealt to other GPUs (csrc/comm.cpp): the hook returns with the three
            // evaluation vectors complete in this context's memory
            HIPCHK(hipStreamSynchronize(st));
            const void* cin[3] = {canon[0], canon[1], canon[2]};
            void* eout[3] = {ev[0], ev[1], ev[2]};
            hook_slot() = &s;
            const int rc = wire_hook_(wire_hook_user_, 3, cin, lens, eout);
            hook_slot() = nullptr;
            if (rc != APK_OK) { set_error("wire hook failed with %d", rc); return rc == APK_ERR_ARG ? APK_ERR_ARG : APK_ERR_STATE; }
        } else if (fill) {
            CHK(side_begin(s));
            CHK(run_ntt_batch(s.side, 1, false, 3, canon, ev, lens, n4_, ptr<Fr>(coset_pre_), nullptr, nullptr, 0, true));   // semi-canonical: coset_eval
            CHK(side_end(s));
        } else {
            CHK(coset_eval(st, 3, canon, lens, ev));
        }
    }
    CHK(sync_results(s));
    if (run.measuring) wire_route_finish(run);
    for (int j = 0; j < 3; j++) { run.lro[j] = hp[j]; store_pt(run.out->lro[j], run.lro[j]); }
    return APK_OK;
}

// ---------------- round 2: grand product Z --------------------------------------------------------
template <class FRP, class FPP, int CURVE_ID>
int CurveBackend<FRP, FPP, CURVE_ID>::round2_grand_product(ProofRun& run) {
    Slot& s = run.s;
    hipStream_t st = run.st;
    const uint32_t n = n_;
    const int fill = run.fill;
    {
        Fr* hfr = pin_host<Fr>(s.h_pinned, PIN_FR);
        const GpScan<FRP> g = poly_gp_scan<FRP>(ptr<Fr>(s.ratio), ptr<Fr>(s.tmp), ptr<Fr>(s.scan_tot), n);
        // (the kernel multiplies on unsaturated limbs: the challenges in the product's radix R' = 32 R)
        CHK(poly_gp_terms<FRP>(kl(), st, run.dL, run.dR, run.dO, (const Fr*)ptr<Fr>(s_lag_[0]), (const Fr*)ptr<Fr>(s_lag_[1]), (const Fr*)ptr<Fr>(s_lag_[2]),
                               (const Fr*)ptr<Fr>(tw_n_), n, run.beta * fr_u64(32), run.gamma, run.beta_u * fr_u64(32), run.beta_u2 * fr_u64(32), g));
        Fr* const tot_pin = pin_dev<Fr>(s.d_pinned, PIN_FR);     // hfr[0], from the device
        Fr* const tot_out = tot_pin ? tot_pin : poly_gp_total_slot<FRP>(g, n);
        CHK(poly_gp_scans<FRP>(kl(), st, g, n, tot_out));
        if (!tot_pin) HIPCHK(hipMemcpyAsync(hfr, tot_out, sizeof(Fr), hipMemcpyDeviceToHost, st));
        CHK(sync_results(s));
        CHK(poly_gp_finish<FRP>(kl(), st, g, n, hfr[0], ptr<Fr>(s.zlag)));
    }
    CHK(inv_ntt_n(st, ptr<Fr>(s.zlag), ptr<Fr>(s.cz)));
    {
        Fr4<FRP> b{};
        b.v[0] = run.bl[6]; b.v[1] = run.bl[7]; b.v[2] = run.bl[8];
        CHK((klaunch<BlindK<FRP>, 256>(st, 1, 64, 0, ptr<Fr>(s.cz), n, b, 3)));
        MsmBatchArgs a{};
        a.batch = 1; a.scalars[0] = s.cz.p; a.len[0] = n + 3; a.offset[0] = 0;
        s.mark_acc = fill;
        const int rc = commit(s, tab_can_, 0, a);
        s.mark_acc = 0;
        CHK(rc);
    }
    if (fill) {
        CHK(side_begin(s));
        CHK(coset_ntt_4n(s.side, ptr<Fr>(s.cz), n + 3, ptr<Fr>(s.ez), true));   // semi-canonical: coset_eval
        CHK(side_end(s));
    } else {
        const Fr* cin = ptr<Fr>(s.cz); Fr* eout = ptr<Fr>(s.ez);
        const uint32_t zl = n + 3;
        CHK(coset_eval(st, 1, &cin, &zl, &eout));
        if (sc_.on() && sc_.glog == 3) {   // Z(omega X) lives in class (k + 4) mod 8: evaluated there as well (eqk is free: Qk is completed in the kernel)
            Fr* e2 = ptr<Fr>(s.eqk);
            CHK(coset_eval(st, 1, &cin, &zl, &e2, 1));
        }
    }
    CHK(sync_results(s));
    run.zcom = pin_host<Aff>(s.h_pinned, PIN_AFF)[0];
    store_pt(run.out->z, run.zcom);
    return APK_OK;
}

// the quotient kernel's arguments on the whole 4n coset (round 3 narrows them for a sub-coset)
template <class FRP, class FPP, int CURVE_ID>
QuotientArgs<FRP> CurveBackend<FRP, FPP, CURVE_ID>::quotient_args(const ProofRun& run) {
    Slot& s = run.s;
    QuotientArgs<FRP> q{};
    q.l = ptr<Fr>(s.el); q.r = ptr<Fr>(s.er); q.o = ptr<Fr>(s.eo); q.z = ptr<Fr>(s.ez); q.qk = ptr<Fr>(s.eqk);
    if (qk_direct_) {
        q.qk = ptr<Fr>(eqk_trace_);
        q.nb_inject = (int)inj_row_.size();
        for (size_t j = 0; j < inj_row_.size(); j++) {
            const Fr written = j < nb_public_ ? run.pubv[j] : run.cval[j - nb_public_];
            q.inj_delta[j] = written - inj_trace_val_[j];
            q.inj_tab[j] = inj_row_[j] == 0 ? ptr<Fr>(l0_4_) : ptr<Fr>(inj_tab_[j]);
        }
    }
    q.ql = ptr<Fr>(eql_); q.qr = ptr<Fr>(eqr_); q.qm = ptr<Fr>(eqm_); q.qo = ptr<Fr>(eqo_);
    q.s1 = ptr<Fr>(es_[0]); q.s2 = ptr<Fr>(es_[1]); q.s3 = ptr<Fr>(es_[2]);
    q.x = ptr<Fr>(x4_); q.l0 = ptr<Fr>(l0_4_);
    q.nb_commit = (int)nb_commit_;
    for (uint32_t k = 0; k < nb_commit_; k++) { q.qcp[k] = ptr<Fr>(eqcp_[k]); q.pi2[k] = ptr<Fr>(s.epi2[k]); }
    // the kernel multiplies in the radix R' = 32 R: constants carry the factors its header lists
    const Fr c5 = fr_u64(1u << 5), c10 = fr_u64(1u << 10), c20 = fr_u64(1u << 20);
    q.alpha = run.alpha * c20; q.beta = run.beta * c5; q.gamma = run.gamma; q.beta_u = run.beta_u * c5; q.beta_u2 = run.beta_u2 * c5;
    q.alpha2 = run.alpha * run.alpha * c10;
    for (int k = 0; k < 4; k++) q.zh_inv[k] = zh_inv_[k] * c5;
    for (int j = 0; j < q.nb_inject; j++) q.inj_delta[j] = q.inj_delta[j] * c5;
    q.n4 = n4_;
    return q;
}

// ---------------- round 3: quotient on the 4n coset ------------------------------------------------------------------
// APK_ERR_WITNESS: the quotient is not a polynomial; the stream has been waited for when that is known.
template <class FRP, class FPP, int CURVE_ID>
int CurveBackend<FRP, FPP, CURVE_ID>::round3_quotient(ProofRun& run) {
    Slot& s = run.s;
    hipStream_t st = run.st;
    const uint32_t n = n_;
    {
        QuotientArgs<FRP> q = quotient_args(run);
        if (!sc_.on()) {
            CHK((klaunch<QuotientK<FRP>, POLY_THREADS>(st, cdiv(n4_, POLY_THREADS), POLY_THREADS, 0, q, ptr<Fr>(s.quot))));
            CHK(run_ntt(st, 1, true, ptr<Fr>(s.quot), ptr<Fr>(s.hcan), n4_, n4_, nullptr, ptr<Fr>(coset_post_inv_), nullptr));
        } else {
            // sub-coset split: the quotient on this rank's m points, the local part of the inverse transform, ONE all-gather,
            // the last log2(G) stages on every rank - hcan comes out bit for bit as above
            const uint32_t m = n4_ >> sc_.glog;
            q.n4 = m; q.sub_k = (uint32_t)sc_.k; q.sub_glog = (uint32_t)sc_.glog; q.zs = ptr<Fr>(s.eqk);
            quotient_kernel<FRP><<<cdiv(m, POLY_THREADS), POLY_THREADS, 0, st>>>(q, ptr<Fr>(s.quot)); KCHK();
            Fr* mine = ptr<Fr>(s.sc_gather) + (size_t)sc_.k * m;
            CHK(run_ntt(st, 1, true, ptr<Fr>(s.quot), mine, m, m, nullptr, ptr<Fr>(sc_.post), nullptr, sc_.glog));
            HIPCHK(hipStreamSynchronize(st));
            hook_slot() = &s;
            const int grc = sc_.hook(sc_.user, s.sc_gather.p, (size_t)m * sizeof(Fr));
            hook_slot() = nullptr;
            if (grc != APK_OK) { set_error("sub-coset gather hook failed with %d", grc); return grc == APK_ERR_ARG ? APK_ERR_ARG : APK_ERR_STATE; }
            SubMergeArgs<FRP> ma{};
            for (int e = 0; e < 8; e++) ma.rho_inv[e] = sc_.rho_inv[e];
            ma.m = m; ma.glog = (uint32_t)sc_.glog;
            subcoset_merge_kernel<FRP><<<cdiv(m, POLY_THREADS), POLY_THREADS, 0, st>>>(ma, ptr<Fr>(s.sc_gather), ptr<Fr>(coset_post_inv_), ptr<Fr>(s.hcan)); KCHK();
        }
        // h = h1 + X^(n+2) h2 + X^(2(n+2)) h3   (templateLogicSigBN254.go:79,220-226)
        MsmBatchArgs a{};
        a.batch = 3;
        for (int j = 0; j < 3; j++) { a.scalars[j] = ptr<Fr>(s.hcan) + (size_t)j * (n + 2); a.len[j] = n + 2; a.offset[j] = 0; }
        CHK(commit(s, tab_can_, 0, a));
        // the quotient is a polynomial of degree < 3n+6 iff the witness satisfies the circuit: every coefficient of the tail
        // h[3(n+2) .. 4n) must vanish (OR-reduce on the device, one flag word back)
        s.epoch++;
        const uint32_t tail4 = (n4_ - 3 * (n + 2)) * (uint32_t)(sizeof(Fr) / 16);
        uint32_t* const flag_pin = pin_dev<uint32_t>(s.d_pinned, PIN_TAIL);
        CHK(poly_tail_nonzero(kl(), st, reinterpret_cast<const uint4*>(ptr<Fr>(s.hcan) + 3 * (size_t)(n + 2)), tail4, s.epoch,
                              flag_pin ? flag_pin : ptr<uint32_t>(s.tail_flag)));
        if (!flag_pin) HIPCHK(hipMemcpyAsync(pin_host<uint32_t>(s.h_pinned, PIN_TAIL), s.tail_flag.p, 4, hipMemcpyDeviceToHost, st));
    }
    CHK(sync_results(s));
    if (*pin_host<const volatile uint32_t>(s.h_pinned, PIN_TAIL) == s.epoch) {
        set_error("quotient is not a polynomial: the witness does not satisfy the circuit");
        return APK_ERR_WITNESS;
    }
    const Aff* hp = pin_host<Aff>(s.h_pinned, PIN_AFF);
    for (int j = 0; j < 3; j++) { run.hcom[j] = hp[j]; store_pt(run.out->h[j], run.hcom[j]); }
    return APK_OK;
}

// the tables of powers round 4 evaluates and divides with: zeta^i, (omega zeta)^i and their inverses, n + 3 of each
template <class FRP, class FPP, int CURVE_ID>
int CurveBackend<FRP, FPP, CURVE_ID>::zeta_powers(ProofRun& run) {
    Slot& s = run.s;
    hipStream_t st = run.st;
    const uint32_t n = n_;
    const Fr& zeta = run.zeta;
    const Fr zw = zeta * omega_;
    const bool z0 = zeta.is_zero();
    const Fr zeta_inv = Fr::inv(zeta), zw_inv = zeta_inv * omega_inv_;   // (one host inversion, ~10 us, before the launches below)
    Fr* outs[4] = {ptr<Fr>(s.pw_z), ptr<Fr>(s.pw_zw), ptr<Fr>(s.pw_zi), ptr<Fr>(s.pw_zwi)};
    const Fr ws[4] = {zeta, zw, zeta_inv, zw_inv};
    if (z0 || !prover_knobs().powers_derive) return powers_batch(st, z0 ? 2 : 4, outs, ws, n + 3);
    // zeta^i and zeta^-i by square-and-multiply walks (~6 products per element); (omega zeta)^(+-i) from them and the
    // transform's own table of omega^j: one product per element
    Fr* two[2] = {outs[0], outs[2]};
    const Fr w2[2] = {zeta, zeta_inv};
    CHK(powers_batch(st, 2, two, w2, n + 3));
    DerivePowers<FRP> dp{};
    dp.in[0] = outs[0]; dp.out[0] = outs[1]; dp.inverse[0] = 0;
    dp.in[1] = outs[2]; dp.out[1] = outs[3]; dp.inverse[1] = 1;
    return klaunch<DerivePowersK<FRP>, POLY_THREADS>(st, dim3(cdiv(n + 3, POLY_THREADS), 2), POLY_THREADS, 0, dp, (const Fr*)ptr<Fr>(twu_n_), n, n + 3);
}

// [lin] = sum coef_i * [poly_i]: the group element kzg.Commit(lin) would give, taken from commitments already in hand
// (host_msm.h) instead of a tenth size-n MSM.  lin_h: the [H] part where round 4 took it early, else null.
template <class FRP, class FPP, int CURVE_ID>
typename CurveBackend<FRP, FPP, CURVE_ID>::Aff CurveBackend<FRP, FPP, CURVE_ID>::lin_commitment(ProofRun& run, const LinTerm* terms, int count,
                                                                                                HostPool* pool, const HostSum* lin_h) {
    const ProverKnobs& kn = prover_knobs();
    // the [H] part was taken earlier when the pool was there; [Qk] has coefficient one: a plain addition
    Aff lp[HOST_MSM_MAX];
    Fr lk[HOST_MSM_MAX];
    // [Ql][Qr][Qm][Qo][S3] come out of the context's fixed-base tables: 33 additions each
    int cnt = 0;
    for (int i = 0; i < count; i++) {
        if (i == LT_QK || (lin_h && i >= LT_H1 && i <= LT_H3) || (kn.host_fixed && (i <= LT_QO || i == LT_S3))) continue;
        lp[cnt] = terms[i].com; lk[cnt] = terms[i].coef; cnt++;
    }
    const auto t_lc = std::chrono::steady_clock::now();
    HostSum sum = host_lincomb_sum<FRP, FPP>(lp, lk, cnt, pool, kn.host_glv);
    if (kn.host_fixed) {
        const Fr fk[5] = {terms[LT_QL].coef, terms[LT_QR].coef, terms[LT_QM].coef, terms[LT_QO].coef, terms[LT_S3].coef};
        vk_fixed_.template accumulate<FRP>(sum, fk);
    }
    if (lin_h) sum.add(*lin_h);
    {
        using F64 = Fe64<FPP>;
        sum.madd(Affine<FPP, F64>{F64::from(run.key.qk.x), F64::from(run.key.qk.y)});
    }
    const Aff lin_com = host_xyzz_to_affine<FPP>(sum);
    if (stats_on_) run.lincomb_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_lc).count();
    return lin_com;
}

// ---------------- round 4: evaluations, linearised polynomial, openings ----------------------------------------------
template <class FRP, class FPP, int CURVE_ID>
int CurveBackend<FRP, FPP, CURVE_ID>::round4_openings(ProofRun& run) {
    Slot& s = run.s;
    hipStream_t st = run.st;
    const uint32_t n = n_;
    const ProverKnobs& kn = prover_knobs();
    const Fr& zeta = run.zeta;
    const Aff* hp = pin_host<Aff>(s.h_pinned, PIN_AFF);
    Fr* hfr = pin_host<Fr>(s.h_pinned, PIN_FR);
    // what the batched opening at zeta folds beside lin, in the fold's order (Proto::fold): L, R, O, S1, S2, Qcp_k
    const Fr* opened[5 + APK_MAX_COMMITMENTS] = {ptr<Fr>(s.cl), ptr<Fr>(s.cr), ptr<Fr>(s.co), ptr<Fr>(s_c_[0]), ptr<Fr>(s_c_[1])};
    uint32_t opened_len[5 + APK_MAX_COMMITMENTS] = {n + 2, n + 2, n + 2, n, n};
    for (uint32_t k = 0; k < nb_commit_; k++) { opened[5 + k] = ptr<Fr>(qcp_c_[k]); opened_len[5 + k] = n; }
    const int nb_opened = 5 + (int)nb_commit_;
    typename Proto::AtZeta at;   // PI(zeta), L_0(zeta), the scalars of [H1..3]: worked out below while the GPU evaluates
    // the context's parked host threads for the [lin] combination (ProverKnobs::lc_threads)
    HostPool* pool = nullptr;
    const bool host_idle = !device_load_over(2);     // no other proofs' threads competing for the host while the GPU works on this one
    if (kn.lc_threads > 1 && host_idle) {
        std::lock_guard<std::mutex> lk2(mu_);
        if (!lc_pool_) lc_pool_.reset(new HostPool(kn.lc_threads - 1));
        pool = lc_pool_.get();
        path(P_LINCOMB_POOL);
    }
    HostSum lin_h = HostSum::inf();
    bool lin_h_done = false;
    const bool z0 = zeta.is_zero();
    CHK(zeta_powers(run));
    // the two opening quotients of round 4 as ONE batched launch sequence (poly_run.h poly_kzg_quotient_batch; measurement:
    // profiles/launch_chain_ab.txt).  zeta = 0 keeps the two sequences: its quotients are plain shifts.
    const bool open_pair = kn.open_pair && !z0;
    Fr ev[EVAL_MAX];
    {
        EvalArgs<FRP> ea{};
        for (int i = 0; i < nb_opened; i++) { ea.f[i] = opened[i]; ea.len[i] = opened_len[i]; }
        ea.count = nb_opened;
        // Z(omega*zeta) rides in the same launch with its own table of powers
        const int iz = ea.count;
        ea.f[iz] = ptr<Fr>(s.cz); ea.len[iz] = n + 3; ea.pw[iz] = ptr<Fr>(s.pw_zw); ea.count++;
        CHK(eval_many(s, ea, ptr<Fr>(s.pw_z), hfr));
        // The opening quotient of Z at omega*zeta does not wait for anything the host derives from the evaluations - but the host
        // waits for the stream below, so its five launches stood between the evaluations and the host all the same.  It rides
        // with the folded polynomial's quotient instead (open_pair): three launches for the two.  APK_OPEN_PAIR=0: here, alone.
        if (!open_pair) CHK(kzg_quotient(s, ptr<Fr>(s.cz), n + 3, ptr<Fr>(s.pw_zw), ptr<Fr>(s.pw_zwi), z0, ptr<Fr>(s.q2)));
        // [lin] (below) is a combination of commitments the host holds; the coefficients of [H1..3] depend on zeta alone, so a
        // lone proof's host thread works that part out while the GPU evaluates (the rest needs the evaluations).  With other
        // proofs in flight it stays one pass: a second pass repeats the doublings, and the host is what those proofs share.
        // PI(zeta) and L_0(zeta), over the rows the prover wrote into Qk (public inputs, commitment hashes), need no evaluation
        // either.  at.ok is not looked at: zeta on the domain has probability ~ n / r and the verifier refuses such a proof.
        at = Proto::at_zeta(zeta, n, omega_, n_inv_, run.pubv, nb_public_, run.cval, cci_, nb_commit_);
        if (host_idle && kn.lin_early_h && (pool || FPP::N <= 8)) {   // (one thread takes longer over BLS12-381's three than the GPU over the evaluations)
            const auto t_lc = std::chrono::steady_clock::now();
            lin_h = host_lincomb_sum<FRP, FPP>(run.hcom, at.h, 3, pool, kn.host_glv);
            lin_h_done = true;
            if (stats_on_) run.lincomb_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_lc).count();
        }
        CHK(sync_results(s));
        const Fr c32 = fr_u64(32);        // eval_partial_kernel multiplies value x value on the product's radix: f(z) / 32 comes back
        for (int i = 0; i < ea.count; i++) ev[i] = hfr[i] * c32;
    }
    typename Proto::Evals e{ev[0], ev[1], ev[2], ev[3], ev[4], {}, ev[5 + nb_commit_]};
    for (uint32_t k = 0; k < nb_commit_; k++) e.qcp[k] = ev[5 + k];
    // lin(zeta), and which scalar multiplies which constituent of the linearised polynomial
    const typename Proto::LinScalars lin_sc = Proto::lin_scalars(run.gamma, run.beta, run.alpha, zeta, shift_, at, e);
    const typename Proto::LinCoefs lcf = Proto::lin_coefs(e, at, lin_sc, nb_commit_);
    const Fr* const hcan = ptr<Fr>(s.hcan);
    LinTerm lin_terms[LT_MAX] = {
        {ptr<Fr>(ql_c_), n, run.key.ql, lcf.ql}, {ptr<Fr>(qr_c_), n, run.key.qr, lcf.qr}, {ptr<Fr>(qm_c_), n, run.key.qm, lcf.qm},
        {ptr<Fr>(qo_c_), n, run.key.qo, lcf.qo}, {ptr<Fr>(qk_c_), n, run.key.qk, Fr::one()}, {ptr<Fr>(s_c_[2]), n, run.key.s3, lcf.s3},
        {ptr<Fr>(s.cz), n + 3, run.zcom, lcf.z}, {hcan, n + 2, run.hcom[0], lcf.h[0]},
        {hcan + (n + 2), n + 2, run.hcom[1], lcf.h[1]}, {hcan + 2 * (size_t)(n + 2), n + 2, run.hcom[2], lcf.h[2]}};
    for (uint32_t k = 0; k < nb_commit_; k++) lin_terms[LT_BSB + k] = {ptr<Fr>(s.pi2_can[k]), n, run.bsb[k], lcf.bsb[k]};
    const int nb_terms = LT_BSB + (int)nb_commit_;
    const Aff lin_com = lin_commitment(run, lin_terms, nb_terms, pool, lin_h_done ? &lin_h : nullptr);
    memcpy(run.out->zshift_value, &e.zw, sizeof(Fr));
    Fr claimed[6 + APK_MAX_COMMITMENTS] = {lin_sc.lin_z, e.l, e.r, e.o, e.s1, e.s2};
    for (uint32_t k = 0; k < nb_commit_; k++) claimed[6 + k] = e.qcp[k];
    for (uint32_t i = 0; i < 6 + nb_commit_; i++) memcpy(run.out->claimed_values[i], &claimed[i], sizeof(Fr));
    // gamma' for the batched opening (templateLogicSigBN254.go:280-286) and its powers; the folded claim is the verifier's
    run.gk = Proto::gamma_kzg(zeta, lin_com, run.lro[0], run.lro[1], run.lro[2], run.key, lin_sc.lin_z, e, run.gk_raw);
    Fr gpow[5 + APK_MAX_COMMITMENTS];
    (void)Proto::fold(run.gk, lin_sc.lin_z, e, nb_commit_, gpow);
    {
        // folded = lin + gk l + gk^2 r + gk^3 o + gk^4 S1 + gk^5 S2 + gk^(6+k) Qcp_k, one fused linear combination over the
        // constituents of lin (the linearised polynomial itself is never materialised)
        LinCombArgs<FRP> lc{};
        int c = 0;
        for (int i = 0; i < nb_terms; i++, c++) { lc.f[c] = lin_terms[i].poly; lc.len[c] = lin_terms[i].len; lc.coef[c] = lin_terms[i].coef; }
        for (int i = 0; i < nb_opened; i++, c++) { lc.f[c] = opened[i]; lc.len[c] = opened_len[i]; lc.coef[c] = gpow[i]; }
        lc.count = c; lc.out_len = n + 3;
        {   // the kernel multiplies on unsaturated limbs: coefficients in the product's radix R' = 32 R
            const Fr c32 = fr_u64(32);
            for (int k = 0; k < c; k++) lc.coef[k] = lc.coef[k] * c32;
        }
        CHK((klaunch<LincombK<FRP>, POLY_THREADS>(st, cdiv(n + 3, POLY_THREADS), POLY_THREADS, 0, lc, ptr<Fr>(s.folded))));
        if (open_pair) {
            // W_zeta and W_omega*zeta divide different polynomials at different points: neither needs the other (the folded
            // polynomial is only needed by its own division), so one sequence of three launches carries both
            KzgQuotBatch<FRP> qb{};
            const uint32_t sb = poly_scan_blocks(n + 3);
            qb.f[0] = ptr<Fr>(s.folded); qb.pw[0] = ptr<Fr>(s.pw_z); qb.pwi[0] = ptr<Fr>(s.pw_zi); qb.tmp[0] = ptr<Fr>(s.tmp); qb.tot[0] = ptr<Fr>(s.scan_tot); qb.q[0] = ptr<Fr>(s.q1);
            qb.f[1] = ptr<Fr>(s.cz); qb.pw[1] = ptr<Fr>(s.pw_zw); qb.pwi[1] = ptr<Fr>(s.pw_zwi); qb.tmp[1] = ptr<Fr>(s.tmp2); qb.tot[1] = ptr<Fr>(s.scan_tot) + sb; qb.q[1] = ptr<Fr>(s.q2);
            qb.len[0] = qb.len[1] = n + 3;
            CHK(poly_kzg_quotient_batch<FRP>(kl(), st, qb, 2));
        } else {
            CHK(kzg_quotient(s, ptr<Fr>(s.folded), n + 3, ptr<Fr>(s.pw_z), ptr<Fr>(s.pw_zi), z0, ptr<Fr>(s.q1)));
        }
        // both opening proofs in one batch: W_zeta (batched opening) and W_omega*zeta (kzg.Open of Z [UPSTREAM])
        MsmBatchArgs a{};
        a.batch = 2;
        a.scalars[0] = s.q1.p; a.len[0] = n + 2; a.offset[0] = 0;
        a.scalars[1] = s.q2.p; a.len[1] = n + 2; a.offset[1] = 0;
        CHK(commit(s, tab_can_, 0, a));
    }
    CHK(sync_results(s));
    store_pt(run.out->zshift_h, hp[1]);
    store_pt(run.out->batched_h, hp[0]);
    return APK_OK;
}

}  // namespace apk
