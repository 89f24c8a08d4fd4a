// BLS12-381 instantiation of the batch verifier's device kernels (kernels_lincomb.h): segmented variable-base G1 sums and the
// per-point checks - and of the fold of many coset openings' values (kernels_kzg_cosets_fold.h).  A translation unit of its own, so that it compiles next to the two backends instead of lengthening them.
#include "kernels_lincomb.h"
#include "kernels_kzg_cosets_fold.h"
namespace apk {
int g1_lincomb_segments_bls12381(int device, const void* points, const void* scalars, const uint64_t* seg, uint32_t nb_segments, void* out) {
    return g1_lincomb_segments_impl<FrBLS12381, FpBLS12381>(device, points, scalars, seg, nb_segments, out);
}
int g1_check_points_bls12381(int device, const void* points, uint64_t count, uint8_t* flags) {
    return g1_check_points_impl<FrBLS12381, FpBLS12381, true>(device, points, count, flags);
}
int kzg_cosets_fold_bls12381(int device, int log_l, uint32_t count, const void* values, const void* scale, const void* step, const void* tw, void* out) {
    return kzg_cosets_fold_impl<FrBLS12381>(device, log_l, count, values, scale, step, tw, out);
}
}  // namespace apk
