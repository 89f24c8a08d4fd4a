// BN254 instantiation of the test seams (seam_run.h, include/apk.h apk_device_*_op).  A translation unit of its own: the seams
// are instantiated here and not in backend_bn254.hip, so they compile next to the backend instead of lengthening it - and without
// the prover (backend_impl.h), which they do not need.
#include "seam_run.h"
namespace apk {
int fe_op_device_bn254(int device, int field, int op, uint64_t count, const void* a, const void* b, void* out) {
    return fe_op_device_impl<FrBN254, FpBN254>(device, field, op, count, a, b, out);
}
int feu_op_device_bn254(int device, int field, int op, uint64_t count, const void* in, void* out) {
    return feu_op_device_impl<FrBN254, FpBN254>(device, field, op, count, in, out);
}
int g1_op_device_bn254(int device, int op, uint64_t count, const void* p, const void* q, void* out) {
    return g1_op_device_impl<FrBN254, FpBN254>(device, op, count, p, q, out);
}
int poly_op_device_bn254(int device, int op, const apk_poly_args* args) {
    return poly_op_device_impl<FrBN254, FpBN254>(device, op, args);
}
}  // namespace apk
