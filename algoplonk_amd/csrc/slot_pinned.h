// A slot's page-locked result buffer (the last kernel of a chain writes there through the buffer's device view):
//   [PIN_AFF ..)     this proof's commitments after sync_results(), affine
//   [PIN_XYZZ ..)    MSM sums as they leave the device, XYZZ: up to MSM_ARGS_MAX points - a gang's merged batch lands in its LEAD's
//   [PIN_FR ..)      evaluations / the grand product's total / an opening's values (kzg_run.h)
//   PIN_TAIL, PIN_DENSITY   the quotient's tail flag, the wires' digit count
// Nobody adds an offset to the buffer by hand: pin_host / pin_dev give a region as the type that lives there.  What each region
// must hold at most is asserted where the types are known (backend_impl.h, kzg_run.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace apk {
constexpr size_t PIN_AFF = 0, PIN_XYZZ = 1024, PIN_FR = 4096, PIN_TAIL = 6144, PIN_DENSITY = 6208, PIN_BYTES = 8192;

// the region at `off` as the host sees it
template <class T>
inline T* pin_host(void* h_pinned, size_t off) { return reinterpret_cast<T*>(static_cast<uint8_t*>(h_pinned) + off); }
template <class T>
inline const T* pin_host(const void* h_pinned, size_t off) { return reinterpret_cast<const T*>(static_cast<const uint8_t*>(h_pinned) + off); }
// ... and as the device does: null without a device view of the buffer (the caller then writes a device buffer and copies)
template <class T>
inline T* pin_dev(uint8_t* d_pinned, size_t off) { return d_pinned ? reinterpret_cast<T*>(d_pinned + off) : nullptr; }
// the device's twin of `bytes` bytes at the host pointer `h`: null without a device view, or when they do not lie inside the buffer
template <class T>
inline T* pin_dev_of(const void* h_pinned, uint8_t* d_pinned, const T* h, size_t bytes) {
    const uint8_t *base = static_cast<const uint8_t*>(h_pinned), *p = reinterpret_cast<const uint8_t*>(h);
    if (!d_pinned || p < base || p + bytes > base + PIN_BYTES) return nullptr;
    return reinterpret_cast<T*>(d_pinned + (p - base));
}
}  // namespace apk
