// Error returns and device buffers: shared by the runners (msm_run.h, kzg_run.h) and the backend that includes them.
#pragma once
#include <hip/hip_runtime.h>

#include "backend.h"

namespace apk {

#define HIPCHK(x)                                                                                              \
    do {                                                                                                       \
        hipError_t e_ = (x);                                                                                   \
        if (e_ != hipSuccess) {                                                                                \
            set_error("%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__);                        \
            return APK_ERR_HIP;                                                                                \
        }                                                                                                      \
    } while (0)
#define CHK(x)                 \
    do {                       \
        int r_ = (x);          \
        if (r_ != APK_OK) return r_; \
    } while (0)
#define KCHK() HIPCHK(hipGetLastError())

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    int alloc(size_t n) {
        release();
        if (n == 0) n = 16;
        HIPCHK(hipMalloc(&p, n));
        bytes = n;
        return APK_OK;
    }
};
template <class T> static inline T* ptr(const DevBuf& b) { return reinterpret_cast<T*>(b.p); }

}  // namespace apk
