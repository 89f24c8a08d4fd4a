// The one runtime setting the library depends on: GPU_MAX_HW_QUEUES, the number of hardware queues ROCm maps a process's HIP streams
// onto.  The rule for what the load-time constructor (apk_api.cpp) does to the variable, GPU-free and without state, so that it
// reads the same in the library and in a test of its own.
//
// The need: a queue per proving stream, 16.  With fewer queues than proving streams the narrow, latency-bound kernels of one proof
// (sort, scans, combine, row/column and bit sums) stand in front of other proofs' wide ones.  More is not better: 20, 24 and 32
// queues - room for the copy, side and lincomb streams too - give the same proofs/s under load as 16 and cost a LONE proof 0.4 ms
// of its 3.2 (measured on the parent build as well, with the variable set in front: it is the queue count, not this code;
// CHANGELOG "Hardware queues", profiles/hw_queues_ab.txt).
//
// The rule is RAISE-ONLY: a value at or above the need stays as the host set it; a lower, missing or unreadable one becomes the
// need.  "Unless already set" was not enough: a machine that exports the ROCm default (4) in front of every command has set it.
// APK_HW_QUEUES = 4 .. 32 sets the need; APK_HW_QUEUES = 0 leaves the environment exactly as found (a host that insists, or one
// that initialised HIP before it loaded the library and knows the variable is no longer read).  Nothing written here is below
// HWQ_MIN or above HWQ_MAX.
#pragma once
#include <stdlib.h>

namespace apk {

constexpr int HWQ_MIN = 4, HWQ_MAX = 32, HWQ_NEED = 16;
constexpr int HWQ_UNSET = -1, HWQ_UNREADABLE = -2;      // (APK_HWQ_UNSET / APK_HWQ_UNREADABLE of include/apk.h)

// the value of a queue-count string: >= 0, HWQ_UNSET for no string, HWQ_UNREADABLE for an empty one or one with any character
// that is not a decimal digit (no sign, no blanks, no suffix: " 8", "+8", "4x" are unreadable, whatever the HIP runtime's own
// parser would make of them - an unreadable value is raised to the need, so the two never disagree about what is in force)
inline int hwq_parse(const char* v) {
    if (!v) return HWQ_UNSET;
    if (!*v) return HWQ_UNREADABLE;
    long x = 0;
    for (const char* p = v; *p; p++) {
        if (*p < '0' || *p > '9') return HWQ_UNREADABLE;
        if (x <= 1000000) x = x * 10 + (*p - '0');
    }
    return x > 1000000 ? 1000000 : (int)x;
}

struct HwqPlan {
    int need;       // queues the library asks for; 0 = leave the environment as found
    int write;      // the value to put into the variable; 0 = write nothing
};

// found: hwq_parse of GPU_MAX_HW_QUEUES; knob: hwq_parse of APK_HW_QUEUES
inline HwqPlan hwq_plan(int found, int knob) {
    if (knob == 0) return {0, 0};
    int need = knob > 0 ? knob : HWQ_NEED;
    if (need < HWQ_MIN) need = HWQ_MIN;
    if (need > HWQ_MAX) need = HWQ_MAX;
    return {need, found >= need ? 0 : need};
}

// The record of the library's first call into the HIP runtime: whether the variable still held what the constructor left - a host
// that changed it in between shows in apk_runtime_read.  INVARIANT: every path on which the library can be the first to reach
// the HIP runtime passes through runtime_checkpoint() before its first HIP call.  The backends (backend_impl.h, kernels_lincomb.h)
// are reached only through exports of apk_api.cpp and verify_api.cpp, so the checkpoints sit there: in every export that takes a
// device ordinal or creates a context, in the two helpers that probe for a device (kzg_need_device, host_mem_device) and in the
// stream pool.  comm.cpp selects its device through one helper, comm_set_device(), which checkpoints.  A new export that can
// reach a device adds the call; tests/test_hw_queues_host.py walks the device-taking exports, each in a process of its own.
void runtime_checkpoint();

}  // namespace apk
