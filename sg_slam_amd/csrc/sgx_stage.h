// sgx_stage.h — per-thread, grow-only device staging slots for the host-pointer (synchronous) entry points, and the call-scoped helper that hands them out.
// A Tracking thread calls sgx_match_project_frame / sgx_match_project_local / sgx_pose_optimization once per frame; allocating their ~40 device buffers
// with hipMalloc / hipFree on every call costs milliseconds — more than the kernels.  A slot keeps its allocation from call to call and only grows, so in
// steady state a call allocates nothing.  The slots are never freed (they live as long as the thread that tracks; tearing HIP allocations down from a
// thread_local destructor at process exit races the runtime's own shutdown).
// An entry creates one SgxStaging on its stack and stages every buffer through it, in a fixed order: slot numbers are never written out.
#pragma once
#include "sgx_rt.h"
#include "../../include/sgx.h"
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test / tuning taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif
#include <stdio.h>
#include <vector>

struct SgxStage {
    struct Slot { void *p = nullptr; size_t cap = 0; };
    std::vector<Slot> slots;
    int get(int k, size_t bytes, void **out)
    {
        if ((int)slots.size() <= k) slots.resize((size_t)k + 1);
        Slot &s = slots[(size_t)k];
        if (!s.p || s.cap < bytes) {
            if (s.p) (void)hipFree(s.p);
            s.p = nullptr; s.cap = 0;
            const size_t c = bytes + bytes / 2 + 256;
            if (hipMalloc(&s.p, c) != hipSuccess) { s.p = nullptr; return SGX_ERR_NOMEM; }
            s.cap = c;
        }
        *out = s.p;
        return SGX_OK;
    }
};
inline SgxStage &sgx_stage() { static thread_local SgxStage st; return st; }

// Slot bases.  The three per-frame entries of a Tracking thread keep ranges of their own, so that none of them regrows a slot another one sized; every other
// entry is synchronous, ends with a blocking copy and shares the first range.
enum { SGX_STAGE_SHARED = 0, SGX_STAGE_FRAME_MATCH = 0, SGX_STAGE_LOCAL_MATCH = 20, SGX_STAGE_POSE_OPT = 40 };

static_assert(sizeof(sgx_keypoint) == 28, "the kernels read keypoints as 28-byte records");

// The staging of one call: hands out this thread's slots from `base` upwards, one per in() / inout() / out(), and returns the typed device pointer, so a kernel
// argument is set where its buffer is staged.  Counts are elements of T.  Uploads are asynchronous on the legacy stream (the host source must live until the
// entry's blocking read-back, or be followed by a synchronisation); back() is a blocking copy.  `rc` is sticky: after a failure every later call does nothing,
// so an entry tests it once before it launches and once after its read-backs.
struct SgxStaging {
    int next, rc = SGX_OK;
    explicit SgxStaging(int base) : next(base) {}
    // scratch or output of n elements; the contents are whatever the slot held before
    template <class T> T *out(size_t n)
    {
        void *p = nullptr;
        if (rc == SGX_OK) rc = sgx_stage().get(next, n ? n * sizeof(T) : 1, &p);
        next++;
        return (T *)p;
    }
    // n elements uploaded from src, which the kernel also writes; a NULL source with a non-zero count is an error, never a silent out()
    template <class T> T *inout(const T *src, size_t n)
    {
        T *p = out<T>(n);
        if (rc == SGX_OK && n && !src) rc = SGX_ERR_INVALID;
        if (rc == SGX_OK && n) hip(hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, 0));
        return p;
    }
    template <class T> const T *in(const T *src, size_t n) { return inout(src, n); }
    const uint8_t *keys(const sgx_keypoint *k, size_t n) { return (const uint8_t *)in(k, n); }                  // the kernels take keypoints as bytes
    const uint32_t *desc(const uint8_t *d, size_t n) { return (const uint32_t *)in(d, n * 32); }                // n 256-bit descriptors, read as 8 words each
    template <class T> void back(T *dst, const T *dev, size_t n) { if (rc == SGX_OK && n) hip(hipMemcpy(dst, dev, n * sizeof(T), hipMemcpyDeviceToHost)); }
    void hip(hipError_t e)
    {
        if (e == hipSuccess) return;
        fprintf(stderr, "sgx: HIP error %d (%s) in a staged copy\n", (int)e, hipGetErrorString(e));
        rc = SGX_ERR_DEVICE;
    }
};
