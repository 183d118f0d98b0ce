// sgx_devmem.h — the device allocations of one handle (host only).  A handle has an SgxDevMem member and takes every device buffer from it: alloc / upload record the
// allocation, the destructor frees what is recorded, so a create function has one failure exit (`delete h`) and a buffer cannot be added to a handle without an owner.
// Compiles in the device, tap, nofma and emulator builds alike (the emulator's hipMalloc is calloc).
#pragma once
#include "sgx_rt.h"
#include "../../include/sgx.h"
#include <vector>

// test tap sgx_debug_devmem_fail_after (include/sgx_debug.h, sgx_devmem.cpp): one counter per thread, consulted by alloc and by the copy of upload; the n-th consultation
// fails with the status the runtime's refusal would have given.  Folds to nothing in the product build, as sgx_getenv() does.
#ifdef SGX_DEBUG_TAPS
inline thread_local int g_devmem_fail_after = 0, g_devmem_fail_status = SGX_OK;
static inline bool sgx_devmem_fail(int status) { if (g_devmem_fail_after <= 0 || --g_devmem_fail_after > 0) return false; g_devmem_fail_status = status; return true; }
#else
static inline bool sgx_devmem_fail(int) { return false; }
#endif

struct SgxDevMem {
    std::vector<void *> owned;
    SgxDevMem() = default;
    SgxDevMem(const SgxDevMem &) = delete;
    SgxDevMem &operator=(const SgxDevMem &) = delete;
    ~SgxDevMem() { for (void *q : owned) (void)hipFree(q); }

    // max(n, 1) elements; *p is written on success only
    template <class T> int alloc(T **p, size_t n)
    {
        owned.push_back(nullptr);                                // the record first: a vector that cannot grow throws before there is anything to lose
        if (sgx_devmem_fail(SGX_ERR_NOMEM) || hipMalloc(&owned.back(), (n ? n : 1) * sizeof(T)) != hipSuccess) { owned.pop_back(); return SGX_ERR_NOMEM; }
        *p = (T *)owned.back();
        return SGX_OK;
    }
    // a host array as a device allocation (blocking copy); the destination may be a pointer to const
    template <class T> int upload(T **p, const T *src, size_t n)
    {
        const int rc = alloc(p, n);
        if (rc != SGX_OK) return rc;
        return n && (sgx_devmem_fail(SGX_ERR_DEVICE) || hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) ? SGX_ERR_DEVICE : SGX_OK;
    }
    template <class T> int upload(const T **p, const T *src, size_t n) { T *d = nullptr; const int rc = upload(&d, src, n); *p = d; return rc; }
    template <class P, class T> int upload(P **p, const std::vector<T> &v) { return upload(p, v.data(), v.size()); }
    // frees one recorded allocation and forgets it (nullptr: nothing to do)
    void release(void *q)
    {
        for (size_t i = 0; q && i < owned.size(); i++) if (owned[i] == q) { (void)hipFree(q); owned.erase(owned.begin() + (long)i); return; }
    }
};
