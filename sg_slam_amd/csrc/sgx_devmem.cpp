// sgx_devmem.cpp — the failure-injection tap of SgxDevMem (sgx_devmem.h); nothing in the product build.
#include "sgx_devmem.h"
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"
// test tap: the n-th allocation or upload copy that this thread's handles make through SgxDevMem fails (n <= 0: off).  Returns the status the previous arming delivered,
// SGX_OK if it never fired
SGX_TAP int sgx_debug_devmem_fail_after(int n)
{
    const int delivered = g_devmem_fail_status;
    g_devmem_fail_after = n > 0 ? n : 0; g_devmem_fail_status = SGX_OK;
    return delivered;
}
#endif
