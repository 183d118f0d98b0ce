// orb_plan_probe.cpp — stand-alone host program: creates and destroys an ORB extractor handle for every geometry of tests/test_orb_plan.py, the refused ones included,
// and checks the statuses and that *out is NULL on refusal.  tests/test_orb_plan_probe.py builds this file and the emulator units with AddressSanitizer / UBSan; in the
// emulator hipMalloc is calloc, so LeakSanitizer sees a handle or a buffer that a refused geometry leaves behind, and ASan a planner that writes outside its tables.
#include "../../include/sgx.h"
#include <stdio.h>

struct Case { int w, h, nlevels, nfeatures; float sf; int status; };
static const Case CASES[] = {
    {640, 480, 8, 1000, 1.2f, SGX_OK}, {1241, 376, 8, 2000, 1.2f, SGX_OK}, {322, 242, 8, 1000, 1.2f, SGX_OK}, {298, 226, 8, 1000, 1.2f, SGX_OK},
    {200, 136, 1, 1000, 1.2f, SGX_OK}, {64, 64, 1, 100, 1.2f, SGX_OK}, {640, 480, 3, 1000, 1.5f, SGX_OK}, {1280, 960, 2, 1000, 2.5f, SGX_OK},
    {752, 480, 8, 1200, 1.2f, SGX_OK},
    {203, 151, 8, 1000, 1.2f, SGX_ERR_UNSUPPORTED}, {100, 300, 1, 500, 1.2f, SGX_ERR_UNSUPPORTED}, {640, 480, 2, 3000, 1.2f, SGX_ERR_UNSUPPORTED},
    {4000, 100, 2, 500, 1.2f, SGX_ERR_UNSUPPORTED}, {640, 480, 4, 1000, 2.0f, SGX_ERR_UNSUPPORTED},
};

int main()
{
    int bad = 0;
    for (const Case &c : CASES) {
        sgx_orb_config cfg;
        cfg.nfeatures = c.nfeatures; cfg.scale_factor = c.sf; cfg.nlevels = c.nlevels; cfg.ini_th_fast = 20; cfg.min_th_fast = 7;
        cfg.width = c.w; cfg.height = c.h; cfg.max_batch = 2;
        sgx_orb *h = (sgx_orb *)&cfg;          // anything but NULL: a failed create must clear it
        const int rc = sgx_orb_create(&cfg, &h);
        if (rc != c.status || (rc == SGX_OK) != (h != NULL)) {
            fprintf(stderr, "%dx%d levels %d features %d scale %g: status %d (expected %d), handle %s\n", c.w, c.h, c.nlevels, c.nfeatures, c.sf, rc, c.status, h ? "set" : "NULL");
            bad++;
        }
        if (rc == SGX_OK) {
            if (sgx_orb_keypoint_capacity(h) < 1) { fprintf(stderr, "%dx%d: no keypoint capacity\n", c.w, c.h); bad++; }
            sgx_orb_destroy(h);
        }
    }
    {   // an invalid configuration is refused before anything is planned, and clears *out as well
        sgx_orb_config cfg = {1000, 1.2f, 0, 20, 7, 640, 480, 1};
        sgx_orb *h = (sgx_orb *)&cfg;
        if (sgx_orb_create(&cfg, &h) != SGX_ERR_INVALID || h) { fprintf(stderr, "nlevels 0: not refused as invalid with a NULL handle\n"); bad++; }
    }
    if (!bad) printf("orb_plan_probe: %d geometries ok\n", (int)(sizeof CASES / sizeof CASES[0]));
    return bad ? 1 : 0;
}
