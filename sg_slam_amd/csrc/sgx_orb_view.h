// sgx_orb_view.h — what another unit of the library may know of an ORB extractor handle (host only, not part of the C ABI): the level geometry and scale tables that
// creation decided, and the image pyramid of the handle's last extraction.  sgx_stereo.cpp reads both pyramids of a stereo pair through it (Frame::ComputeStereoMatches reads
// mpORBextractorLeft/Right->mvImagePyramid).  Filled by sgx_orb_view() in sgx_orb.cpp, the only unit that sees the handle itself.
#pragma once
#include <stdint.h>

#define SGX_VIEW_LEVELS 12      /* == SGX_MAX_LEVELS (checked in sgx_orb.cpp) */

// plain data, zero-filled before it is written: two handles have the same geometry iff their SgxOrbLevels compare equal bytewise
struct SgxOrbLevels {
    int nlevels, W, H, kp_cap, pyr_pitch;          // pyr_pitch: bytes per frame of pyramid storage (levels 1..)
    int w[SGX_VIEW_LEVELS], h[SGX_VIEW_LEVELS], stride[SGX_VIEW_LEVELS], off[SGX_VIEW_LEVELS];      // off: byte offset of a level inside one frame's pyramid storage
    float scale[SGX_VIEW_LEVELS], inv_scale[SGX_VIEW_LEVELS];      // mvScaleFactor, mvInvScaleFactor
};

struct SgxOrbView {
    SgxOrbLevels lv;
    const uint8_t *d_pyr;       // levels 1.. of every frame of the last extraction
    const uint8_t *d_gray;      // level 0 of that extraction: the caller's image, or the handle's staging copy after sgx_orb_extract
    int gray_pitch;
    int pyr_batch;              // frames of the last extraction whose pyramid is in d_pyr (0: none)
    int staged;                 // 1: the last extraction was sgx_orb_extract (d_gray is the handle's own copy of the host image)
};

struct sgx_orb;
int sgx_orb_view(const sgx_orb *h, SgxOrbView *v);
