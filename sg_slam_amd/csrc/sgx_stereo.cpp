// sgx_stereo.cpp — host side of Frame::ComputeStereoMatches (src/sg-slam/src/Frame.cc:716-890) behind the C ABI: the handle owns the per-keypoint workspace;
// sgx_stereo_match_batch_dev checks its arguments against the two extractor handles (sgx_orb_view.h), enqueues the three kernels of sgx_stereo_kernels.h on the caller's
// stream and reads nothing back; sgx_stereo_match is one pair fed from host memory after two sgx_orb_extract calls.
#include "sgx_stereo_kernels.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#include <stdio.h>
#include <string.h>
#include <new>
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif

struct sgx_stereo {
    SgxOrbLevels lv;               // the geometry the workspace was sized for
    int max_batch = 0, cap = 0, last_batch = 0;
    int *best = nullptr, *code = nullptr, *sad = nullptr, *tap = nullptr;
    // the synchronous entry's staging: both key sets, both descriptor sets, the two counts, the outputs
    uint8_t *one_keys = nullptr, *one_desc = nullptr; int *one_n = nullptr; float *one_out = nullptr;
    SgxDevMem mem;
};

extern "C" int sgx_stereo_create(const sgx_orb *geometry_of, int max_batch, sgx_stereo **out)
{
    if (out) *out = nullptr;
    SgxOrbView v;
    if (!out || !geometry_of || max_batch < 1 || sgx_orb_view(geometry_of, &v) != SGX_OK) return SGX_ERR_INVALID;
    if (v.lv.kp_cap < 1 || v.lv.kp_cap > 65535) return SGX_ERR_UNSUPPORTED;          // bestIdxR travels in 16 bits beside the distance
    sgx_stereo *h = new (std::nothrow) sgx_stereo();
    if (!h) return SGX_ERR_NOMEM;
    h->lv = v.lv; h->max_batch = max_batch; h->cap = v.lv.kp_cap;
    const size_t P = (size_t)max_batch * (size_t)h->cap, c = (size_t)h->cap;
    SgxDevMem &m = h->mem;
    int rc;
    if ((rc = m.alloc(&h->best, P)) || (rc = m.alloc(&h->code, P)) || (rc = m.alloc(&h->sad, P)) ||
#ifdef SGX_DEBUG_TAPS
        (rc = m.alloc(&h->tap, P * SGX_ST_TAPS)) ||
#endif
        (rc = m.alloc(&h->one_keys, 2 * c * 28)) || (rc = m.alloc(&h->one_desc, 2 * c * 32)) || (rc = m.alloc(&h->one_n, 3)) || (rc = m.alloc(&h->one_out, 2 * c))) { delete h; return rc; }
    *out = h;
    return SGX_OK;
}

extern "C" void sgx_stereo_destroy(sgx_stereo *h) { delete h; }

// one side of the pair against the handle's geometry and the extractor's last pyramid
static bool stereo_side_ok(const sgx_stereo *h, const sgx_orb *orb, int first, int batch, const uint8_t *d_gray, int pitch, SgxOrbView *v)
{
    if (sgx_orb_view(orb, v) != SGX_OK || memcmp(&v->lv, &h->lv, sizeof h->lv) != 0) return false;
    if (first < 0 || v->pyr_batch < 1 || (long long)first + batch > (long long)v->pyr_batch) return false;      // no pyramid, or one for fewer frames
    return d_gray == v->d_gray && pitch == v->gray_pitch;                                                        // the image that pyramid was built from
}

extern "C" int sgx_stereo_match_batch_dev(sgx_stereo *h, int batch, sgx_orb *orb_left, int left_first_frame, const uint8_t *d_gray_left, int pitch_left,
                                          sgx_orb *orb_right, int right_first_frame, const uint8_t *d_gray_right, int pitch_right, int cap,
                                          const sgx_keypoint *d_keys_left, const uint8_t *d_desc_left, const int32_t *d_n_left,
                                          const sgx_keypoint *d_keys_right, const uint8_t *d_desc_right, const int32_t *d_n_right,
                                          float fx, float bf, float *d_uright, float *d_zdepth, int32_t *d_nmatched, void *stream)
{
    if (!h || !orb_left || !orb_right || !d_gray_left || !d_gray_right || !d_keys_left || !d_desc_left || !d_n_left || !d_keys_right || !d_desc_right || !d_n_right ||
        !d_uright || !d_zdepth) return SGX_ERR_INVALID;
    if (batch < 1 || batch > h->max_batch || cap != h->cap) return SGX_ERR_INVALID;      // cap below the extractors' capacity, or beyond the workspace
    SgxOrbView vl, vr;
    if (!stereo_side_ok(h, orb_left, left_first_frame, batch, d_gray_left, pitch_left, &vl) ||
        !stereo_side_ok(h, orb_right, right_first_frame, batch, d_gray_right, pitch_right, &vr)) return SGX_ERR_INVALID;
    const sgx_stream_t s = (sgx_stream_t)stream;
    SgxStereoArgs A; memset(&A, 0, sizeof A);
    A.lv = h->lv; A.cap = cap;
    A.L.gray = d_gray_left; A.L.pyr = vl.d_pyr; A.L.pitch = pitch_left; A.L.first = left_first_frame;
    A.L.keys = (const uint8_t *)d_keys_left; A.L.desc = d_desc_left; A.L.n = d_n_left;
    A.R.gray = d_gray_right; A.R.pyr = vr.d_pyr; A.R.pitch = pitch_right; A.R.first = right_first_frame;
    A.R.keys = (const uint8_t *)d_keys_right; A.R.desc = d_desc_right; A.R.n = d_n_right;
    // minZ = mb, maxD = mbf / minZ (:746-748).  The reference reads mb before the constructor assigns it (Frame.cc:99 against :123); defined here as mb = mbf / fx
    const float mb = bf / fx;
    A.bf = bf; A.maxD = bf / mb;
    A.uright = d_uright; A.zdepth = d_zdepth; A.best = h->best; A.code = h->code; A.sad = h->sad; A.tap = h->tap; A.nmatched = d_nmatched;
    h->last_batch = batch;
    const unsigned B = (unsigned)batch, C = (unsigned)cap;
    SGX_LAUNCH(k_stereo_best, dim3((C + SGX_ST_KPB - 1) / SGX_ST_KPB, B), dim3(256), s, A);
    SGX_LAUNCH(k_stereo_sad, dim3((C + 3) / 4, B), dim3(256), s, A);
    SGX_LAUNCH(k_stereo_median, dim3(B), dim3(256), s, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_stereo_match(sgx_stereo *h, sgx_orb *orb_left, sgx_orb *orb_right, const sgx_keypoint *keys_left, const uint8_t *desc_left, int n_left,
                                const sgx_keypoint *keys_right, const uint8_t *desc_right, int n_right, float fx, float bf, float *uright, float *zdepth, int *nmatched)
{
    if (!h || !orb_left || !orb_right || orb_left == orb_right || n_left < 0 || n_right < 0 || n_left > h->cap || n_right > h->cap || !uright || !zdepth) return SGX_ERR_INVALID;
    if ((n_left && (!keys_left || !desc_left)) || (n_right && (!keys_right || !desc_right))) return SGX_ERR_INVALID;
    SgxOrbView vl, vr;
    if (sgx_orb_view(orb_left, &vl) != SGX_OK || sgx_orb_view(orb_right, &vr) != SGX_OK || !vl.staged || !vr.staged) return SGX_ERR_INVALID;      // each after its own sgx_orb_extract
    const size_t c = (size_t)h->cap;
    const int32_t cnt[3] = { n_left, n_right, 0 };
    if (n_left) {
        SGX_CHECK_HIP(hipMemcpy(h->one_keys, keys_left, 28 * (size_t)n_left, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(h->one_desc, desc_left, 32 * (size_t)n_left, hipMemcpyHostToDevice));
    }
    if (n_right) {
        SGX_CHECK_HIP(hipMemcpy(h->one_keys + 28 * c, keys_right, 28 * (size_t)n_right, hipMemcpyHostToDevice));
        SGX_CHECK_HIP(hipMemcpy(h->one_desc + 32 * c, desc_right, 32 * (size_t)n_right, hipMemcpyHostToDevice));
    }
    SGX_CHECK_HIP(hipMemcpy(h->one_n, cnt, sizeof cnt, hipMemcpyHostToDevice));
    const int rc = sgx_stereo_match_batch_dev(h, 1, orb_left, 0, vl.d_gray, vl.gray_pitch, orb_right, 0, vr.d_gray, vr.gray_pitch, h->cap,
                                              (const sgx_keypoint *)h->one_keys, h->one_desc, h->one_n, (const sgx_keypoint *)(h->one_keys + 28 * c), h->one_desc + 32 * c, h->one_n + 1,
                                              fx, bf, h->one_out, h->one_out + c, h->one_n + 2, nullptr);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    if (n_left) {
        SGX_CHECK_HIP(hipMemcpy(uright, h->one_out, 4 * (size_t)n_left, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(zdepth, h->one_out + c, 4 * (size_t)n_left, hipMemcpyDeviceToHost));
    }
    if (nmatched) SGX_CHECK_HIP(hipMemcpy(nmatched, h->one_n + 2, 4, hipMemcpyDeviceToHost));
    return SGX_OK;
}

#ifdef SGX_DEBUG_TAPS
// test tap: the per-keypoint state of left frame `frame` of the handle's last batch, cap entries each (sads: cap x 11).  Synchronises the device.
SGX_TAP int sgx_stereo_debug_read(sgx_stereo *h, int frame, int32_t *best_idx, int32_t *best_dist, int32_t *exit_code, int32_t *best_inc, int32_t *sads)
{
    if (!h || frame < 0 || frame >= h->last_batch) return SGX_ERR_INVALID;
    SGX_CHECK_HIP(hipDeviceSynchronize());
    const size_t c = (size_t)h->cap, o = (size_t)frame * c;
    std::vector<int> b(c), t(c * SGX_ST_TAPS);
    SGX_CHECK_HIP(hipMemcpy(b.data(), h->best + o, 4 * c, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(t.data(), h->tap + o * SGX_ST_TAPS, 4 * c * SGX_ST_TAPS, hipMemcpyDeviceToHost));
    if (exit_code) SGX_CHECK_HIP(hipMemcpy(exit_code, h->code + o, 4 * c, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < c; i++) {
        if (best_idx) best_idx[i] = b[i] & 0xFFFF;
        if (best_dist) best_dist[i] = b[i] >> 16;
        if (best_inc) best_inc[i] = t[i * SGX_ST_TAPS];
        if (sads) for (int j = 0; j < 11; j++) sads[i * 11 + j] = t[i * SGX_ST_TAPS + 1 + j];
    }
    return SGX_OK;
}
#endif
