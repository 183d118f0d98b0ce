/* sgx.h — C ABI of the MI355X-native SG-SLAM tracking hot path (libsgx.so).
 *
 * The reference (silencht/SG-SLAM) has no FFI layer: its Tracking / LocalMapping threads call
 * C++ classes directly.  Each entry point below replaces one of those call sites; the C++
 * adapters in sg_slam_amd/host/ keep the reference class signatures and forward here.
 * All functions return SGX_OK (0) or a negative sgx_status; no C++ types cross this line.
 * Pointers named d_* are DEVICE pointers (HBM); all others are host pointers.
 * `stream` is a hipStream_t passed as void* (NULL = default stream).
 */
#ifndef SGX_H
#define SGX_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum sgx_status {
    SGX_OK = 0,
    SGX_ERR_INVALID = -1,      /* bad argument */
    SGX_ERR_UNSUPPORTED = -2,  /* geometry outside compiled limits */
    SGX_ERR_NOMEM = -3,
    SGX_ERR_DEVICE = -4,       /* HIP runtime error */
    SGX_ERR_OVERFLOW = -5      /* a fixed-capacity device buffer overflowed (result not valid) */
} sgx_status;

const char *sgx_version(void);
const char *sgx_status_string(int status);

/* cv::KeyPoint (OpenCV 3.4 layout, 28 bytes) as produced by ORBextractor::operator()
 * (reference: src/sg-slam/src/ORBextractor.cc:838-848, :1096-1104). */
typedef struct sgx_keypoint {
    float x, y;      /* pt, already multiplied by the level scale for octave > 0 */
    float size;      /* (int)(31 * scale[octave]) */
    float angle;     /* degrees in [0,360), cv::fastAtan2 of the intensity centroid */
    float response;  /* FAST score */
    int32_t octave;
    int32_t class_id; /* -1 */
} sgx_keypoint;

/* ---- ORB extractor ------------------------------------------------------------------------
 * Replaces ORB_SLAM2::ORBextractor (src/sg-slam/include/ORBextractor.h:45-111):
 *   ctor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)   -> sgx_orb_create
 *   operator()(image, mask [ignored], keypoints, descriptors)   -> sgx_orb_extract[_batch_dev]
 *   GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 *   GetInverseScaleSigmaSquares / GetLevels / GetnFeatures         -> sgx_orb_get_tables
 * The image size is fixed per handle (the reference re-derives level sizes per call,
 * ORBextractor.cc:1112-1113; a Tracking instance only ever feeds one size). */
typedef struct sgx_orb_config {
    int32_t nfeatures;      /* ORBextractor.nFeatures  (TUM3.yaml: 1000) */
    float scale_factor;     /* ORBextractor.scaleFactor (1.2) */
    int32_t nlevels;        /* ORBextractor.nLevels (8) */
    int32_t ini_th_fast;    /* ORBextractor.iniThFAST (20) */
    int32_t min_th_fast;    /* ORBextractor.minThFAST (7) */
    int32_t width, height;  /* gray image size (640x480) */
    int32_t max_batch;      /* frames per batched call (device workspace is sized for this) */
} sgx_orb_config;

typedef struct sgx_orb sgx_orb;

int sgx_orb_create(const sgx_orb_config *cfg, sgx_orb **out);
void sgx_orb_destroy(sgx_orb *h);
/* keypoint capacity per frame that callers must provide (sum of per-level quotas + slack;
 * the octree may return up to 3 more than a level's quota, ORBextractor.cc:670-735). */
int sgx_orb_keypoint_capacity(const sgx_orb *h);
/* each array has nlevels entries; any pointer may be NULL */
int sgx_orb_get_tables(const sgx_orb *h, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2,
                       int32_t *features_per_level);
/* Batched, device-resident.  d_gray: batch frames, each height rows of `pitch` bytes; d_gray and pitch must be multiples of 4
 * (the kernels stage aligned dwords; any image WIDTH is fine — sgx_orb_extract pads its staging copy itself), else SGX_ERR_INVALID.
 * d_kps: batch*cap keypoints, d_desc: batch*cap*32 bytes, d_count: batch int32.
 * Asynchronous on `stream`.  cap must be >= sgx_orb_keypoint_capacity(). */
int sgx_orb_extract_batch_dev(sgx_orb *h, const uint8_t *d_gray, int pitch, int batch,
                              sgx_keypoint *d_kps, uint8_t *d_desc, int32_t *d_count, int cap, void *stream);
/* The same extraction in two calls, for a caller that erases keypoints in between (Frame::RmDynamicPointWithSemanticAndGeometry needs positions only): orientation and
 * descriptors are then computed for the survivors alone.  detect -> [anything that reads positions] -> sgx_frame_compact_keys_src_batch_dev -> describe gives, keypoint for
 * keypoint and byte for byte, what sgx_orb_extract_batch_dev -> sgx_frame_compact_keys_batch_dev gives.
 *   sgx_orb_detect_batch_dev: pyramid, FAST, octree.  d_kps / d_count as above, every field final except `angle`, which holds -1 (cv::KeyPoint's "not applicable") until
 *     the describe call.  Raises the overflow status under the same condition as the one-shot call.  The pyramid and the selection lists stay in the handle.
 *   sgx_orb_describe_batch_dev: same d_gray / pitch / batch as the detect call it follows on the same stream (SGX_ERR_INVALID without one; any other extraction on the
 *     handle in between invalidates it).  d_n_kept[f] keypoints of frame f survive; d_src[f * cap + j] is the index that compacted keypoint j had in the detect call's
 *     output, ascending.  Writes the angle of d_kps[f * cap + j] and descriptor row d_desc[(f * cap + j) * 32 ..] for j < d_n_kept[f], nothing else. */
int sgx_orb_detect_batch_dev(sgx_orb *h, const uint8_t *d_gray, int pitch, int batch, sgx_keypoint *d_kps, int32_t *d_count, int cap, void *stream);
int sgx_orb_describe_batch_dev(sgx_orb *h, const uint8_t *d_gray, int pitch, int batch, const int32_t *d_src, const int32_t *d_n_kept,
                               sgx_keypoint *d_kps, uint8_t *d_desc, int cap, void *stream);
/* Single host frame == ORBextractor::operator() (ORBextractor.cc:1045-1106).  Synchronous. */
int sgx_orb_extract(sgx_orb *h, const uint8_t *gray, int stride, sgx_keypoint *kps, uint8_t *desc, int cap, int *n);
/* device-side overflow/status word of the last batched call (synchronises `stream`) */
int sgx_orb_last_status(sgx_orb *h, void *stream);

/* ---- ORB matcher ----------------------------------------------------------------------------
 * Replaces ORB_SLAM2::ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame,
 * const float th, const bool bMono)  (src/sg-slam/include/ORBmatcher.h:56, src/sg-slam/src/ORBmatcher.cc:1332-1472),
 * the motion-model tracker's matcher (Tracking.cc:924-931), including Frame::GetFeaturesInArea's
 * 64x48-grid candidate semantics (Frame.cc:354-419), the greedy "observed map point keeps its
 * keypoint" rule (:1407-1409) and the rotation-histogram filter (:1436-1469).
 * Frames are passed flattened: per keypoint arrays with a common per-frame
 * pitch `cap`.  l_* arrays describe LastFrame.mvpMapPoints[i]: has_mp (non-NULL), outlier
 * (mvbOutlier), xw (GetWorldPos, 3 floats), obs (Observations()), mpdesc (GetDescriptor(), 32 B).
 * cur_match[k] (out) = index i of the last-frame map point assigned to current keypoint k, or -1;
 * the current frame starts with no map points, as at Tracking.cc:919. */
typedef struct sgx_camera {
    float fx, fy, cx, cy, bf;                  /* Frame::fx.. and mbf */
    float min_x, max_x, min_y, max_y;          /* Frame::mnMinX.. (0,cols,0,rows for zero distortion, Frame.cc:707-713) */
} sgx_camera;

int sgx_match_project_frame_batch_dev(
    int batch, int cap,
    const sgx_keypoint *d_ckeys, const uint8_t *d_cdesc, const float *d_curight, const int32_t *d_cn, const float *d_cTcw,
    const sgx_keypoint *d_lkeys, const int32_t *d_ln, const uint8_t *d_l_has_mp, const uint8_t *d_l_outlier, const float *d_l_xw,
    const int32_t *d_l_obs, const uint8_t *d_l_mpdesc, const float *d_lTcw,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float th, int b_mono, int check_orientation,
    int32_t *d_cur_match, int32_t *d_nmatches, void *stream);
/* host pointers, one frame pair, synchronous */
int sgx_match_project_frame(
    int nc, const sgx_keypoint *ckeys, const uint8_t *cdesc, const float *curight, const float *cTcw,
    int nl, const sgx_keypoint *lkeys, const uint8_t *l_has_mp, const uint8_t *l_outlier, const float *l_xw,
    const int32_t *l_obs, const uint8_t *l_mpdesc, const float *lTcw,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float th, int b_mono, int check_orientation,
    int32_t *cur_match, int32_t *nmatches);

/* Tracking::SearchLocalPoints' inner work (src/sg-slam/src/Tracking.cc:1284-1311): Frame::isInFrustum(pMP, viewing_cos_limit = 0.5)
 * (Frame.cc:296-352, MapPoint::PredictScale MapPoint.cc:402-417) for every local map point, then
 * ORBmatcher(nnratio = 0.8).SearchByProjection(Frame &F, const std::vector<MapPoint*> &vpMapPoints, th) (ORBmatcher.cc:45-129).
 * Local map point i: m_xw (GetWorldPos), m_normal (GetNormal), m_min_dist / m_max_dist (mfMinDistance / mfMaxDistance), m_desc,
 * m_obs (Observations()), m_skip (isBad() or mnLastFrameSeen == current frame, Tracking.cc:1288-1291); per-frame pitch mcap (<= 4096).
 * cur_mp_obs[k] = Observations() of the map point keypoint k already holds (-1 = none; NULL = no keypoint holds one).
 * Out: cur_match[k] = local map point newly assigned to keypoint k or -1, nmatches, in_view[i] = mbTrackInView (for IncreaseVisible).
 * The batched entry writes -1 to the rows [d_cn[f], cap) of d_cur_match; the rows [d_mn[f], mcap) of d_in_view are not written and nothing is promised about them. */
int sgx_match_project_local_batch_dev(
    int batch, int cap, const sgx_keypoint *d_ckeys, const uint8_t *d_cdesc, const float *d_curight, const int32_t *d_cn, const float *d_cTcw, const int32_t *d_cur_mp_obs,
    int mcap, const int32_t *d_mn, const float *d_m_xw, const float *d_m_normal, const float *d_m_min_dist, const float *d_m_max_dist, const uint8_t *d_m_desc,
    const int32_t *d_m_obs, const uint8_t *d_m_skip,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float th, float nnratio, float viewing_cos_limit,
    int32_t *d_cur_match, int32_t *d_nmatches, uint8_t *d_in_view, void *stream);

/* host pointers, one frame, synchronous (cur_mp_obs and in_view may be NULL) */
int sgx_match_project_local(
    int nc, const sgx_keypoint *ckeys, const uint8_t *cdesc, const float *curight, const float *cTcw, const int32_t *cur_mp_obs,
    int nm, const float *m_xw, const float *m_normal, const float *m_min_dist, const float *m_max_dist, const uint8_t *m_desc, const int32_t *m_obs, const uint8_t *m_skip,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float th, float nnratio, float viewing_cos_limit,
    int32_t *cur_match, int32_t *nmatches, uint8_t *in_view);

/* ---- ORBmatcher gates of the LocalMapping thread (tier N2) --------------------------------------------------------------------
 * static int ORBmatcher::DescriptorDistance(const cv::Mat &a, const cv::Mat &b) (src/sg-slam/include/ORBmatcher.h:45, ORBmatcher.cc:1649-1665) for every pair of two
 * descriptor sets (rows of 32 bytes): out[i * nb + j]. */
int sgx_hamming_matrix(const uint8_t *desc_a, int na, const uint8_t *desc_b, int nb, uint16_t *out);
int sgx_hamming_matrix_dev(const uint8_t *d_desc_a, int na, const uint8_t *d_desc_b, int nb, uint16_t *d_out, void *stream);
/* int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs, const bool bOnlyStereo)
 * (src/sg-slam/include/ORBmatcher.h:72-73, src/sg-slam/src/ORBmatcher.cc:659-827; caller LocalMapping::CreateNewMapPoints, LocalMapping.cc:268).  Flattened keyframes:
 * keys*_un = mvKeysUn, desc* = mDescriptors, uright* = mvuRight, has_mp*[i] = GetMapPoint(i) != NULL, feat_node*[i] = the key under which keypoint i sits in mFeatVec
 * (DBoW2 FeatureVector: vocabulary node 4 levels up; -1 = not in the map), cam_center1 = pKF1->GetCameraCenter() (3 floats), Tcw2 = pKF2->GetPose() (4x4 row-major),
 * F12 = 3x3 row-major float, cam2 / scale_factors2 / level_sigma2_2 = pKF2's fx.., mvScaleFactors, mvLevelSigma2.  pairs (out, capacity n1 pairs) = vMatchedPairs as
 * (idx1, idx2) in ascending idx1; *npairs = return value.  Host pointers, synchronous. */
int sgx_match_search_for_triangulation(
    int n1, const sgx_keypoint *keys1_un, const uint8_t *desc1, const float *uright1, const uint8_t *has_mp1, const int32_t *feat_node1, const float *cam_center1,
    int n2, const sgx_keypoint *keys2_un, const uint8_t *desc2, const float *uright2, const uint8_t *has_mp2, const int32_t *feat_node2, const float *Tcw2,
    const float *F12, const sgx_camera *cam2, const float *scale_factors2, const float *level_sigma2_2, int nlevels, int only_stereo, int check_orientation,
    int32_t *pairs, int32_t *npairs);
/* int ORBmatcher::SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches) (src/sg-slam/include/ORBmatcher.h:65, src/sg-slam/src/ORBmatcher.cc:159-290;
 * callers Tracking::TrackReferenceKeyFrame Tracking.cc:806, Relocalization :1496): kf_good_mp[i] = the keyframe's keypoint i holds a map point that is not bad,
 * feat_node_* = mFeatVec keys per keypoint (the vocabulary transform itself — DBoW2 + ORBvoc — stays with the caller).  match_f[j] = index of the keyframe keypoint whose
 * map point the frame's keypoint j receives (vpMapPointMatches[j] = vpMapPointsKF[match_f[j]]), -1 = NULL; *nmatches = return value.  Host pointers, synchronous. */
int sgx_match_search_by_bow(
    int nk, const sgx_keypoint *keys_kf_un, const uint8_t *desc_kf, const uint8_t *kf_good_mp, const int32_t *feat_node_kf,
    int nf, const sgx_keypoint *keys_f_un, const uint8_t *desc_f, const int32_t *feat_node_f, float nnratio, int check_orientation,
    int32_t *match_f, int32_t *nmatches);
/* int ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12) (src/sg-slam/include/ORBmatcher.h:66, src/sg-slam/src/ORBmatcher.cc:524-655;
 * caller LoopClosing::ComputeSim3, LoopClosing.cc:265): good*[i] = keypoint i of that keyframe holds a map point that is not bad; match12[i1] (out, n1 entries) = keypoint of
 * pKF2 whose map point is vpMatches12[i1], -1 = NULL; *nmatches = return value.  Differs from the KeyFrame-Frame overload in the strict `< TH_LOW` gate (:597) and in requiring a
 * map point on both sides (:581-587).  Host pointers, synchronous. */
int sgx_match_search_by_bow_kf(
    int n1, const sgx_keypoint *keys1_un, const uint8_t *desc1, const uint8_t *good1, const int32_t *feat_node1,
    int n2, const sgx_keypoint *keys2_un, const uint8_t *desc2, const uint8_t *good2, const int32_t *feat_node2, float nnratio, int check_orientation,
    int32_t *match12, int32_t *nmatches);
/* The search of int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th = 3.0) (src/sg-slam/include/ORBmatcher.h:80,
 * src/sg-slam/src/ORBmatcher.cc:829-979; caller LocalMapping::SearchInNeighbors, LocalMapping.cc:489,514): for every candidate map point i (m_skip[i] = NULL / isBad() /
 * IsInKeyFrame(pKF); m_min_dist / m_max_dist = mfMinDistance / mfMaxDistance) the keyframe keypoint best_idx[i] it fuses with (-1: none within TH_LOW) and the Hamming
 * distance best_dist[i].  *nfused = return value (number of best_idx >= 0).  The map mutations that follow in the reference (Replace / AddObservation / AddMapPoint,
 * :950-969) are applied by the caller in index order: they do not influence the search.  Host pointers, synchronous. */
int sgx_match_fuse_search(
    int nk, const sgx_keypoint *keys_un, const uint8_t *desc, const float *uright, const float *Tcw,
    int nm, const float *m_xw, const float *m_normal, const float *m_min_dist, const float *m_max_dist, const uint8_t *m_desc, const uint8_t *m_skip,
    const sgx_camera *cam, const float *scale_factors, const float *inv_level_sigma2, int nlevels, float log_scale_factor, float th,
    int32_t *best_idx, int32_t *best_dist, int32_t *nfused);

/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, const float th, const int ORBdist)
 * (src/sg-slam/include/ORBmatcher.h:56, src/sg-slam/src/ORBmatcher.cc:1474-1601; caller Tracking::Relocalization, Tracking.cc:1571,1584): projection of the keyframe's map
 * points into the frame.  kf_ok[i] = vpMPs[i] && !isBad() && !sAlreadyFound.count(vpMPs[i]); c_has_mp[k] = CurrentFrame.mvpMapPoints[k] != NULL on entry (such keypoints are
 * never taken); m_min_dist / m_max_dist = mfMinDistance / mfMaxDistance.  cur_match[k] (out) = index i of the keyframe map point keypoint k receives
 * (CurrentFrame.mvpMapPoints[k] = vpMPs[i]), -1 = left alone; *nmatches = return value.  Host pointers, synchronous. */
int sgx_match_project_keyframe(
    int nc, const sgx_keypoint *ckeys_un, const uint8_t *cdesc, const uint8_t *c_has_mp, const float *cTcw,
    int nk, const sgx_keypoint *kf_keys_un, const uint8_t *kf_ok, const float *m_xw, const float *m_min_dist, const float *m_max_dist, const uint8_t *m_desc,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float th, int orb_dist, int check_orientation,
    int32_t *cur_match, int32_t *nmatches);

/* ---- ORBmatcher gates of the LoopClosing thread that project map points through a similarity (tier N2) ----------------------------------------------------------
 * Shared conventions: keys_un / desc = the target keyframe's mvKeysUn / mDescriptors; Scw = 4x4 row-major float (sRcw | tcw), decomposed as the reference does
 * (:301-306, :990-995); m_xw / m_normal / m_min_dist / m_max_dist / m_desc = GetWorldPos, GetNormal, mfMinDistance, mfMaxDistance, GetDescriptor of every candidate;
 * cam supplies fx, fy, cx, cy and the image bounds (KeyFrame::IsInImage), scale_factors = mvScaleFactors, log_scale_factor = mfLogScaleFactor.  Host pointers, synchronous.
 *
 * The search of int ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, float th, vector<MapPoint*> &vpReplacePoint)
 * (src/sg-slam/include/ORBmatcher.h:83, src/sg-slam/src/ORBmatcher.cc:981-1101; caller LoopClosing::SearchAndFuse, LoopClosing.cc:599): m_skip[i] = isBad() ||
 * pKF->GetMapPoints().count(pMP).  best_idx[i] = keyframe keypoint candidate i lands on (-1: none within TH_LOW), best_dist[i] its Hamming distance (256: none); the caller
 * reads pKF->GetMapPoint(best_idx[i]) to fill vpReplacePoint[i] or to add the observation (:1084-1097).  *nfused = return value. */
int sgx_match_fuse_search_sim3(
    int nk, const sgx_keypoint *keys_un, const uint8_t *desc, const float *Scw,
    int nm, const float *m_xw, const float *m_normal, const float *m_min_dist, const float *m_max_dist, const uint8_t *m_desc, const uint8_t *m_skip,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float th,
    int32_t *best_idx, int32_t *best_dist, int32_t *nfused);
/* int ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th)
 * (src/sg-slam/include/ORBmatcher.h:60, src/sg-slam/src/ORBmatcher.cc:292-407; caller LoopClosing::ComputeSim3, LoopClosing.cc:375): matched_in[k] = vpMatched[k] != NULL on
 * entry, m_skip[i] = isBad() || the point is already in vpMatched.  matched_out[k] = index i of the candidate this call stores in vpMatched[k], -1 = unchanged; the
 * reference's in-order greedy assignment (a point skips keypoints filled by earlier points, :381) is reproduced exactly.  *nmatches = return value. */
int sgx_match_project_sim3(
    int nk, const sgx_keypoint *keys_un, const uint8_t *desc, const uint8_t *matched_in, const float *Scw,
    int nm, const float *m_xw, const float *m_normal, const float *m_min_dist, const float *m_max_dist, const uint8_t *m_desc, const uint8_t *m_skip,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, int th,
    int32_t *matched_out, int32_t *nmatches);
/* int ORBmatcher::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12, const cv::Mat &t12, const float th)
 * (src/sg-slam/include/ORBmatcher.h:77, src/sg-slam/src/ORBmatcher.cc:1106-1330; caller LoopClosing::ComputeSim3, LoopClosing.cc:323).  Per keyframe, indexed by keypoint:
 * Tcw = GetPose() (4x4 row-major), mp_ok[i] = GetMapPointMatches()[i] is neither NULL nor bad, m_* = that map point's fields.  R12 = 3x3 row-major, t12 = 3 floats.
 * match12 (in/out, n1 entries): -1 = vpMatches12[i1] is NULL; >= 0 = the keypoint of pKF2 its map point sits on (GetIndexInKeyFrame(pKF2)); -2 = non-NULL but not observed by
 * pKF2.  Pairs that agree in both directions are written as keypoint indices of pKF2 (vpMatches12[i1] = vpMapPoints2[match12[i1]]); *nfound = return value.  Both keyframes
 * share cam / scale_factors (one sensor, one ORB pyramid). */
int sgx_match_search_by_sim3(
    int n1, const sgx_keypoint *keys1_un, const uint8_t *desc1, const float *Tcw1, const uint8_t *mp_ok1, const float *m_xw1, const float *m_min_dist1, const float *m_max_dist1, const uint8_t *m_desc1,
    int n2, const sgx_keypoint *keys2_un, const uint8_t *desc2, const float *Tcw2, const uint8_t *mp_ok2, const float *m_xw2, const float *m_min_dist2, const float *m_max_dist2, const uint8_t *m_desc2,
    const sgx_camera *cam, const float *scale_factors, int nlevels, float log_scale_factor, float s12, const float *R12, const float *t12, float th,
    int32_t *match12, int32_t *nfound);

/* int ORBmatcher::SearchForInitialization(Frame &F1, Frame &F2, vector<cv::Point2f> &vbPrevMatched, vector<int> &vnMatches12, int windowSize = 10)
 * (src/sg-slam/include/ORBmatcher.h:69, src/sg-slam/src/ORBmatcher.cc:407-522; caller Tracking::MonocularInitialization, Tracking.cc:639, windowSize 100): the monocular
 * initialiser's matcher (the RGB-D system never reaches it; built so that every ORBmatcher method has a device form).  prev_matched (in/out, n1 x 2 floats) = vbPrevMatched,
 * matches12 (out, n1) = vnMatches12; cam supplies the image bounds of F2's grid.  The reference's order-dependent stealing rule (a later keypoint takes a match only with a
 * strictly smaller distance) is reproduced exactly.  Host pointers, synchronous. */
int sgx_match_search_for_initialization(
    int n1, const sgx_keypoint *keys1_un, const uint8_t *desc1, int n2, const sgx_keypoint *keys2_un, const uint8_t *desc2,
    float *prev_matched, int window_size, float nnratio, int check_orientation, const sgx_camera *cam, int32_t *matches12, int32_t *nmatches);

/* The per-pair body of void LocalMapping::CreateNewMapPoints() (src/sg-slam/src/LocalMapping.cc:283-421) for the pairs sgx_match_search_for_triangulation returned for
 * (mpCurrentKeyFrame, pKF2): parallax test (:300-317), linear triangulation by cv::SVD::compute on the 4 x 4 system (:320-338) or the stereo unprojection of the side with
 * the larger parallax (:340-349), positive depth in both keyframes (:353-360), the chi-square reprojection gates (:362-406: 5.991 mono, 7.8 stereo, times mvLevelSigma2) and
 * the scale-consistency gate (:408-423).  keys*_un = mvKeysUn, keys* = mvKeys (KeyFrame::UnprojectStereo reads those, KeyFrame.cc:621-622; the same array when the camera
 * has no distortion), uright* = mvuRight, depth* = mvDepth, Tcw* = GetPose() (4x4 row-major); cam: fx, fy, cx, cy, bf.  ok[q] = 1 and x3d[q] = the new map point of pair q;
 * the map mutations (:425-442: new MapPoint, AddObservation, ComputeDistinctiveDescriptors, UpdateNormalAndDepth ...) stay with the caller.  *nnew = number of ok pairs.
 * Divergence: where the reference would dereference the empty Mat of UnprojectStereo (depth <= 0 on the chosen stereo side) the pair is rejected. */
int sgx_triangulate_new_map_points(
    int npairs, const int32_t *pairs,
    int n1, const sgx_keypoint *keys1_un, const sgx_keypoint *keys1, const float *uright1, const float *depth1, const float *Tcw1,
    int n2, const sgx_keypoint *keys2_un, const sgx_keypoint *keys2, const float *uright2, const float *depth2, const float *Tcw2,
    const sgx_camera *cam, const float *scale_factors, const float *level_sigma2, int nlevels, uint8_t *ok, float *x3d, int32_t *nnew);

/* ---- MapPoint post-steps of the optimisers and of map-point creation, batched over points (host pointers, synchronous) -----------------------------------------------
 * Observations of point p = entries obs_start[p] .. obs_start[p + 1] - 1, IN THE ORDER THE REFERENCE WALKS mObservations (a std::map keyed by KeyFrame*: the float sums
 * below depend on it; the caller flattens in that order).
 * void MapPoint::UpdateNormalAndDepth() (src/sg-slam/src/MapPoint.cc:330-371; callers Optimizer.cc:227,776,1042 — the last statement of BundleAdjustment / LocalBundleAdjustment /
 * OptimizeEssentialGraph per point — LocalMapping.cc:152,444,527, Tracking.cc:572,708,1234): obs_center = GetCameraCenter() of every observing keyframe, ref_center /
 * ref_level = mpRefKF's camera centre and the octave of the point's keypoint in it.  normal / min_dist / max_dist (in/out) = mNormalVector, mfMinDistance, mfMaxDistance;
 * a point without observations keeps its values (:345-346). */
int sgx_mappoint_update_normal_and_depth(int n, const float *xw, const int32_t *obs_start, const float *obs_center, const float *ref_center, const int32_t *ref_level,
                                         const float *scale_factors, int nlevels, float *normal, float *min_dist, float *max_dist);
/* void MapPoint::ComputeDistinctiveDescriptors() (MapPoint.cc:242-307): obs_desc = the observed descriptor rows (keyframes that are not bad).  best[p] = index within the
 * point's list of the descriptor with the least median Hamming distance to the others (first on ties), -1 for an empty list; desc_out (optional, n x 32) = that row. */
int sgx_mappoint_distinctive_descriptors(int n, const int32_t *obs_start, const uint8_t *obs_desc, int32_t *best, uint8_t *desc_out);

/* ---- Sim3Solver (src/sg-slam/include/Sim3Solver.h:36-130, src/sg-slam/src/Sim3Solver.cc), the RANSAC initialiser of LoopClosing::ComputeSim3 (LoopClosing.cc:274-301) ----
 * The constructor's flattening stays with the caller (:40-111): for every usable pair (vpMatched12[i1] set, both map points good and indexed in their keyframes)
 * x3dc1 = Rcw1 * X3D1w + tcw1, x3dc2 = Rcw2 * X3D2w + tcw2 (n x 3 floats), max_err1/2 = 9.210 * mvLevelSigma2[octave] (n floats), K1 / K2 = fx, fy, cx, cy.
 * create runs FromCameraToImage (:407-425) and SetRansacParameters() with the class defaults (0.99, 6, 300).
 * iterate(nIterations, bNoMore, vbInliers, nInliers) (:140-208): every iteration of the call is a hypothesis evaluated on the device (three correspondences, Horn's
 * closed form ComputeSim3 :228-337 in the reference's cv::Mat arithmetic incl. cv::eigen's Jacobi and cv::Rodrigues, CheckInliers :340-365); the sequential accept rule
 * (>= best so far, return at the first model with more than minInliers inliers) is replayed in iteration order, iterations after a success are not consumed.
 * Random numbers: the reference calls the process-global rand() (DUtils::Random::RandomInt, Random.cpp:71-74), three times per iteration.  rand_draws = those raw rand()
 * values (3 x n_iterations; only the first 3 x *iterations_run are consumed — a caller sharing the global stream passes one iteration per call), or NULL: the solver then
 * uses its own replica of glibc's rand() seeded with rand_seed at creation (srand(rand_seed)).
 * Outputs: *found = a model was returned (T12 = 4x4 row-major mBestT12, inliers[n] over the n pairs — the caller maps them through mvnIndices1 — *n_inliers);
 * *no_more = bNoMore.  get_estimate = GetEstimatedRotation / Translation / Scale of the best model so far, and the effective mRansacMaxIts.
 * A failed create clears *out and returns the status that occurred: SGX_ERR_NOMEM for a refused allocation, SGX_ERR_DEVICE for a failed copy. */
typedef struct sgx_sim3_solver sgx_sim3_solver;
int sgx_sim3_solver_create(int n, const float *x3dc1, const float *x3dc2, const float *max_err1, const float *max_err2, const float *K1, const float *K2, int fix_scale,
                           unsigned rand_seed, sgx_sim3_solver **out);
int sgx_sim3_solver_set_ransac_parameters(sgx_sim3_solver *s, double probability, int min_inliers, int max_iterations);
int sgx_sim3_solver_iterate(sgx_sim3_solver *s, int n_iterations, const int32_t *rand_draws, float *T12, int32_t *no_more, uint8_t *inliers, int32_t *n_inliers,
                            int32_t *found, int32_t *iterations_run);
int sgx_sim3_solver_get_estimate(const sgx_sim3_solver *s, float *R12, float *t12, float *scale, int32_t *max_iterations);
void sgx_sim3_solver_destroy(sgx_sim3_solver *s);

/* ---- PnPsolver (src/sg-slam/include/PnPsolver.h, src/sg-slam/src/PnPsolver.cc), the EPnP RANSAC of Tracking::Relocalization (Tracking.cc:1504-1530) ----------------
 * The constructor's flattening stays with the caller (:67-110): for every matched map point that is not bad, p2d = mvKeysUn[i].pt (x, y), sigma2 =
 * mvLevelSigma2[octave], p3dw = its world position (n x 3); the caller keeps the keypoint index i (mvKeyPointIndices) to map inliers back.  cam4 = fx, fy, cx, cy.
 * create ends with SetRansacParameters() and its defaults (0.99, 8, 300, 4, 0.4, 5.991).  set_ransac_parameters = :121-157 (min_set must be 4); mnIterations and the best
 * model are kept.  iterate(nIterations, bNoMore, vbInliers, nInliers) = :165-257 with its quirks: the loop condition `mnIterations < mRansacMaxIts || nCurrent <
 * nIterations` runs max(nIterations, mRansacMaxIts - mnIterations) hypotheses; Refine (:260-306, EPnP on the best-so-far inliers, success only with more than
 * mRansacMinInliers) follows every hypothesis with at least mRansacMinInliers inliers and ends the call at its first success; otherwise, once mnIterations >=
 * mRansacMaxIts, *no_more is set and the best model is returned if it has at least mRansacMinInliers inliers.  EPnP and the OpenCV algebra it calls run in fp64 on the
 * device (sg_slam_amd/csrc/sgx_pnp_kernels.h, which also defines the two undefined cases of the reference: no Gauss-Newton update on a singular A, IEEE division by a
 * zero beta).
 * Random numbers: the reference draws from the process-global rand() (DUtils::Random::RandomInt, Random.cpp:47-50), four times per hypothesis, and so does
 * LoopClosing's Sim3Solver on another thread, so the reference's own sequence is not reproducible.  Here every solver owns its stream: rand_draws = the raw rand()
 * values, 4 x the call's hypothesis count (max(n_iterations, max_iterations - iterations), get_estimate), of which the first 4 x *iterations_run are consumed; or NULL:
 * the solver's replica of glibc's rand(), srand(rand_seed) at creation, draws of hypotheses that did not run are handed back.
 * Outputs: *found = a model was returned (Tcw 4 x 4 row-major float, inliers[n] over the n correspondences, *n_inliers); *no_more = bNoMore.  get_estimate: mBestTcw,
 * the effective mRansacMaxIts and mRansacMinInliers, mnIterations and mnBestInliers.  Synchronous, host pointers.
 * A failed create clears *out and returns the status that occurred: SGX_ERR_NOMEM for a refused allocation, SGX_ERR_DEVICE for a failed copy. */
typedef struct sgx_pnp_solver sgx_pnp_solver;
int sgx_pnp_solver_create(int n, const float *p2d, const float *sigma2, const float *p3dw, const float *cam4, unsigned rand_seed, sgx_pnp_solver **out);
int sgx_pnp_solver_set_ransac_parameters(sgx_pnp_solver *s, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, float th2);
int sgx_pnp_solver_iterate(sgx_pnp_solver *s, int n_iterations, const int32_t *rand_draws, float *Tcw, int32_t *no_more, uint8_t *inliers, int32_t *n_inliers,
                           int32_t *found, int32_t *iterations_run);
int sgx_pnp_solver_get_estimate(const sgx_pnp_solver *s, float *best_tcw, int32_t *max_iterations, int32_t *min_inliers, int32_t *iterations, int32_t *best_inliers);
void sgx_pnp_solver_destroy(sgx_pnp_solver *s);
/* Batch: B independent solvers, one launch sequence per iterate() for all of them, state (mnIterations, the best model) kept on the device between calls.
 * set_dev (re)creates the B solvers: offsets[B + 1] (host) delimit each solver's correspondences in the concatenated device arrays p2d (x, y), sigma2, p3dw (x, y, z);
 * cam (host, B x 4) = fx, fy, cx, cy; ransac (host, B x 6) = SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2) of each solver;
 * rand_seeds (host, B) seeds each solver's rand() replica (NULL: 0).  iterate_dev = iterate(n_iterations) of every solver on `stream`: rand_draws_dev (device, optional)
 * = solver b's raw rand() values at b * draw_stride, 4 per hypothesis as above; result_dev (B x 4 int32) = found, bNoMore, nInliers, iterations run; tcw_dev (B x 16);
 * inliers_dev (offsets[B] bytes).  Asynchronous on `stream`.
 * A failed create clears *out and returns the status that occurred: SGX_ERR_NOMEM for a refused allocation, SGX_ERR_DEVICE for a failed copy.  A failed set_dev leaves the batch not set: iterate_dev answers SGX_ERR_INVALID until a
 * set_dev succeeds. */
typedef struct sgx_pnp_batch sgx_pnp_batch;
int sgx_pnp_batch_create(int max_solvers, int max_correspondences, sgx_pnp_batch **out);
int sgx_pnp_batch_set_dev(sgx_pnp_batch *t, int B, const int32_t *offsets, const float *p2d_dev, const float *sigma2_dev, const float *p3dw_dev, const float *cam,
                          const double *ransac, const uint32_t *rand_seeds, void *stream);
int sgx_pnp_batch_iterate_dev(sgx_pnp_batch *t, int n_iterations, const int32_t *rand_draws_dev, int draw_stride, int32_t *result_dev, float *tcw_dev,
                              uint8_t *inliers_dev, void *stream);
void sgx_pnp_batch_destroy(sgx_pnp_batch *t);

/* ---- Initializer (src/sg-slam/include/Initializer.h, src/sg-slam/src/Initializer.cc), the two-view initialisation of Tracking::MonocularInitialization
 * (Tracking.cc:605-671): the consumer of sgx_match_search_for_initialization ---------------------------------------------------------------------------------------
 * create = the constructor (:33-42): keys1_un = ReferenceFrame.mvKeysUn, cam4 = fx, fy, cx, cy, sigma and iterations as Tracking passes them (1.0, 200).
 * initialize = Initialize (:44-121) with keys2_un = CurrentFrame.mvKeysUn and matches12 = vMatches12 (n1 entries, -1 = unmatched): the 8-point sets of every
 * iteration, FindHomography and FindFundamental over all of them (Normalize runs over ALL keys of each frame; the float score is summed in match order; the first
 * strictly greater score wins), RH = SH / (SH + SF), ReconstructH (RH > 0.40; `minParallax` 1.0, `minTriangulated` 50) or ReconstructF with CheckRT / Triangulate,
 * all on the device (sg_slam_amd/csrc/sgx_init_kernels.h states the OpenCV algebra it restates).
 * Outputs: *ok = the return value; R21 (3 x 3 row-major), t21; p3d (n1 x 3) and triangulated (n1) = vP3D and vbTriangulated, indexed by the keypoint index of frame 1
 * (a point that passes every gate of CheckRT is written even when its cosParallax >= 0.99998 leaves triangulated 0); all zero when *ok = 0.  inliers (n1) =
 * vbMatchesInliers of the chosen model, scattered to the keypoint index of frame 1.  report (optional): the scores, the chosen model (0 H, 1 F), N, the inlier counts
 * of both winners, the number of motion hypotheses checked (8, 4, or 0 when ReconstructH left at `d1/d2 < 1.00001 || d2/d3 < 1.00001`), per hypothesis nGood, the
 * selected cosine vCosParallax[min(50, nGood - 1)] and its parallax in degrees, best_hyp = bestSolutionIdx (H) or the first hypothesis with maxGood (F; -1 = none),
 * and the winning H21 / F21 (zero when no hypothesis scored above 0).
 * parallax = (float)(acos((double)cos) * 180 / CV_PI) is evaluated on the host; the device applies the two gates as cosine thresholds derived from that expression.
 * Defined where the reference is undefined: fewer than 8 matches -> *ok = 0 and no random number is consumed; no hypothesis of the chosen model scored above 0 (the
 * reference decomposes an empty matrix) -> *ok = 0; a hypothesis whose score is NaN never wins; matches12[i] >= n2 counts as unmatched.
 * Random numbers: the reference draws 8 x iterations values from the process-global rand() after SeedRandOnce(0).  rand_draws = those raw rand() values, or NULL: the
 * object's replica of glibc's rand(), srand(rand_seed) at creation, continuing across calls (seed 0 = a process's first Initialize).  Synchronous, host pointers.
 * A failed create clears *out and returns the status that occurred: SGX_ERR_NOMEM for a refused allocation, SGX_ERR_DEVICE for a failed copy.  An initialize that fails while it makes room for a larger frame 2 leaves the
 * initializer as it was: usable at its old size, the replica unmoved. */
typedef struct sgx_initializer sgx_initializer;
typedef struct sgx_init_report {
    float SH, SF, RH; int32_t model /* 0 H, 1 F */, n_matches, n_inliers_h, n_inliers_f, n_hyp /* 8, 4 or 0 */, best_hyp;
    int32_t n_good[8]; float cos_parallax[8], parallax[8]; float H21[9], F21[9];
} sgx_init_report;
int sgx_initializer_create(int n1, const sgx_keypoint *keys1_un, const float *cam4, float sigma, int iterations, unsigned rand_seed, sgx_initializer **out);
int sgx_initializer_initialize(sgx_initializer *s, int n2, const sgx_keypoint *keys2_un, const int32_t *matches12, const int32_t *rand_draws, float *R21, float *t21,
                               float *p3d, uint8_t *triangulated, uint8_t *inliers, int32_t *ok, sgx_init_report *report);
void sgx_initializer_destroy(sgx_initializer *s);
/* Batch: B independent frame pairs, one launch sequence for all of them.  create: max_keys = capacity of each concatenated key array, max_matches = capacity of the
 * concatenated matches12 array (one entry per key of frame 1), iterations = mMaxIterations of every pair.  run_dev: offsets1 / offsets2 (host, B + 1) delimit pair b's
 * keys in keys1_dev / keys2_dev; matches12_dev, p3d_dev, triangulated_dev and inliers_dev follow offsets1; cam (host, B x 4), sigma (host, B); rand_seeds (host, B)
 * re-seeds the pairs' rand() replicas before this run (NULL: they continue; all start as srand(0)); rand_draws_dev (device, optional) = pair b's 8 x iterations raw
 * rand() values at b * draw_stride.  Outputs on the device: R21_dev (B x 9), t21_dev (B x 3), ok_dev (B), report_dev (B; its parallax[] stays 0: the host
 * evaluates acos).  Asynchronous on `stream`. A failed create clears *out and returns the status that occurred: SGX_ERR_NOMEM for a refused allocation, SGX_ERR_DEVICE for a failed copy. */
typedef struct sgx_init_batch sgx_init_batch;
int sgx_init_batch_create(int max_pairs, int max_keys, int max_matches, int iterations, sgx_init_batch **out);
int sgx_init_batch_run_dev(sgx_init_batch *t, int B, const int32_t *offsets1, const sgx_keypoint *keys1_dev, const int32_t *matches12_dev, const int32_t *offsets2,
                           const sgx_keypoint *keys2_dev, const float *cam, const float *sigma, const uint32_t *rand_seeds, const int32_t *rand_draws_dev, int draw_stride,
                           float *R21_dev, float *t21_dev, float *p3d_dev, uint8_t *triangulated_dev, uint8_t *inliers_dev, int32_t *ok_dev, sgx_init_report *report_dev,
                           void *stream);
void sgx_init_batch_destroy(sgx_init_batch *t);

/* ---- Detector3D (src/sg-slam/include/Detector3D.h, src/sg-slam/src/Detector3D.cc) and ObjectDatabase (src/sg-slam/src/ObjectDatabase.cc) ---------------------------
 * Detector3D::DetectOne (:41-168) for one Object2D of Detector2D (mvObjects2D), as PointCloudMapping::generatePointCloud calls it for every keyframe
 * (PointcloudMapping.cc:145-151, :189-190): the crop of the box's central 60 % (rows / columns (size_t)h * 0.2 .. (size_t)h * 0.8, depth inside
 * [camera_valid_depth_min, camera_valid_depth_max] and not NaN), the world points of the crop (camera point in float as PointcloudMapping.cc:176-178 writes it, Twc in
 * double as pcl::transformPointCloud applies it), pcl::StatisticalOutlierRemoval (mean_k, stddev_mul), pcl::EuclideanClusterExtraction (tolerance, min / max size)
 * and the selection loop (:101-140: compute3DCentroid, the world-z test against camera_valid_depth_min, GetProjectedROI, GetSimilarity, the `>` / `else if >`
 * bookkeeping and the DetectSimilarCompareRatio test).  PCL and FLANN are restated from their published algorithms (tests/obj3d_ref.py), unpinned.
 * Defined cases: fewer than mean_k + 1 crop points, or no cluster chosen: found = 0 (the reference reads past the neighbour list / returns an object with an
 * uninitialised centroid); equal-size clusters are ordered by their smallest point; powf(x, 2) = x * x; a NaN similarity never wins.  voxel_leaf_size is read and
 * unused, as in the reference (its voxel filter is commented out).
 * SGX_ERR_INVALID: mean_k < 1, depth bounds or tolerance that are not finite, a rect that is not inside the image (x, y, w, h >= 0, x + w <= width, y + h <= height),
 * a crop of more than max_crop_points cells.  Twc must be finite.
 * The diagnostics are part of the record: crop_points (points of the crop), kept_points (after the filter), components (of the kept points, any size), clusters
 * (min <= size <= max), best_cluster_size / best_similar1 / best_similar2 / best_roi (x, y, width, height) of the selection loop (also when the ratio test then
 * rejects; -1 / 0 when no cluster was chosen), larger_window_points (points whose neighbour search needed more than the first pixel window: an implementation
 * figure, equal between the device and the emulator).  centroid and size are 0 when found == 0. */
typedef struct sgx_obj3d_params {
    double sor_stddev_mul;                                  /* Detector3D.Sor_StddevMulThresh */
    int32_t sor_mean_k;                                     /* Detector3D.Sor_MeanK */
    int32_t cluster_min_size, cluster_max_size;             /* Detector3D.EuclideanClusterMinSize / MaxSize */
    float voxel_leaf_size;                                  /* Detector3D.Voxel_LeafSize: unused */
    float cluster_tolerance;                                /* Detector3D.EuclideanClusterTolerance */
    float similar_compare_ratio;                            /* Detector3D.DetectSimilarCompareRatio */
    float camera_valid_depth_min, camera_valid_depth_max;   /* PointCloudMapping.camera_valid_depth_Min / Max */
} sgx_obj3d_params;
typedef struct sgx_obj3d_job { int32_t image, class_id; float prob, x, y, w, h; } sgx_obj3d_job;        /* image index in the batch; Object2D id, prob, rect */
typedef struct sgx_obj3d_result {
    int32_t found, class_id; float prob, centroid[3], size[3];
    int32_t crop_points, kept_points, components, clusters, best_cluster_size, larger_window_points;
    float best_similar1, best_similar2, best_roi[4];
} sgx_obj3d_result;
typedef struct sgx_obj3d sgx_obj3d;
/* width x height images, at most max_images images and max_jobs jobs per batch, at most max_crop_points cells per crop; 0 = the largest crop there is:
 * Detector2D only clamps its boxes to the image (Detector2D.cc:63-71), so a box can be the whole image and its crop the central 60 % of it, 384 x 288 = 110 592 cells
 * of a 640 x 480 image.  The workspace is 32 bytes per cell and job, plus 64 bytes per job for every max_crop_points / max(cluster_min_size, 1) cells: the surviving
 * clusters are ranked pairwise by one workgroup, so a cluster_min_size of a few points on a large crop costs (cells / min_size)^2 reads there.
 * A failed create clears *out and returns the status that occurred: SGX_ERR_NOMEM for a refused allocation, SGX_ERR_DEVICE for a failed copy. */
int sgx_obj3d_create(int width, int height, int max_images, int max_jobs, int max_crop_points, const sgx_obj3d_params *params, sgx_obj3d **out);
void sgx_obj3d_destroy(sgx_obj3d *h);
/* n_jobs jobs over n_images depth images (device, float metres as mImDep, n_images x height x pitch floats), cam4 = fx, fy, cx, cy (host), twc_dev = n_images x 16
 * doubles (device, Twc row-major), jobs (host; copied before the call returns), results_dev = n_jobs records (device).  One launch sequence, asynchronous on
 * `stream`.  A handle serves one batch at a time: batches of one handle must be ordered by their streams. */
int sgx_obj3d_detect_batch_dev(sgx_obj3d *h, const float *depth_dev, int pitch, int n_images, const float *cam4, const double *twc_dev, const sgx_obj3d_job *jobs,
                               int n_jobs, sgx_obj3d_result *results_dev, void *stream);
/* one job (image 0) from host memory: depth = height x width floats, twc = 16 doubles.  Synchronous. */
int sgx_obj3d_detect(sgx_obj3d *h, const float *depth, const float *cam4, const double *twc, const sgx_obj3d_job *job, sgx_obj3d_result *result);
/* ObjectDatabase::addObject (:44-112), host code: objects of the same class (the reference compares object_name = class_names[class_id]) within mvSizes[class_id]
 * (0.6; bottle 5: 0.2, chair 9: 1.0, tvmonitor 20: 0.5) of the nearest one, searched from center_distance = 100, are merged by a mean of prob, centroid and size;
 * otherwise the object is appended with object_id = ++DataBaseSize.  class_id outside 0..20 is SGX_ERR_INVALID (the reference indexes mvSizes with it).
 * *object_id = the id appended or merged into, *merged = 1 when merged (either may be NULL). */
typedef struct sgx_semantic_object { int32_t class_id, object_id; float prob, centroid[3], size[3]; } sgx_semantic_object;
typedef struct sgx_objdb sgx_objdb;
int sgx_objdb_create(sgx_objdb **out);
void sgx_objdb_destroy(sgx_objdb *db);
int sgx_objdb_add(sgx_objdb *db, const sgx_semantic_object *obj, int32_t *object_id, int32_t *merged);
int sgx_objdb_size(const sgx_objdb *db);                                      /* number of objects (mvSemanticObject.size()) */
int sgx_objdb_get(const sgx_objdb *db, int index, sgx_semantic_object *out);  /* mvSemanticObject[index] */

/* ---- PointCloudMapping (src/sg-slam/include/PointcloudMapping.h, src/sg-slam/src/PointcloudMapping.cc) -----------------------------------------------------------
 * The cloud of a keyframe as PointCloudMapping::generatePointCloud / generatePointCloudForDyamic (:69-194) build it and MapViewer filters it (:252-286 voxel_local /
 * sor_local, :332-338 voxel_global / sor_global on temp_globalMap): every pixel of the depth image as a coloured point, pcl::VoxelGrid<PointXYZRGB> with leaf L on all
 * three axes, pcl::StatisticalOutlierRemoval (mean_k, stddev_mul), the axis map slam_to_ros_mode_transform (:364-375).  PCL is restated from its published sources
 * (tests/cloud_ref.py), unpinned.
 * Generate: the cloud has width * height points, index m * width + n, every one x = y = z = 0, r = g = b = 0, a = 255 (PCL's default point).  A pixel is skipped when
 * d < min || d > max || isnan(d), and, when consider_dynamic and the image's have_dynamic flag are set, when it lies in a dynamic rect: n > int(x) && n < int(x + w) &&
 * m > int(y) && m < int(y + h) (:449-458; float sum, C truncation; a value no int holds converts to the nearest int, NaN to 0).  Any other pixel gets z = d,
 * x = (n - cx) * d / fx, y = (m - cy) * d / fy in float and r = color[3n + 2], g = color[3n + 1], b = color[3n].  A skipped pixel is NOT dropped: it stays a point at
 * the camera origin with colour 0 and goes through the filters, as in the reference.
 * SGX_CLOUD_LOCAL (localMap): the filters run in the camera frame, then every surviving point becomes (z, -x, -y).  SGX_CLOUD_WORLD (temp_globalMap): every point,
 * the origin points included, becomes (float)(((T[r][0]*x + T[r][1]*y) + T[r][2]*z) + T[r][3]) in double, then (z, -x, -y), then the filters run.
 * VoxelGrid: inv = 1.0f / L; min_p, max_p the extremes over the finite points; dx = (int64)((max_p[0] - min_p[0]) * inv) + 1 (dy, dz alike); min_b = (int)floor(min_p *
 * inv), max_b alike, div = max_b - min_b + 1; ijk = (int)(floor(p * inv) - (float)min_b), idx = ijk0 + ijk1 * div0 + ijk2 * div0 * div1; one point per occupied idx
 * in ascending idx: float running sums of x, y, z, (float)r, (float)g, (float)b, (float)a over the voxel's points, xyz = sum / (float)n, channel = (uint32)(sum /
 * (float)n).  StatisticalOutlierRemoval on the voxel cloud as for sgx_obj3d: a point goes when its mean distance to its mean_k nearest neighbours is > thr.
 * Defined cases:
 *  1. fewer than mean_k + 1 voxel points (the reference reads a stale neighbour list): no points, flags has SGX_CLOUD_FEW_POINTS;
 *  2. dx * dy * dz > INT32_MAX (PCL warns and passes the cloud through unfiltered), or |min_p * inv| or |max_p * inv| >= 2^31, or div0 * div1 * div2 > INT32_MAX (PCL's
 *     int index overflows): no points, flags has SGX_CLOUD_LEAF_TOO_SMALL, and the call succeeds: a batch does not fail because of one keyframe;
 *  3. the points of a voxel are summed in ascending point index (PCL sorts (idx, point) with an unstable sort);
 *  4. a zero that the axis map produces is written as +0;
 *  5. a point that is not finite (a Twc that is not finite) joins neither the extremes nor a voxel, as in PCL.
 * SGX_ERR_INVALID: mean_k < 1, a leaf that is not finite or <= 0, depth bounds that are not finite, more than max_boxes rects or a NaN in Twc (both in sgx_cloud_build,
 * which sees them; sgx_cloud_build_batch_dev reads nothing back: it takes min(n_boxes, max_boxes) rects, and a NaN in Twc gives case 5).
 * The result record: n_points (points written), n_pixels_used (pixels not skipped), n_voxels (voxel points before the outlier filter), flags, mean and thr of the
 * outlier filter, larger_window_points (voxel points whose neighbour search needed more than the first cell window: an implementation figure, equal between the device
 * and the emulator). */
#define SGX_CLOUD_LOCAL 0
#define SGX_CLOUD_WORLD 1
#define SGX_CLOUD_FEW_POINTS 1
#define SGX_CLOUD_LEAF_TOO_SMALL 2
#define SGX_CLOUD_MAX_BOXES 128
typedef struct sgx_cloud_params {
    double sor_stddev_mul;                                  /* PointCloudMapping.Sor_Local_StddevMulThresh / Sor_Global_StddevMulThresh */
    int32_t sor_mean_k;                                     /* PointCloudMapping.Sor_Local_MeanK / Sor_Global_MeanK */
    int32_t consider_dynamic;                               /* PointCloudMapping.is_map_construction_consider_dynamic */
    float voxel_leaf_size;                                  /* PointCloudMapping.Voxel_Local_LeafSize / Voxel_Global_LeafSize */
    float camera_valid_depth_min, camera_valid_depth_max;   /* PointCloudMapping.camera_valid_depth_Min / Max */
    int32_t reserved;
} sgx_cloud_params;
typedef struct sgx_cloud_point { float x, y, z; uint32_t rgba; } sgx_cloud_point;      /* rgba = a << 24 | r << 16 | g << 8 | b: PCL's PointXYZRGB, the x y z rgb fields of a PointCloud2 */
typedef struct sgx_cloud_result {
    int32_t n_points, n_pixels_used, n_voxels, flags, larger_window_points, reserved;
    double mean, thr;
} sgx_cloud_result;
typedef struct sgx_cloud sgx_cloud;
/* width x height images (at most 2^20 pixels), at most max_images keyframes per batch and max_boxes <= SGX_CLOUD_MAX_BOXES dynamic rects per keyframe; mode =
 * SGX_CLOUD_LOCAL or SGX_CLOUD_WORLD.  The workspace is 76 bytes per pixel and keyframe.  A failed create clears *out and returns the status that occurred. */
int sgx_cloud_create(int width, int height, int max_images, int max_boxes, int mode, const sgx_cloud_params *params, sgx_cloud **out);
void sgx_cloud_destroy(sgx_cloud *h);
/* n_images keyframes in one launch sequence, asynchronous on `stream`, no read-back: depth_dev = n_images x height x depth_pitch floats (metres, as mImDep),
 * color_dev = n_images x height x color_pitch bytes (3 bytes per pixel in mImRGB's order), cam4 = fx, fy, cx, cy (host), twc_dev = n_images x 16 doubles (Twc
 * row-major; may be NULL in SGX_CLOUD_LOCAL), boxes_dev = n_images x max_boxes x (x, y, w, h) floats, n_boxes_dev and have_dynamic_dev = n_images int32
 * (mvPotentialDynamicBorderForMapping, its size, mbHaveDynamicObjectForMapping; all three may be NULL: no dynamic region), points_dev = max_images x width * height
 * records (keyframe i writes its n_points records from i * width * height on), results_dev = n_images records.  A handle serves one batch at a time. */
int sgx_cloud_build_batch_dev(sgx_cloud *h, const float *depth_dev, int depth_pitch, const uint8_t *color_dev, int color_pitch, int n_images, const float *cam4,
                              const double *twc_dev, const float *boxes_dev, const int32_t *n_boxes_dev, const int32_t *have_dynamic_dev, sgx_cloud_point *points_dev,
                              sgx_cloud_result *results_dev, void *stream);
/* one keyframe from host memory (tight images; twc = 16 doubles, may be NULL in SGX_CLOUD_LOCAL; boxes = n_boxes x 4 floats): the record, and its n_points points
 * into points (SGX_ERR_OVERFLOW when cap is smaller; the record is written all the same).  Synchronous. */
int sgx_cloud_build(sgx_cloud *h, const float *depth, const uint8_t *color, const float *cam4, const double *twc, const float *boxes, int n_boxes, int have_dynamic,
                    sgx_cloud_point *points, int cap, sgx_cloud_result *result);
/* camera_to_map_tf of MapViewer (:254-265), host code: tcw = the keyframe's float pose Tcw (16 floats, row-major).  Rwc = Rcw^T, twc = -Rwc * tcw rounded to float
 * from a double product (cv::gemm); Q = Eigen::Quaterniond(Rwc as double); origin = (twc[2], -twc[0], -twc[1]); rotation = (Q.z, -Q.x, -Q.y, Q.w) in tf's x, y, z, w. */
int sgx_cloud_camera_to_map_tf(const float *tcw, double origin[3], double rotation[4]);

/* ---- OctomapServer (src/octomap_server/src/OctomapServer.cpp) -----------------------------------------------------------------------------------------------------
 * The occupancy map that consumes the keyframe cloud: insertCloudCallback's non-ground branch (:261-354: transformPointCloud, three PassThrough filters), insertScan
 * (:356-480: one ray per point, free cells on the rays, occupied end cells, one update per cell and scan) and the tree queries of publishAll (:484-: the occupied /
 * free cell centres, the projected 2-D grid of handlePreNodeTraversal / update2DMap with m_projectCompleteMap, :934-1107).  Occupancy only: no colour, no ground
 * filter, no speckle filter, no serialisation, max_depth 16.  octomap is restated from its published algorithm (tests/octomap_ref.py), unpinned.
 * The map is kept as depth-16 cells; octomap's maximally pruned tree gives every cell the same log-odds (tests/test_octomap_emu.py holds the equivalence).
 * Keys: coordToKeyChecked(c) = (int)floor((1.0 / res) * (double)c) + 32768, valid in [0, 65536); keyToCoord(k) = ((double)(k - 32768) + 0.5) * res.
 * Defaults are octomap_server's: res 0.05, prob_hit 0.7, prob_miss 0.4, thres_min 0.12, thres_max 0.97, max_range -1 (none), bounds -/+DBL_MAX, min_size 0.
 * sgx_octomap_create: SGX_ERR_INVALID for a res that is not finite or <= 0, a probability or clamp outside (0, 1), thres_min >= thres_max, a NaN bound,
 * max_bricks outside [1, 2^17] (the cells query ranks the B bricks by counting, B^2 comparisons), max_points_per_scan outside [1, 2^24].  Device memory: 2 072 bytes per brick of 8 x 8 x 8 cells, 144 per table slot (the next
 * power of two >= 2 * max_bricks slots) and 32 per point. */
typedef struct sgx_octomap_params {
    double res, prob_hit, prob_miss, thres_min, thres_max;
    double max_range;                                            /* < 0: none */
    double pointcloud_min_x, pointcloud_max_x, pointcloud_min_y, pointcloud_max_y, pointcloud_min_z, pointcloud_max_z;       /* PassThrough limits, taken as float */
    double occupancy_min_z, occupancy_max_z;                     /* the z window of the cell lists and the grid */
    double min_size_x, min_size_y;                               /* padding of the 2-D grid */
} sgx_octomap_params;
#define SGX_OCTOMAP_ORIGIN_OUT_OF_RANGE 1   /* the sensor origin has no key: every ray is invalid, end cells are still inserted (:359-363, :400-410) */
#define SGX_OCTOMAP_RAY_LEFT_KEYSPACE 2     /* a ray would have stepped outside [0, 65535] (octomap only asserts): the ray ends there */
#define SGX_OCTOMAP_MAP_FULL 4              /* the scan needs more than max_bricks bricks: the map is unchanged; RAY_LEFT_KEYSPACE is not reported for such a scan */
#define SGX_OCTOMAP_TOO_MANY_POINTS 8       /* more than max_points_per_scan points: the map is unchanged, only n_in and flags are set */
typedef struct sgx_octomap_record {
    int32_t n_in, n_passed;                 /* points of the scan, points behind the PassThrough filters */
    int32_t n_truncated;                    /* beyond max_range: the ray ends at new_end, which is free */
    int32_t n_bad_end_key, n_invalid_rays;  /* end points without a key; rays computeRayKeys refuses */
    int32_t n_free_updates, n_occupied_updates, n_new_cells;    /* cells that got a miss (free set minus occupied set) / a hit; cells unknown before; 0 when MAP_FULL */
    int32_t bbx_min[3], bbx_max[3];         /* m_updateBBXMin / Max: the origin key (when valid) and every inserted end key; 65535 / 0 when there is none */
    int32_t flags, reserved;
} sgx_octomap_record;
typedef struct sgx_octomap_cell { uint16_t key[3], reserved; float x, y, z, logodds; } sgx_octomap_cell;   /* the centre is (float)keyToCoord per axis */
typedef struct sgx_octomap_bounds_t { int32_t n_known, n_occupied, n_free, n_bricks, key_min[3], key_max[3]; } sgx_octomap_bounds_t;   /* occupied: logodds >= 0.0f; 65535 / 0 when empty */
#define SGX_OCTOMAP_GRID_EMPTY 1             /* no known cell: width = height = 0 */
#define SGX_OCTOMAP_GRID_KEY_OUT_OF_RANGE 2  /* a padded corner has no key (the reference logs an error and publishes nothing): width = height = 0 */
typedef struct sgx_octomap_grid_header_t {
    int32_t width, height, flags, reserved;
    int32_t pad_min_key[2], pad_max_key[2], key_min_z, key_max_z;
    double resolution, origin_x, origin_y;  /* nav_msgs::MapMetaData: origin = (float)keyToCoord(pad_min_key) - res * 0.5 */
} sgx_octomap_grid_header_t;
typedef struct sgx_octomap sgx_octomap;
int sgx_octomap_create(const sgx_octomap_params *params, int max_bricks, int max_points_per_scan, sgx_octomap **out);      /* *out is NULL after a failed call */
void sgx_octomap_destroy(sgx_octomap *h);
/* The synchronous entries (reset, insert, bounds, cells, project) run on the null stream and wait for it only: after sgx_octomap_insert_batch_dev or a _dev query on a
 * non-blocking stream the caller synchronises that stream first. */
int sgx_octomap_reset(sgx_octomap *h);                                                                    /* the map becomes empty, its capacity stays; synchronous */
/* n_scans scans in order, one asynchronous launch sequence on `stream`, nothing read back.  Scan i: *(int32_t *)((char *)n_points_dev + i * n_points_stride_bytes)
 * points at points_dev + i * point_stride (rgba ignored), the row-major 4 x 4 float sensorToWorld at sensor_to_world_dev + 16 * i, its record at records_dev + i.
 * n_points_dev may point at sgx_cloud_result.n_points (stride sizeof(sgx_cloud_result)) and points_dev at the output of sgx_cloud_build_batch_dev (stride
 * width * height): the chain needs no copy.  A scan that sets MAP_FULL or TOO_MANY_POINTS leaves the map as every query sees it; the later scans are applied. */
int sgx_octomap_insert_batch_dev(sgx_octomap *h, const sgx_cloud_point *points_dev, int64_t point_stride, const int32_t *n_points_dev, int64_t n_points_stride_bytes,
                                 const float *sensor_to_world_dev, int n_scans, sgx_octomap_record *records_dev, void *stream);
int sgx_octomap_insert(sgx_octomap *h, const sgx_cloud_point *points, int n_points, const float *sensor_to_world, sgx_octomap_record *record);   /* host pointers, synchronous */
int sgx_octomap_bounds(sgx_octomap *h, sgx_octomap_bounds_t *out);                                        /* synchronous */
/* the occupied (occupied != 0) or free cells with z + res / 2 > occupancy_min_z && z - res / 2 < occupancy_max_z in ascending Morton code of the key (bit 3i = x bit i,
 * 3i + 1 = y, 3i + 2 = z): the order of octomap's leaf iterator.  *n_cells is the true count; the first cap are written; sgx_octomap_cells answers SGX_ERR_OVERFLOW
 * beyond cap.  One cells query of a handle at a time. */
int sgx_octomap_cells_dev(sgx_octomap *h, int occupied, sgx_octomap_cell *cells_dev, int cap, int32_t *n_cells_dev, void *stream);
int sgx_octomap_cells(sgx_octomap *h, int occupied, sgx_octomap_cell *cells, int cap, int32_t *n_cells);
/* OcTree::search at depth 16 for m keys (3 uint16 each) or m points (3 floats each), exactly one of the two pointers: the log-odds, a quiet NaN for unknown */
int sgx_octomap_search_dev(sgx_octomap *h, const uint16_t *keys_dev, const float *points_dev, int m, float *logodds_dev, void *stream);
/* the grid's header from the bounds (host code) and the grid: width x height int8, index x + y * width, -1 unknown, 100 when a passing occupied cell lies in the
 * column, 0 when only free ones do.  sgx_octomap_project = bounds + header + grid from host memory (SGX_ERR_OVERFLOW when width * height > cap). */
int sgx_octomap_grid_header(const sgx_octomap *h, const sgx_octomap_bounds_t *bounds, sgx_octomap_grid_header_t *out);
int sgx_octomap_project_dev(sgx_octomap *h, const sgx_octomap_grid_header_t *header, int8_t *grid_dev, void *stream);
int sgx_octomap_project(sgx_octomap *h, sgx_octomap_grid_header_t *header, int8_t *grid, int64_t cap);
/* sensorToWorld from the (origin, rotation = x, y, z, w) of sgx_cloud_camera_to_map_tf as tf + pcl_ros::transformAsMatrix form it: tf::Matrix3x3::setRotation in
 * double (s = 2 / |q|^2), every entry and the origin cast to float; row-major 4 x 4 */
int sgx_octomap_sensor_to_world(const double origin[3], const double rotation[4], float out[16]);

/* ---- The global map (src/sg-slam/src/PointcloudMapping.cc:332-360) --------------------------------------------------------------------------------------------------
 * MapViewer's accumulating dense cloud (/SG_SLAM/Global_Point_Clouds, is_global_pc_reconstruction): `*globalMap += *temp_globalMap` for every keyframe, and
 * voxel_global + sor_global over the WHOLE accumulated map when no keyframe is waiting or count > global_pc_update_kf_threshold.  The map is a device-resident list
 * of sgx_cloud_point in ROS axes (what SGX_CLOUD_WORLD builds).  PCL is restated as for sgx_cloud (tests/globalmap_ref.py), unpinned.
 * Append: the cloud's points go behind the points already there, in order; a point that is not finite is stored, as PCL's operator+= does.
 * Consolidate: pcl::VoxelGrid (leaf) then pcl::StatisticalOutlierRemoval (mean_k, stddev_mul) over the whole map, exactly as stated for sgx_cloud (header, ijk,
 * ascending idx, float running sums in ascending point index, so an old map point comes before the points appended after it; colour truncation; distances, K-th
 * smallest, tie rule, mean / threshold); a point that is not finite joins no voxel and is gone afterwards; the survivors, in ascending idx, replace the map.  There
 * is no axis map: the cloud is in ROS axes already.
 * Defined cases:
 *  1. a consolidation that sgx_cloud would answer with LEAF_TOO_SMALL or FEW_POINTS (<= mean_k voxel points, an empty map included) leaves the map exactly as it
 *     was and sets SGX_GMAP_LEAF_TOO_SMALL / SGX_GMAP_FEW_POINTS in the record: a refused call does not wipe an accumulated map;
 *  2. an appended cloud that does not fit into max_points is refused whole: SGX_GMAP_FULL in its record, offset -1, nothing appended; the later clouds of the same
 *     batch are still tried, in order, against the running size: the outcome is a function of the sizes alone.  A negative count is an empty cloud;
 *  3. sgx_globalmap_create: SGX_ERR_INVALID for mean_k < 1, a leaf that is not finite or <= 0, a NaN stddev_mul, max_points < 1 or > SGX_GMAP_MAX_POINTS.
 * SGX_GMAP_MAX_POINTS = 2^22: the sort's one-workgroup scan (k_cloud_scan) then walks 16 * 2048 tile counts, 128 a lane, and every index is far inside an int.
 * Device memory: 77 bytes per point of capacity.
 * The schedule is host code and the caller's (sg_slam_amd/globalmap.py: GlobalMapSchedule; sgx::GlobalMap::update): count starts at 0; after every appended
 * keyframe `if (!pending || count > threshold)` consolidate, publish, and count = 0 only when the published cloud is not empty; then count++ in every case.
 * The consolidation record: n_points_in (the map before), n_voxels (voxel points before the outlier filter), n_points (the map after the call: n_points_in when a
 * flag is set), flags, mean and thr of the outlier filter, and two implementation figures that are equal between the device and the emulator:
 * wider_window_points (voxel points whose first cell window was not proven and that searched windows of doubled radius, up to SGX_GMAP_MAX_RADIUS cells) and
 * whole_cloud_points (voxel points that searched the whole voxel cloud: those that the widest window did not prove, and every point when there is no search grid). */
#define SGX_GMAP_FEW_POINTS 1
#define SGX_GMAP_LEAF_TOO_SMALL 2
#define SGX_GMAP_FULL 4
#define SGX_GMAP_MAX_POINTS (1 << 22)
#define SGX_GMAP_MAX_RADIUS 16
typedef struct sgx_globalmap_params {
    double sor_stddev_mul;                                  /* PointCloudMapping.Sor_Global_StddevMulThresh */
    int32_t sor_mean_k;                                     /* PointCloudMapping.Sor_Global_MeanK */
    float voxel_leaf_size;                                  /* PointCloudMapping.Voxel_Global_LeafSize */
} sgx_globalmap_params;
typedef struct sgx_globalmap_append_record {
    int32_t n_in;                                           /* points of the cloud */
    int32_t offset;                                         /* where its first point went; -1 when refused */
    int32_t map_size;                                       /* the map's size after this cloud */
    int32_t flags;                                          /* SGX_GMAP_FULL */
} sgx_globalmap_append_record;
typedef struct sgx_globalmap_result {
    int32_t n_points_in, n_voxels, n_points, flags, wider_window_points, whole_cloud_points;
    double mean, thr;
} sgx_globalmap_result;
typedef struct sgx_globalmap sgx_globalmap;
int sgx_globalmap_create(int max_points, const sgx_globalmap_params *params, sgx_globalmap **out);       /* *out is NULL after a failed call */
void sgx_globalmap_destroy(sgx_globalmap *h);
/* The synchronous entries (reset, append, consolidate, size, read) run on the null stream and wait for it only: after a _dev entry on a non-blocking stream the
 * caller synchronises that stream first. */
int sgx_globalmap_reset(sgx_globalmap *h);                                                               /* the map becomes empty, its capacity stays; synchronous */
/* n_clouds (at most 65535) clouds in order, one asynchronous launch sequence on `stream`, nothing read back.  Cloud i: *(int32_t *)((char *)n_points_dev + i *
 * n_points_stride_bytes) points at points_dev + i * point_stride, its record at records_dev + i.  n_points_dev may point at sgx_cloud_result.n_points (stride
 * sizeof(sgx_cloud_result)) and points_dev at the output of sgx_cloud_build_batch_dev (stride width * height): the chain depth image -> world cloud -> global map
 * needs no copy.  The clouds must not overlap the map. */
int sgx_globalmap_append_batch_dev(sgx_globalmap *h, const sgx_cloud_point *points_dev, int64_t point_stride, const int32_t *n_points_dev, int64_t n_points_stride_bytes,
                                   int n_clouds, sgx_globalmap_append_record *records_dev, void *stream);
int sgx_globalmap_append(sgx_globalmap *h, const sgx_cloud_point *points, int n_points, sgx_globalmap_append_record *record);     /* host pointers, synchronous */
/* voxel_global + sor_global over the whole map; one asynchronous launch sequence on `stream`, the record goes to result_dev.  One consolidation of a handle at a time. */
int sgx_globalmap_consolidate_dev(sgx_globalmap *h, sgx_globalmap_result *result_dev, void *stream);
int sgx_globalmap_consolidate(sgx_globalmap *h, sgx_globalmap_result *result);                           /* synchronous */
int sgx_globalmap_size(sgx_globalmap *h, int32_t *n_points);                                             /* synchronous */
/* *n_points is the true size; the first cap points are written; SGX_ERR_OVERFLOW beyond cap.  Synchronous. */
int sgx_globalmap_read(sgx_globalmap *h, sgx_cloud_point *points, int cap, int32_t *n_points);
/* the map and its size on the device, for a consumer on the same stream (both stay valid, at fixed addresses, for the life of the handle) */
int sgx_globalmap_points_dev(sgx_globalmap *h, const sgx_cloud_point **points_dev, const int32_t **n_points_dev);

/* ---- ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (src/sg-slam/include/ORBVocabulary.h:31-32) ----------------------------------------------
 * The bag-of-words transform behind Frame::ComputeBoW (src/sg-slam/src/Frame.cc:422-429) and KeyFrame::ComputeBoW (src/sg-slam/src/KeyFrame.cc:60-69):
 *     mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4)          src/sg-slam/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1139-1206
 * The per-feature tree descent (:1231-1273, FORB::distance FORB.cpp:81-101) runs on the device; BowVector / FeatureVector assembly and scoring are host work in
 * sgx_voc_transform / sgx_voc_score and device work in sgx_voc_bow_batch_dev and the sgx_kfdb_* entries.
 *
 * sgx_voc_load: loadFromTextFile (:1351-1438) for a path ending in ".txt", loadFromBinaryFile (:1467-1510) otherwise — System::System's rule (System.cc:69-73).
 * sgx_voc_create: the same tree from flat arrays: node 0 is the root, parent[i] < i for i >= 1, desc32 = nnodes x 32 bytes, is_leaf[i] gives node i the next word id.
 * A failed create clears *out and returns the status that occurred: SGX_ERR_NOMEM for a refused allocation, SGX_ERR_DEVICE for a failed copy. */
typedef struct sgx_voc sgx_voc;
int sgx_voc_load(const char *path, sgx_voc **out);
int sgx_voc_create(int k, int L, int scoring, int weighting, int nnodes, const int32_t *parent, const uint8_t *desc32, const double *weight, const uint8_t *is_leaf, sgx_voc **out);
int sgx_voc_info(const sgx_voc *v, int32_t *k, int32_t *L, int32_t *scoring, int32_t *weighting, int32_t *nnodes, int32_t *nwords);
void sgx_voc_destroy(sgx_voc *v);
/* transform(features, v, fv, levelsup) for one frame (host pointers, synchronous): desc = n x 32 bytes (mDescriptors rows).  bow_ids / bow_weights (capacity n) = the
 * BowVector in std::map order (word ids ascending; weights accumulated in feature order and normalised as the vocabulary's scoring demands), *nbow its size;
 * feat_node[i] = key of mFeatVec under which feature i sits (the node levelsup levels above its word), -1 when the word is stopped (weight <= 0, :1170) — exactly the
 * feat_node_* input of the sgx_match_search_by_bow* and sgx_match_search_for_triangulation entries; feat_word (optional) = word id per feature.
 * Divergence: when a descent reaches a leaf above level L - levelsup the reference leaves the node id unassigned (uninitialised variable); this build reports the leaf. */
int sgx_voc_transform(sgx_voc *v, int n, const uint8_t *desc, int levelsup, int32_t *bow_ids, double *bow_weights, int32_t *nbow, int32_t *feat_node, int32_t *feat_word);
/* the per-feature part for B frames resident on the device (frame b: d_n[b] descriptors at d_desc + b * desc_pitch; outputs with row pitch cap); asynchronous on `stream` */
int sgx_voc_transform_batch_dev(sgx_voc *v, const uint8_t *d_desc, size_t desc_pitch, const int32_t *d_n, int batch, int cap, int levelsup,
                                int32_t *d_word_id, double *d_weight, int32_t *d_feat_node, void *stream);
/* The BowVector half of transform() (:1159-1204; BowVector.cpp:33-86) for the B frames of sgx_voc_transform_batch_dev, on the device: d_word_id / d_weight are that
 * entry's outputs (row pitch cap, d_n[b] features in row b).  Row b of d_bow_ids / d_bow_weights (pitch cap) receives the BowVector, d_nbow[b] its size: word ids
 * ascending, weights of a repeated word accumulated in feature order (TF_IDF, TF) or the first one kept (IDF, BINARY), stopped words (!(w > 0), :1170) dropped, then the
 * / nd step of :1177-1183 or normalize() with the L1 / L2 norm summed in ascending word order: bit for bit what sgx_voc_transform returns for the same descriptors.
 * Rows and counts are the query layout of sgx_kfdb_detect_batch_dev.  cap <= 8192 (SGX_ERR_UNSUPPORTED beyond).  Asynchronous on `stream`. */
int sgx_voc_bow_batch_dev(sgx_voc *v, const int32_t *d_n, int batch, int cap, const int32_t *d_word_id, const double *d_weight,
                          int32_t *d_bow_ids, double *d_bow_weights, int32_t *d_nbow, void *stream);
/* double TemplatedVocabulary::score(const BowVector&, const BowVector&) (:1210-1215) for the L1 scoring the ORB vocabulary files select (L1Scoring::score,
 * src/sg-slam/Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-67; callers KeyFrameDatabase.cc:133,249, LoopClosing.cc:134); SGX_ERR_UNSUPPORTED for the other scoring types */
int sgx_voc_score(const sgx_voc *v, int n1, const int32_t *ids1, const double *w1, int n2, const int32_t *ids2, const double *w2, double *score);

/* ---- KeyFrameDatabase (src/sg-slam/src/KeyFrameDatabase.cc) -------------------------------------------------------------------------------------------------------
 * DetectRelocalizationCandidates (:199-309; caller Tracking::Relocalization, Tracking.cc:1467) and DetectLoopCandidates (:76-197; caller LoopClosing::DetectLoop,
 * LoopClosing.cc:141) on the device.  The handle keeps every keyframe's BowVector (the forward file), its id, its add() sequence number, its best-covisibility list and
 * its mRelocScore on the device.  The reference's inverted file is not built: a query intersects every keyframe's vector with the query's.  What the inverted file
 * decides beyond the set of keyframes found is their order in lKFsSharingWords (the query's words ascending, within a word that word's list in add() order), and that is
 * reproduced exactly: a keyframe's place is (its first common word, its add() sequence number) ascending; the candidates come back in that order.  Kept as written:
 * minCommonWords = (int)(maxCommonWords * 0.8f), the gate words > minCommonWords, si = (float) of L1Scoring's double sum in ascending word order
 * (ScoringObject.cpp:23-67), loop keeps si >= minScore, accScore a float sum in neighbour order, pBestKF moves on a strictly greater score, bestAccScore starts at
 * minScore (loop) or 0 (relocalisation), retention accScore > 0.75f * bestAccScore, the first occurrence of a pBestKF stands, the early empty returns.
 * Loop: a connected keyframe is never listed, so maxCommonWords is taken over the unconnected ones, and a neighbour counts only if it was listed and passed the word
 * gate (:93-102, :159).  Relocalisation: a neighbour counts if it shares any word (:273) and adds its mRelocScore whether or not THIS query scored it (:276): a neighbour
 * that shares a word but failed the gate contributes what an earlier query left in it.  mRelocScore is therefore persistent state of the handle, and query q of a batch
 * sees what queries 0 .. q-1 left: a batch of Q equals Q single calls bit for bit.
 * Defined where the reference is not:
 *   - mRelocScore of a keyframe no query has scored is 0 (the reference's constructor leaves it uninitialised, KeyFrame.cc:35); add() gives a keyframe a fresh one.
 *   - a query has no id: it behaves as one whose mnId is fresh and nonzero (mnRelocQuery(0) / mnLoopQuery(0) make id 0 special in the reference; nothing queries with it).
 *   - weights must be finite, a BowVector's ids strictly ascending and below the vocabulary's size, keyframe ids >= 0: anything else is SGX_ERR_INVALID.
 *   - an empty query or an empty database gives no candidates and a zero report.
 *   - a query longer than max_query_words is SGX_ERR_INVALID (single entries) or, in a batch, status = SGX_ERR_INVALID in its report, no candidates, no state change.
 *
 * sgx_kfdb_create: nwords and the scoring type are copied from the vocabulary (the pointer is not kept); SGX_ERR_UNSUPPORTED unless the scoring is L1, as sgx_voc_score.
 *   Capacity is fixed: max_keyframes keyframes, max_bow_entries BowVector entries over all of them, queries of at most max_query_words words (0 = 2048, 24 KB of LDS;
 *   at most 4096), batches of at most max_queries.  The workspace is 37 bytes x max_queries x max_keyframes.
 *   A failed create clears *out and returns the status that occurred: SGX_ERR_NOMEM for a refused allocation, SGX_ERR_DEVICE for a failed copy.
 * sgx_kfdb_add / erase / clear (:40-73), set_covisibility: host pointers, synchronous; none may run while a batch of this handle is in flight.  add of an id that is
 *   present, erase or set_covisibility of one that is absent: SGX_ERR_INVALID; a full database: SGX_ERR_NOMEM.  erase gives the keyframe's slot and entries back.  clear
 *   also forgets every mRelocScore.  set_covisibility: what pKFi->GetBestCovisibilityKeyFrames(10) returns for that keyframe (:151, :265), in its order, n <= 10; the
 *   caller refreshes it when its covisibility graph changes.  A neighbour id that is not in the database when a query runs contributes nothing.
 * sgx_kfdb_slots: kf_ids[max_keyframes] = the keyframe id held by every slot (-1 = free), *n_slots = slots in use from 0: the order of words_dev / score_dev. */
typedef struct sgx_kfdb sgx_kfdb;
typedef struct sgx_kfdb_report {
    int32_t n_sharing;                      /* lKFsSharingWords.size() */
    int32_t max_common_words, min_common_words, n_scores;
    int32_t n_score_and_match;              /* lScoreAndMatch.size() */
    float best_acc_score, min_score_to_retain;
    int32_t n_candidates;
    int32_t status;                         /* SGX_OK, or SGX_ERR_INVALID for a query of a batch that is longer than max_query_words */
} sgx_kfdb_report;                          /* fields past an early return stay 0 */
enum { SGX_KFDB_RELOCALIZATION = 0, SGX_KFDB_LOOP_CLOSING = 1 };
int sgx_kfdb_create(const sgx_voc *voc, int max_keyframes, int max_bow_entries, int max_query_words, int max_queries, sgx_kfdb **out);
void sgx_kfdb_destroy(sgx_kfdb *db);
int sgx_kfdb_size(const sgx_kfdb *db);                                                                        /* keyframes in the database */
int sgx_kfdb_add(sgx_kfdb *db, int32_t kf_id, int nbow, const int32_t *ids, const double *weights);           /* ids / weights as sgx_voc_transform returns them */
int sgx_kfdb_erase(sgx_kfdb *db, int32_t kf_id);
int sgx_kfdb_clear(sgx_kfdb *db);
int sgx_kfdb_set_covisibility(sgx_kfdb *db, int32_t kf_id, int n, const int32_t *neighbour_ids);
int sgx_kfdb_slots(const sgx_kfdb *db, int32_t *kf_ids, int32_t *n_slots);
/* One query from host memory, synchronous, a batch of one.  cand (capacity sgx_kfdb_size) = vpRelocCandidates / vpLoopCandidates as keyframe ids, *n_cand their number;
 * report may be NULL.  connected_ids = pKF->GetConnectedKeyFrames() (:78), min_score = minScore. */
int sgx_kfdb_detect_relocalization_candidates(sgx_kfdb *db, int nbow, const int32_t *ids, const double *weights, int32_t *cand, int32_t *n_cand, sgx_kfdb_report *report);
int sgx_kfdb_detect_loop_candidates(sgx_kfdb *db, int nbow, const int32_t *ids, const double *weights, int n_connected, const int32_t *connected_ids, float min_score,
                                    int32_t *cand, int32_t *n_cand, sgx_kfdb_report *report);
/* LoopClosing::DetectLoop's reference score (LoopClosing.cc:126-138): starts from the float 1 and takes the float-cast L1 score of the query against each listed
 * keyframe that is in the database; the caller lists only keyframes that are not isBad().  Host pointers, synchronous; leaves mRelocScore alone. */
int sgx_kfdb_min_score(sgx_kfdb *db, int nbow, const int32_t *ids, const double *weights, int n, const int32_t *kf_ids, float *min_score);
/* Q queries (mode: SGX_KFDB_RELOCALIZATION or SGX_KFDB_LOOP_CLOSING) as one launch sequence, asynchronous on `stream`; every pointer is device memory.  Query q = the
 * first counts_dev[q] entries of row q of ids_dev / weights_dev (row pitch `pitch` elements, counts_dev[q] <= pitch): the layout sgx_voc_bow_batch_dev writes.  Loop only: the connected
 * keyframes of query q are conn_ids_dev[conn_offsets_dev[q] .. conn_offsets_dev[q + 1]) (Q + 1 offsets; ids that are not in the database are ignored), its minScore
 * min_score_dev[q]; all three may be NULL for relocalisation.  cand_dev = Q rows of max_keyframes ids, n_cand_dev / report_dev one per query.  words_dev / score_dev
 * (optional, Q x max_keyframes, by slot: sgx_kfdb_slots) = what the reference leaves in the keyframes' public members after query q: mnRelocWords / mnLoopWords (0 for a
 * keyframe the query did not touch; 1 for a connected keyframe of a loop query, whose counter :95 resets at every word) and mRelocScore, or for a loop query mLoopScore
 * where this query wrote it and 0 elsewhere.  A handle serves one call at a time: calls of one handle must be ordered by their streams. */
int sgx_kfdb_detect_batch_dev(sgx_kfdb *db, int mode, int Q, const int32_t *ids_dev, const double *weights_dev, int pitch, const int32_t *counts_dev,
                              const int32_t *conn_offsets_dev, const int32_t *conn_ids_dev, const float *min_score_dev,
                              int32_t *cand_dev, int32_t *n_cand_dev, sgx_kfdb_report *report_dev, int32_t *words_dev, float *score_dev, void *stream);

/* ---- Covisibility graph (src/sg-slam/src/KeyFrame.cc, MapPoint.cc, Tracking.cc:1314-1458, LocalMapping.cc:632-696) --------------------------------------------------
 * The handle holds the relation "keyframe k observes map point p at keypoint index i" on the device, and what the reference derives from it: mConnectedKeyFrameWeights,
 * the ordered list, the spanning tree (parent, children, mbFirstConnection), every point's observation list and nObs.  Three walks of it are batched launch sequences:
 * KeyFrame::UpdateConnections (KeyFrame.cc:290-380), Tracking::UpdateLocalKeyFrames + UpdateLocalPoints (Tracking.cc:1324-1458) and the votes of
 * LocalMapping::KeyFrameCulling (LocalMapping.cc:632-696).  Everything is integer; a batch of Q equals Q single calls in order, bit for bit.
 * Kept as written: the gate th = 15 and the fall-back to the single maximum (pKFmax moves on a strictly greater count); mConnectedKeyFrameWeights holds every count >= 1
 * while the ordered list after UpdateConnections holds only the gated entries; an effective AddConnection / EraseConnection rebuilds the ordered list from the whole
 * weight map (UpdateBestCovisibles), an AddConnection with the weight unchanged does nothing: the ordered list is state (a mode per keyframe), not a function of the
 * weights; lists are sorted ascending on (weight, keyframe) and reversed; an empty KFcounter leaves the old connections; the parent is the front of the list at the first
 * connection of a keyframe whose id is not 0; a mvuRight >= 0 observation counts 2 in nObs, EraseObservation at nObs <= 2 is SetBadFlag; stage 2 of
 * UpdateLocalKeyFrames walks only the stage-1 keyframes, tests size() > 80 before each, adds the first unmarked of GetBestCovisibilityKeyFrames(10), the first unmarked
 * child, and for an unmarked parent adds it and leaves the loop; UpdateLocalPoints keeps the first occurrence; culling counts a point only if close (or monocular),
 * redundant = Observations() > 3 and at least 3 other keyframes at octave <= own + 1, vote nRedundantObservations > 0.9 * nMPs in double, id 0 never voted.
 * A point exists exactly while it has an observation; any other id in [0, max_points) behaves as isBad().
 * Defined where the reference is not:
 *   1. containers keyed or tie-broken by KeyFrame* (map, set, sort of pair<int, KeyFrame*>) run in ascending keyframe id.
 *   2. mvpMapPoints and mObservations are one relation: a second index of one keyframe for the same point, or a point for an index that holds another one, is
 *      SGX_ERR_INVALID (erase first, or use replace_point).
 *   3. a frame has no id: it behaves as one whose mnId is fresh and nonzero.
 *   4. an erased keyframe contributes nothing: in a kept local_kf row, as a culling candidate (counts 0, no vote), as mpReferenceKF (ref_tracked 0).  It stays in the
 *      lists of keyframes whose EraseConnection the reference does not call (those absent from its own map), flagged isBad(), as in the reference; its slot returns to
 *      the pool when no list names it any more.  Its id cannot be added again while it is held so.
 *   5. culling votes are taken against the map as it stands; the reference's loop erases between candidates.  The equivalent caller loop: query, erase the first voted
 *      candidate, query again and go on behind it in the candidate list of the FIRST query.
 *   6. ids out of range and negative counts are SGX_ERR_INVALID, in a batch as that query's status with nothing else of it written; an unknown keyframe id in a query
 *      likewise (culling: n_cand = SGX_ERR_INVALID); exhausted capacity is SGX_ERR_NOMEM; a refused mutation leaves the handle unchanged.
 *   7. erase_keyframe of id 0 does nothing (KeyFrame.cc:458); of a keyframe without parent, its unreachable children are left without one.
 *
 * sgx_covis_create: at most 4096 keyframes of at most cap <= 8192 keypoints (SGX_ERR_UNSUPPORTED beyond), point ids in [0, max_points), max_observations live
 *   observations, batches of at most max_queries; monocular = mbMonocular, th_depth = mThDepth.  Device memory: the relation 4 x (3 max_points + 9 chunks + max_keyframes x
 *   cap) bytes with chunks = max_observations / 8 + min(max_points, max_observations) + 1, attributes max_keyframes x cap, weights 2 x max_keyframes^2, workspace
 *   4 x max_queries x (5 max_keyframes + max_points + 888) bytes (sgx_covis_info reports both totals).
 * Mutations: host pointers, synchronous; none may run while a batch of this handle is in flight.  A mutation uploads the words it changes, never the map.
 *   add_keyframe: mnId (>= 0, not present), per keypoint the octave of mvKeysUn (0..31), mvuRight and mvDepth; close = !(depth > th_depth || depth < 0) in float.
 *   set_observations: pairs (idx, point) in order: point >= 0 is AddMapPoint + AddObservation, -1 is EraseMapPointMatch + EraseObservation with its SetBadFlag.
 *   set_points_bad: MapPoint::SetBadFlag.  replace_point: the relation part of MapPoint::Replace(old -> new).  erase_keyframe: KeyFrame::SetBadFlag past its mbNotErase
 *   gate: EraseConnection in every neighbour, EraseObservation of every point, the spanning-tree loop.
 * Getters: host pointers, synchronous.  get_weights: mConnectedKeyFrameWeights in id order; get_ordered: mvpOrderedConnectedKeyFrames / mvOrderedWeights;
 *   best_covisibles: GetBestCovisibilityKeyFrames(N), what sgx_kfdb_set_covisibility takes; get_tree: parent id (-1 none), mbFirstConnection, children in id order;
 *   get_observations: mObservations in keyframe-id order and nObs; get_keyframe_points: mvpMapPoints.  Array capacities: max_keyframes (cap for keyframe_points). */
typedef struct sgx_covis sgx_covis;
typedef struct sgx_covis_report {
    int32_t status;                         /* SGX_OK, SGX_ERR_INVALID (malformed query / unknown keyframe), SGX_ERR_NOMEM (local_map: more than mcap points) */
    int32_t n_counter;                      /* KFcounter.size() / keyframeCounter.size() */
    int32_t max_weight, max_kf;             /* nmax and pKFmax (id, -1 none) */
    int32_t n_ordered;                      /* update_connections: mvpOrderedConnectedKeyFrames.size() */
    int32_t parent;                         /* update_connections: the parent id after the call (-1 none) */
    int32_t n_stage1, n_local_kf, n_local_points, ref_tracked;      /* local_map */
} sgx_covis_report;
int sgx_covis_create(int max_keyframes, int cap, int max_points, int max_observations, int max_queries, int monocular, float th_depth, sgx_covis **out);
void sgx_covis_destroy(sgx_covis *h);
int sgx_covis_size(const sgx_covis *h);                                                                       /* live keyframes */
int sgx_covis_info(const sgx_covis *h, int64_t *device_bytes, int64_t *workspace_bytes, int32_t *n_observations);
int sgx_covis_clear(sgx_covis *h);
int sgx_covis_add_keyframe(sgx_covis *h, int32_t kf_id, int n, const int32_t *octave, const float *uright, const float *depth);
int sgx_covis_set_observations(sgx_covis *h, int32_t kf_id, int n, const int32_t *idx, const int32_t *point_id);
int sgx_covis_set_points_bad(sgx_covis *h, int n, const int32_t *ids);
int sgx_covis_replace_point(sgx_covis *h, int32_t old_id, int32_t new_id);
int sgx_covis_erase_keyframe(sgx_covis *h, int32_t kf_id);
int sgx_covis_get_weights(sgx_covis *h, int32_t kf_id, int32_t *kf_ids, int32_t *weights, int32_t *n);
int sgx_covis_get_ordered(sgx_covis *h, int32_t kf_id, int32_t *kf_ids, int32_t *weights, int32_t *n);
int sgx_covis_best_covisibles(sgx_covis *h, int32_t kf_id, int N, int32_t *kf_ids, int32_t *n);
int sgx_covis_get_tree(sgx_covis *h, int32_t kf_id, int32_t *parent, int32_t *first_connection, int32_t *children, int32_t *n_children);
int sgx_covis_get_observations(const sgx_covis *h, int32_t point_id, int32_t *kf_ids, int32_t *idx, int32_t *n, int32_t *n_obs);
int sgx_covis_get_keyframe_points(const sgx_covis *h, int32_t kf_id, int32_t *point_ids, int32_t *n);
/* The queries: every pointer is device memory, asynchronous on `stream`, one launch sequence for the Q queries, Q <= max_queries.  A handle serves one call at a time.
 * update_connections: KeyFrame::UpdateConnections of keyframe kf_ids_dev[q], q ascending; one report each.
 * local_map: frame q = the first n_dev[q] entries of row q of frame_mp_dev (row pitch cap; point ids, -1 none; in/out: a bad point becomes -1).  local_kf_dev (rows of
 *   max_keyframes ids), n_local_kf_dev and ref_kf_dev are in/out: mvpLocalKeyFrames and mpReferenceKF; when no point votes they stay and the points are rebuilt from the
 *   old list.  ref_tracked_dev = mpReferenceKF->TrackedMapPoints(min_obs_dev[q]).  local_points_dev / local_obs_dev: rows of mcap, mvpLocalMapPoints as ids and their
 *   Observations(); n_local_points_dev is the true count, the first mcap are written, and more than mcap is status SGX_ERR_NOMEM.
 * keyframe_culling: for current keyframe kf_ids_dev[q], cand_dev (rows of max_cand) = GetVectorCovisibleKeyFrames() in order (the first max_cand; n_cand_dev the true
 *   count), and per candidate nRedundantObservations, nMPs and the vote (0 / 1). */
int sgx_covis_update_connections_batch_dev(sgx_covis *h, int Q, const int32_t *kf_ids_dev, sgx_covis_report *report_dev, void *stream);
int sgx_covis_local_map_batch_dev(sgx_covis *h, int Q, int cap, int32_t *frame_mp_dev, const int32_t *n_dev, const int32_t *min_obs_dev, int32_t *local_kf_dev,
                                  int32_t *n_local_kf_dev, int32_t *ref_kf_dev, int32_t *ref_tracked_dev, int mcap, int32_t *local_points_dev, int32_t *local_obs_dev,
                                  int32_t *n_local_points_dev, sgx_covis_report *report_dev, void *stream);
int sgx_covis_keyframe_culling_batch_dev(sgx_covis *h, int Q, const int32_t *kf_ids_dev, int max_cand, int32_t *cand_dev, int32_t *n_cand_dev,
                                         int32_t *n_redundant_dev, int32_t *n_mps_dev, int32_t *cull_dev, void *stream);
/* One query from host memory, synchronous, a batch of one through the entries above (frame_mp, local_kf, n_local_kf and ref_kf in/out; local_kf has max_keyframes
 * entries).  The return value is the query's status: SGX_ERR_INVALID with nothing written, or for local_map SGX_ERR_NOMEM with the first mcap points written. */
int sgx_covis_update_connections(sgx_covis *h, int32_t kf_id, sgx_covis_report *report);
int sgx_covis_local_map(sgx_covis *h, int n, int32_t *frame_mp, int min_obs, int32_t *local_kf, int32_t *n_local_kf, int32_t *ref_kf, int32_t *ref_tracked,
                        int mcap, int32_t *local_points, int32_t *local_obs, int32_t *n_local_points, sgx_covis_report *report);
int sgx_covis_keyframe_culling(sgx_covis *h, int32_t kf_id, int max_cand, int32_t *cand, int32_t *n_cand, int32_t *n_redundant, int32_t *n_mps, int32_t *cull);

/* The bundle-adjustment graph from the relation: the set selection at the top of Optimizer::LocalBundleAdjustment (src/sg-slam/src/Optimizer.cc:453-504) and its edge loop
 * (:572-653), and the same edge loop over the whole map for Optimizer::BundleAdjustment (:49-150), as the index arrays of sgx_ba_problem.  A query of the handle like the
 * three above: device pointers, asynchronous on `stream`, one launch sequence for the Q queries, nothing read back, integers only, two runs byte-identical, a batch of Q
 * equal to Q single calls.  The handle is not changed, and no memory beyond the workspace of sgx_covis_create is used.
 * mode = SGX_COVIS_BA_LOCAL, query q = keyframe kf_ids_dev[q]:
 *   lLocalKeyFrames  = the keyframe, then GetVectorCovisibleKeyFrames() = its ordered list as its mode defines it (state, not a function of the weights), in list order,
 *                      without the entries that are isBad() (erased keyframes a list still names, :461-468).
 *   lLocalMapPoints  = the local keyframes in that order, each one's mvpMapPoints in index order, the first occurrence of every existing point (:472-486): the order of
 *                      UpdateLocalPoints.  point_id_dev (rows of pcap) holds the ids in this order.
 *   lFixedCameras    = every live keyframe that observes a local point and is not a local keyframe (:489-504).
 *   poses            = local keyframes and fixed cameras together in ascending keyframe id (what sgx_ba_problem.poses wants): pose_id_dev (rows of max_keyframes) the ids,
 *                      pose_fixed_dev 0 for a local keyframe, 1 for a fixed camera, 2 for a local keyframe whose id is 0 (:529, :762-768).  The order in which the
 *                      reference first meets a fixed camera decides nothing and is not reported.
 *   edges            = outer loop over the local points in their order, inner loop over the point's mObservations in ascending keyframe id (rule 1), one edge per
 *                      observation: edge_pose_dev the index into the pose row, edge_point_dev the index into the point row, edge_kp_dev the keypoint index in that
 *                      keyframe, edge_attr_dev the handle's attribute byte of that keypoint: the octave in bits 0-4 (SGX_COVIS_ATTR_OCTAVE), SGX_COVIS_ATTR_RIGHT for a
 *                      stereo edge (mvuRight >= 0), SGX_COVIS_ATTR_CLOSE as add_keyframe defined it.  point_edge_begin_dev (rows of pcap + 1): point i's edges are
 *                      [begin[i], begin[i + 1]), and begin[n_points] = n_edges.  An erased keyframe has no observations in the handle (rule 4), so the isBad() test
 *                      of :589 never fires here: every observation of a local point is an edge.
 * mode = SGX_COVIS_BA_GLOBAL (Q must be 1, kf_ids_dev is not read): poses = all live keyframes in ascending id, pose_fixed 2 for id 0 and 0 otherwise, n_fixed_kf = 0;
 *   points = all existing points; edges as above.
 * Defined where the reference is not:
 *   8. the reference walks GetAllMapPoints(), a set<MapPoint*> in pointer order: the points of the global mode run in ascending point id.
 *   9. the marks mnBALocalForKF / mnBAFixedForKF behave as fresh for every query: a query for keyframe 0 is one like any other (the reference initialises the marks to 0
 *      and never runs local bundle adjustment for keyframe 0), and two queries for one keyframe give the same.
 * Defined cases: a dead list entry is marked (:465) but not local, and having no observations it cannot come back as a fixed camera; a keyframe without points and
 *   neighbours gives one pose, no points, no edges and point_edge_begin[0] = 0; keyframe 0 is pose_fixed 2 as a local keyframe (the queried one included) and 1 as a
 *   fixed camera; a point met through several local keyframes keeps the place of its first occurrence; a stereo observation is one edge.
 * Statuses: Q > max_queries, Q != 1 in global mode, an unknown mode or a missing array: SGX_ERR_INVALID for the call.  An unknown or erased keyframe id, a negative pcap or
 *   ecap: SGX_ERR_INVALID as that query's status with nothing else of the query written.  More than pcap points or more than ecap edges: SGX_ERR_NOMEM as the query's
 *   status; the report and the pose rows are whole, the first pcap points are written with point_edge_begin over them (begin[pcap] = the edges of those points), and the
 *   edges of the points i with begin[i + 1] <= ecap, which fit wholly, are written; nothing is written past a row. */
#ifndef SGX_COVIS_ATTR_BITS
#define SGX_COVIS_ATTR_BITS
enum { SGX_COVIS_ATTR_OCTAVE = 31, SGX_COVIS_ATTR_RIGHT = 32, SGX_COVIS_ATTR_CLOSE = 64 };
#endif
enum { SGX_COVIS_BA_LOCAL = 0, SGX_COVIS_BA_GLOBAL = 1 };
typedef struct sgx_covis_ba_report {
    int32_t status;                         /* SGX_OK, SGX_ERR_INVALID, SGX_ERR_NOMEM */
    int32_t n_local_kf, n_fixed_kf;         /* lLocalKeyFrames.size(), lFixedCameras.size() */
    int32_t n_poses, n_points, n_edges;     /* the true counts, also beyond pcap / ecap */
    int32_t n_mono_edges, n_stereo_edges;   /* vpEdgesMono.size(), vpEdgesStereo.size() */
} sgx_covis_ba_report;
int sgx_covis_ba_graph_batch_dev(sgx_covis *h, int Q, int mode, const int32_t *kf_ids_dev, int32_t *pose_id_dev, uint8_t *pose_fixed_dev, int pcap,
                                 int32_t *point_id_dev, int32_t *point_edge_begin_dev, int ecap, int32_t *edge_pose_dev, int32_t *edge_point_dev,
                                 int32_t *edge_kp_dev, uint8_t *edge_attr_dev, sgx_covis_ba_report *report_dev, void *stream);
/* One query from host memory, synchronous (kf_id is not read in global mode).  Written: the first n_poses of the pose rows (capacity max_keyframes), the first
 * min(n_points, pcap) points and one more entry of point_edge_begin, and the edges that fit wholly.  The return value is the query's status. */
int sgx_covis_ba_graph(sgx_covis *h, int mode, int32_t kf_id, int32_t *pose_id, uint8_t *pose_fixed, int pcap, int32_t *point_id, int32_t *point_edge_begin,
                       int ecap, int32_t *edge_pose, int32_t *edge_point, int32_t *edge_kp, uint8_t *edge_attr, sgx_covis_ba_report *report);

/* Loop closing from the relation: the map bookkeeping of LoopClosing::CorrectLoop (src/sg-slam/src/LoopClosing.cc:432-573) and the vertex and edge loops of
 * Optimizer::OptimizeEssentialGraph (Optimizer.cc:797-983) as index arrays.  Integers only, nothing read back inside a sequence, no result depends on which wave
 * finishes first, two runs byte-identical.  The Sim3 arithmetic on these indices is sgx_loop_propagate_sim3 / sgx_eg_flatten / sgx_eg_recover.
 * State: mspLoopEdges.
 *   add_loop_edge(a, b): b into a's set and a into b's (CorrectLoop :572-573 calls both); a set, so the same edge again (either way round) changes nothing.  Host
 *     pointers, synchronous, the two changed words are uploaded.  Capacity max_keyframes pairs: beyond it SGX_ERR_NOMEM with the handle unchanged.  An unknown or erased
 *     id, or a == b: SGX_ERR_INVALID.  get_loop_edges: the partners in ascending id (rule 1; capacity max_keyframes).  sgx_covis_clear drops the edges.
 *   The device memory of the edges and of the three sequences below is not part of sgx_covis_create's: it is allocated by the first of these calls, once,
 *     4 x max_keyframes x (max_keyframes + 29) + 32 bytes; sgx_covis_loop_info reports it (0 before) and the number of edges.  sgx_covis_info is unchanged.
 *  10. erase_keyframe of a keyframe that has a loop edge is refused with SGX_ERR_INVALID and changes nothing: AddLoopEdge sets mbNotErase and SetBadFlag only records
 *      mbToBeErased (KeyFrame.cc:419-424, :454-464).  That gate stays the caller's control flow.
 *  11. a dead list entry (rule 4: an erased keyframe a list or a row still names) is not a group member, not a loop connection and not an edge end: it has no vertex
 *      (Optimizer.cc:812 skips it; the reference would dereference a null vertex).
 * loop_begin(cur): CorrectLoop :432-436 and the marks of :472-516, one launch sequence:
 *   UpdateConnections(cur); the group mvpCurrentConnectedKFs = GetVectorCovisibleKeyFrames() of cur in list order without dead entries, then cur: group_id_dev (capacity
 *   max_keyframes) and group_vertex_dev = each member's index among the live keyframes in ascending id (the pose row of SGX_COVIS_BA_GLOBAL, the vertex row below);
 *   UpdateConnections of every member in ascending id (the :515 call inside the walk of CorrectedSim3, a map<KeyFrame*, ...>: rule 1); the existing points of the group:
 *   point_id_dev = first occurrence over the members in ascending id, then keypoint index order, point_ref_dev = mnCorrectedReference as an index into the group row: the
 *   member of smallest id that holds the point (what the mnCorrectedByKF test of :488 amounts to), also when it stands later in the list.  The first pcap points are
 *   written; more than pcap is SGX_ERR_NOMEM in the report, whose n_group and n_points are the true counts.  cur unknown or erased, pcap < 0, a missing array:
 *   SGX_ERR_INVALID for the call, nothing enqueued.
 * loop_connections(cur, group row): CorrectLoop :546-564, after the caller's fusion (replace_point / set_observations).  For each member in LIST order: prev = its
 *   ordered list as its mode defines it now (an earlier member's UpdateConnections may have rebuilt it through AddConnection); UpdateConnections of the member;
 *   LoopConnections[member] = the keys of its weight row, minus prev, minus the group, minus dead keys (rule 11: also those of an old row an empty KFcounter left in
 *   place).  Output: CSR over the members in ascending id (the map's order) with the targets of each in ascending id (the set's order): lc_begin_dev (n_group + 1, always
 *   whole) and lc_j_dev (keyframe ids, capacity lcap).  More than lcap: SGX_ERR_NOMEM in the report (n_connections the true count), and only the rows that fit wholly
 *   (lc_begin[r + 1] <= lcap) are written.  The group row is an input: an id that is no live keyframe, an id twice, or a last entry other than cur is SGX_ERR_INVALID in
 *   the report with nothing written and the handle unchanged.  n_group outside [1, live keyframes], lcap < 0, a missing array: SGX_ERR_INVALID for the call.
 * essential_graph(cur, loop, group row, CSR): a query, the handle is not changed.
 *   vertices: vertex_id_dev = all live keyframes in ascending id, vertex_fixed_dev = 1 for loop, vertex_group_dev = the index into the group row or -1 (rows of
 *     max_keyframes).  A vertex of the group starts from its corrected Sim3, any other from its pose.
 *   edges in the reference's insertion order, e_i = vertex 0 (the keyframe whose loop it is), e_j = vertex 1, as vertex indices, e_kind:
 *     0 loop connections (:852-880): CSR order; an entry is kept if (i == cur && j == loop) || i->GetWeight(j) >= 100, the weight read from i's OWN row (rows are not
 *       symmetric: UpdateConnections writes only gated entries into the neighbour).  Only kept edges enter sInsertedEdges.  Both operands of the measurement are vScw.
 *     then per vertex in ascending id (for kinds 1-3 an operand of the measurement is NonCorrectedSim3 for a group vertex, vScw otherwise):
 *     1 the spanning-tree edge to the parent, also when the pair is in sInsertedEdges;
 *     2 the keyframe's loop edges of smaller id, in ascending id;
 *     3 GetCovisiblesByWeight(100) in list order, as written (KeyFrame.cc:185-200): upper_bound finds the first list entry below 100; if there is none (an empty list, or
 *       every entry >= 100) the result is EMPTY, so a gated list whose entries all reach 100 contributes no covisibility edge while the same row in mode "all" with one
 *       weak entry contributes all the strong ones (the list is state).  Dropped: the parent, a child, a loop edge, a dead entry, an entry of larger-or-equal id, a pair
 *       in sInsertedEdges.
 *   The first ecap edges are written; more is SGX_ERR_NOMEM in the report, which holds the true n_vertices, n_edges and the count per kind.
 *   lc_j_dev has capacity lcap.  SGX_ERR_INVALID in the report, nothing else written: a group row refused as above; lc_begin not starting at 0, descending or beyond lcap;
 *   a target that is no live keyframe; a row whose targets are not strictly ascending.  cur or loop unknown or erased, ecap < 0, a missing array: SGX_ERR_INVALID for
 *   the call. */
typedef struct sgx_covis_loop_report {
    int32_t status;                         /* SGX_OK, SGX_ERR_INVALID, SGX_ERR_NOMEM */
    int32_t n_group, n_points;              /* loop_begin: the true counts */
    int32_t n_connections;                  /* loop_connections: the true count; essential_graph: lc_begin[n_group] */
    int32_t n_vertices, n_edges;            /* essential_graph: the true counts */
    int32_t n_kind[4];                      /* essential_graph: edges per kind */
} sgx_covis_loop_report;
int sgx_covis_add_loop_edge(sgx_covis *h, int32_t kf_a, int32_t kf_b);
int sgx_covis_get_loop_edges(const sgx_covis *h, int32_t kf_id, int32_t *kf_ids, int32_t *n);
int sgx_covis_loop_info(const sgx_covis *h, int64_t *loop_bytes, int32_t *n_loop_edges);
/* device pointers, asynchronous on `stream`; a handle serves one call at a time */
int sgx_covis_loop_begin_dev(sgx_covis *h, int32_t cur, int32_t *group_id_dev, int32_t *group_vertex_dev, int pcap, int32_t *point_id_dev, int32_t *point_ref_dev,
                             sgx_covis_loop_report *report_dev, void *stream);
int sgx_covis_loop_connections_dev(sgx_covis *h, int32_t cur, int n_group, const int32_t *group_id_dev, int lcap, int32_t *lc_begin_dev, int32_t *lc_j_dev,
                                   sgx_covis_loop_report *report_dev, void *stream);
int sgx_covis_essential_graph_dev(sgx_covis *h, int32_t cur, int32_t loop, int n_group, const int32_t *group_id_dev, int lcap, const int32_t *lc_begin_dev,
                                  const int32_t *lc_j_dev, int32_t *vertex_id_dev, uint8_t *vertex_fixed_dev, int32_t *vertex_group_dev, int ecap, int32_t *e_i_dev,
                                  int32_t *e_j_dev, uint8_t *e_kind_dev, sgx_covis_loop_report *report_dev, void *stream);
/* the same from host memory, synchronous; the return value is the report's status.  Written: the first n_group entries of the group rows (capacity max_keyframes) and
 * the first min(n_points, pcap) points; lc_begin whole and the rows of lc_j that fit; the first n_vertices of the vertex rows (capacity max_keyframes) and the first
 * min(n_edges, ecap) edges.  essential_graph takes lcap = lc_begin[n_group]. */
int sgx_covis_loop_begin(sgx_covis *h, int32_t cur, int32_t *group_id, int32_t *group_vertex, int pcap, int32_t *point_id, int32_t *point_ref, sgx_covis_loop_report *report);
int sgx_covis_loop_connections(sgx_covis *h, int32_t cur, int n_group, const int32_t *group_id, int lcap, int32_t *lc_begin, int32_t *lc_j, sgx_covis_loop_report *report);
int sgx_covis_essential_graph(sgx_covis *h, int32_t cur, int32_t loop, int n_group, const int32_t *group_id, const int32_t *lc_begin, const int32_t *lc_j,
                              int32_t *vertex_id, uint8_t *vertex_fixed, int32_t *vertex_group, int ecap, int32_t *e_i, int32_t *e_j, uint8_t *e_kind,
                              sgx_covis_loop_report *report);

/* LoopClosing::DetectLoop's covisibility consistency (src/sg-slam/src/LoopClosing.cc:152-225) with mvConsistentGroups as device state of the handle, and
 * KeyFrame::GetConnectedKeyFrames of a batch of keyframes.  Integers only, one launch sequence without a read-back, no result depends on which wave finishes first, two
 * runs byte-identical.
 * State: mvConsistentGroups, a list of (set of keyframe ids, counter) in the reference's order.  It is not part of sgx_covis_create's totals: it is allocated by
 *   sgx_covis_consistency_reserve(max_groups), or with max_groups = SGX_COVIS_DEFAULT_GROUPS by the first consistency call that finds none; the capacity stays until
 *   sgx_covis_clear (a second reserve with the same value does nothing, with another one it is SGX_ERR_INVALID; max_groups < 1: SGX_ERR_INVALID, > 4096:
 *   SGX_ERR_UNSUPPORTED).  Device memory: max_groups x (9 max_keyframes + 24) + 8 max_keyframes + 32 bytes (two halves of max_groups rows of max_keyframes ids, the
 *   candidates x groups flag bytes, the descriptors).  sgx_covis_consistency_info reports the bytes (0 before), the number of groups and the capacity (0 before);
 *   sgx_covis_info is unchanged.  sgx_covis_clear releases the memory; sgx_covis_consistency_clear drops the groups only.
 * consistency(candidates, th): the candidates are vpCandidateKFs as keyframe ids in their order, with their number in device memory (what sgx_kfdb_detect_batch_dev
 *   writes for one query: no read-back sits between the two calls); th = mnCovisibilityConsistencyTh (3).  As written in the reference: a candidate's group is the
 *   candidate and every keyframe with a count >= 1 in its weight row (GetConnectedKeyFrames, not the gated list); the previous groups are visited in stored order; a
 *   candidate consistent with previous group iG (they share a keyframe) that is not marked yet pushes ITS OWN group with counter previous + 1 and marks iG, so a
 *   candidate consistent with two unmarked groups pushes its group twice with the two counters, and a later candidate consistent only with marked groups pushes nothing
 *   (and is not pushed with 0 either); the test counter >= th is made for every consistent iG, marked or not, and enters the candidate into enough_dev (capacity
 *   max_keyframes; mvpEnoughConsistentCandidates as ids in candidate order) at most once; a candidate consistent with no group pushes (group, 0); the new list, in
 *   candidate order then iG order, replaces the old one.  No candidate (*n_cand_dev == 0) clears the groups (:147) and returns no enough-candidate.
 *  12. a set of KeyFrame* is a set of keyframe ids.  A dead entry of a weight row (rule 4) is no member of a candidate's group, the choice of rule 11.  A stored group
 *      keeps the id of a keyframe erased since (get_consistent_groups shows it) but never matches through it, and not through the keyframe that reuses its slot.
 *      Keyframe ids are never reused by the caller (mnId is not): an erased id added again later would match the stored groups that still name it.
 *  13. a candidate id the handle does not hold (unknown or erased), the same candidate twice, or a count outside [0, max_keyframes]: SGX_ERR_INVALID in the report;
 *      more than max_groups resulting groups: SGX_ERR_NOMEM in the report.  In either case the stored groups, enough_dev and n_enough_dev are untouched.
 *   A missing array is SGX_ERR_INVALID for the call, nothing enqueued.
 * get_consistent_groups: host pointers, synchronous.  *n_groups, counter (capacity max_groups), and the members as a CSR: off (capacity max_groups + 1, whole) and ids
 *   (capacity cap) ascending within a group; SGX_ERR_NOMEM when cap is short, with the leading groups that fit wholly written.
 * connected_batch(Q keyframes): GetConnectedKeyFrames() of each, without dead entries (rule 12), as a CSR of ascending ids: off_dev (Q + 1, always whole; off[Q] is the
 *   need) and ids_dev (capacity cap): the conn_offsets / conn_ids layout sgx_kfdb_detect_batch_dev takes.  One sgx_covis_report per query: status and n_counter = its
 *   number of connected keyframes.  A row is written only if it fits wholly (off[q + 1] <= cap); otherwise that query's status is SGX_ERR_NOMEM and nothing of it is
 *   written.  An unknown or erased keyframe: SGX_ERR_INVALID as that query's status and an empty row.  Q > max_queries, cap < 0, a missing array: SGX_ERR_INVALID for the
 *   call.  The handle is not changed and no memory beyond the workspace of sgx_covis_create is used. */
enum { SGX_COVIS_DEFAULT_GROUPS = 64 };
typedef struct sgx_covis_consistency_report {
    int32_t status;                         /* SGX_OK, SGX_ERR_INVALID, SGX_ERR_NOMEM */
    int32_t n_before, n_after;              /* mvConsistentGroups.size() going in and coming out */
    int32_t n_consistent;                   /* candidates consistent with some previous group */
    int32_t n_pushed_zero;                  /* groups pushed with counter 0 */
    int32_t n_pushed_nothing;               /* candidates that pushed nothing: every group they are consistent with was taken */
    int32_t n_enough, n_cand;               /* mvpEnoughConsistentCandidates.size(); the candidates read */
} sgx_covis_consistency_report;
int sgx_covis_consistency_reserve(sgx_covis *h, int max_groups);
int sgx_covis_consistency_clear(sgx_covis *h);
int sgx_covis_consistency_info(const sgx_covis *h, int64_t *bytes, int32_t *n_groups, int32_t *max_groups);
int sgx_covis_get_consistent_groups(const sgx_covis *h, int32_t *n_groups, int32_t *counter, int32_t *off, int cap, int32_t *ids);
/* device pointers, asynchronous on `stream`; a handle serves one call at a time */
int sgx_covis_consistency_dev(sgx_covis *h, const int32_t *cand_dev, const int32_t *n_cand_dev, int th, int32_t *enough_dev, int32_t *n_enough_dev,
                              sgx_covis_consistency_report *report_dev, void *stream);
int sgx_covis_connected_batch_dev(sgx_covis *h, int Q, const int32_t *kf_ids_dev, int32_t *off_dev, int32_t *ids_dev, int cap, sgx_covis_report *report_dev, void *stream);
/* the same from host memory, synchronous.  consistency: the return value is the report's status; enough (capacity n_cand) and *n_enough are written on SGX_OK only.
 * connected_batch (Q >= 1): off whole, the rows of the queries whose status is SGX_OK; the return value is the first query status that is not SGX_OK. */
int sgx_covis_consistency(sgx_covis *h, int n_cand, const int32_t *cand, int th, int32_t *enough, int32_t *n_enough, sgx_covis_consistency_report *report);
int sgx_covis_connected_batch(sgx_covis *h, int Q, const int32_t *kf_ids, int32_t *off, int32_t *ids, int cap, sgx_covis_report *report);

/* The map update of LoopClosing::RunGlobalBundleAdjustment (src/sg-slam/src/LoopClosing.cc:676-737) after Optimizer::GlobalBundleAdjustemnt(nLoopKF), over the spanning
 * tree the handle keeps.  One launch sequence, no read-back, no result depends on which wave finishes first, two runs byte-identical.
 * gba_update: the table lists every live keyframe exactly once (nk rows: kf_ids, in_gba = mnBAGlobalForKF == nLoopKF on entry, Tcw = the pose, 3 x 4 float per row as
 *   sgx_loop_propagate_sim3 takes it, TcwGBA = mTcwGBA, read only where in_gba is set); sgx_covis_ba_graph's global pose order is a natural choice.  The BFS of :676-700
 *   from the origins (mvpKeyFrameOrigins) over the tree: a child that is not in_gba gets mTcwGBA = (Tcw_child * Twc_parent) * mTcwGBA_parent, both factors of the first
 *   product being the OLD poses (:683 and :689 read before :698 writes), and is marked; every visited keyframe gets TcwBef = its old pose and Tcw_out = mTcwGBA.
 *   kf_state: bit 0 = visited, bit 1 = mnBAGlobalForKF == nLoopKF afterwards.  Tcw_out must not be Tcw.
 *   Arithmetic: float cv::Mat arithmetic as the Sim3 propagation states it: a product entry is a float dot product summed left to right, through double with alpha;
 *   KeyFrame::SetPose gives Twc = [Rcw.t() | -Rwc * tcw] (alpha = -1); R * x + t is one gemm (the double of the dot product plus the double of t, rounded once).  The
 *   unit is built without multiply-add fusion.  OpenCV is not pinned; the yardstick is the restatement of tests/loopclose_ref.py, bit for bit.
 *  14. an origin that is not in_gba: status SGX_COVIS_GBA_ORIGIN_NOT_IN_GBA and nothing is written (the reference multiplies by a stale mTcwGBA).
 *      An origin below another origin: the reference's queue would visit that subtree twice and overwrite mTcwBefGBA with the corrected pose on the second visit;
 *      here every keyframe is visited once, TcwBef is the pose before the call, and a keyframe's level is counted up to the FIRST origin on its way up.
 *  15. a live keyframe no origin reaches is not visited: its pose is copied through to Tcw_out, its TcwBef row is not written, it keeps bit 1 if it was in_gba; its
 *      points are corrected only if it was visited (the reference reads a stale mTcwBefGBA there).  The report counts these keyframes.
 *   SGX_ERR_INVALID in the report, nothing written: nk other than the number of live keyframes, an id that is no live keyframe or stands twice, an origin that is no
 *   live keyframe.  A missing array, n_origins or nk outside [1, max_keyframes], Tcw_out == Tcw: SGX_ERR_INVALID for the call.  Device memory: 16 max_keyframes + 32
 *   bytes, allocated by the first call, released with the handle.
 * correct_points (:705-736): a point in the GBA (in_gba[i]) takes xw_gba; any other takes Rwc * (Rcw_bef * Xw + tcw_bef) + twc of its reference keyframe ref[i] (a row
 *   of the table, -1 none; the caller supplies it, as for the loop correction, and the _dev form trusts it) if that keyframe's state is 3, and stays as it was
 *   otherwise.  Bad points are the caller's to leave out.  One lane per point, memory-bound. */
enum { SGX_COVIS_GBA_ORIGIN_NOT_IN_GBA = 1 };
typedef struct sgx_covis_gba_report {
    int32_t status;                         /* SGX_OK, SGX_ERR_INVALID, SGX_COVIS_GBA_ORIGIN_NOT_IN_GBA */
    int32_t n_visited, n_propagated;        /* keyframes the BFS visited; of these, not in the GBA */
    int32_t n_unreached;                    /* rule 15 */
    int32_t max_depth;                      /* the longest chain of keyframes outside the GBA below an optimised one */
    int32_t pad[3];
} sgx_covis_gba_report;
int sgx_covis_gba_update_dev(sgx_covis *h, int n_origins, const int32_t *origins_dev, int nk, const int32_t *kf_ids_dev, const uint8_t *in_gba_dev, const float *Tcw_dev,
                             const float *TcwGBA_dev, float *Tcw_out_dev, float *TcwBef_dev, uint8_t *kf_state_dev, sgx_covis_gba_report *report_dev, void *stream);
int sgx_gba_correct_points_dev(int n, const float *xw_dev, const uint8_t *in_gba_dev, const float *xw_gba_dev, const int32_t *ref_dev, const uint8_t *kf_state_dev,
                               const float *TcwBef_dev, const float *Tcw_out_dev, float *xw_out_dev, void *stream);
/* the same from host memory, synchronous; the return value is the report's status, and nothing is written unless it is SGX_OK (TcwBef is in/out) */
int sgx_covis_gba_update(sgx_covis *h, int n_origins, const int32_t *origins, int nk, const int32_t *kf_ids, const uint8_t *in_gba, const float *Tcw, const float *TcwGBA,
                         float *Tcw_out, float *TcwBef, uint8_t *kf_state, sgx_covis_gba_report *report);
/* the point loop from host memory through sgx_gba_correct_points_dev, synchronous; nk = the rows of the keyframe table: a ref outside [-1, nk) is SGX_ERR_INVALID */
int sgx_gba_correct_points(int n, const float *xw, const uint8_t *in_gba, const float *xw_gba, const int32_t *ref, int nk, const uint8_t *kf_state, const float *TcwBef,
                           const float *Tcw_out, float *xw_out);

/* ---- Keyframe store and LocalMapping::CreateNewMapPoints (src/sg-slam/src/LocalMapping.cc:207-452, :536-553) ------------------------------------------------------------
 * sgx_kfstore holds what LocalMapping reads of a keyframe on the device: mvKeysUn, mvKeys, the descriptors, mvuRight, mvDepth, the pose and the features grouped by
 * vocabulary node in FeatureVector order (ascending node, ascending feature index inside a node, feat_node < 0 left out).  One sensor and one ORB pyramid for all
 * keyframes.  The relation keyframe x map point stays in sgx_covis: the queries below take mvpMapPoints rows (point ids, -1 none: sgx_covis_get_keyframe_points).
 * sgx_kfstore_create: at most 4096 keyframes of at most cap <= 8192 keypoints (SGX_ERR_UNSUPPORTED beyond); nlevels in [2, 12] (ratioFactor reads level 1).  Device
 *   memory: max_keyframes x (cap x 108 + 64) bytes, allocated at create; the batched call adds a workspace of 26 x cap bytes per query of the largest batch seen
 *   (sgx_kfstore_info reports the total and, of it, the workspace).
 * Mutations: host pointers, synchronous, none while a batch of this handle is in flight.  Error conventions as rule 6 of the covisibility section: a refused mutation
 *   leaves the handle unchanged.  add uploads this keyframe only; keys may be NULL (= keys_un; UnprojectStereo reads mvKeys); Tcw is 3 x 4 row-major (12 floats read).
 *   SGX_ERR_INVALID: a negative or known id, n outside [0, cap], an octave of keys_un outside [0, nlevels), a missing array; SGX_ERR_NOMEM: a full store.
 *   set_pose / erase of an unknown id: SGX_ERR_INVALID.  erase gives the slot back; clear drops every keyframe.
 * A failed create clears *out and returns the status that occurred: SGX_ERR_NOMEM for a refused allocation, SGX_ERR_DEVICE for a failed copy.
 *
 * sgx_create_new_map_points_batch_dev: every pointer is device memory, asynchronous on `stream`, one launch for the Q queries, nothing read back, two runs byte-identical,
 *   a batch of Q equal to Q single calls.  A handle serves one call at a time.  Query q: the current keyframe cur_ids_dev[q]; its neighbours nb_ids_dev[nb_offsets_dev[q] ..
 *   nb_offsets_dev[q + 1]) in the order of GetBestCovisibilityKeyFrames(nn); first_new_id_dev[q]; median_depth_dev (optional, one entry per neighbour, aligned with
 *   nb_ids_dev): NULL selects the stereo / RGB-D gate baseline < mb (:249-253), given it selects the monocular gate baseline / median < 0.01 (:254-261).
 *   mp_rows_dev (in/out, pitch cap): query q owns rows q + nb_offsets_dev[q] (the current keyframe) .. q + nb_offsets_dev[q + 1] (its neighbours, in order).
 *   Per neighbour, in order: the camera centres, the baseline and its gate; ComputeF12; the epipole (ORBmatcher.cc:666-674); the join of the two stored node lists;
 *   SearchForTriangulation(cur, kf2, F12, pairs, false) without the orientation check (ORBmatcher(0.6, false)), has_mp = row[i] >= 0; the per-pair body :286-431; the
 *   commit :433-447 in ascending idx1: the k-th accepted pair of the QUERY writes first_new_id + k into both rows and appends its record, and the next neighbour's search
 *   sees the updated row of the current keyframe.
 *   Outputs, rows of pitch cap per query, the first n_new_dev[q] entries written: new_kf2 / new_idx1 / new_idx2, new_x3d (x3), and the two MapPoint post-steps the
 *   reference runs at once (:442-444) over the point's two observations in ascending keyframe id (rule 1): new_desc (x32 bytes, ComputeDistinctiveDescriptors; 4-byte
 *   aligned) and new_normal (x3) / new_min_dist / new_max_dist (UpdateNormalAndDepth, mpRefKF = the current keyframe, level = kp1.octave).  At most n_cur <= cap points can
 *   be created, because every accepted pair fills a free keypoint of the current keyframe: the rows cannot overflow and there is no capacity status.
 *   report_dev: one record per neighbour (aligned with nb_ids_dev), always written whole; fields that were not computed are 0.  pair_idx1_dev / pair_idx2_dev / pair_ok_dev
 *   (each optional, one row of pitch cap per neighbour): vMatchedIndices and which pairs survived, the first n_pairs entries written.
 *   Arithmetic: Ow1 / Ow2 of the report are GetCameraCenter(), Ow = -Rwc * tcw with Rwc stored (float products left to right, alpha = -1 last); they serve the baseline,
 *   the epipole and UpdateNormalAndDepth.  The per-pair body forms its centres as sgx_triangulate_new_map_points does (-Rcw.t() * tcw as one product, double
 *   accumulation), so that it equals that entry bit for bit.  cv::norm accumulates in double.  F12 = K1.t().inv() * t12x * R12 * K2.inv(): products with a transposed
 *   operand (R1w * R2w.t(), -R1w * R2w.t()) accumulate in double, the others are float products left to right; A * B + C is one gemm; inv() is OpenCV's closed 3 x 3 form
 *   with determinant and cofactors in double, and inv() * M is the inverse times M.
 *   Statuses of a neighbour: SGX_NEWPOINTS_PROCESSED, SGX_NEWPOINTS_SKIPPED (the gate), SGX_ERR_INVALID (the neighbour or the current keyframe is not in the store, or
 *   they are the same keyframe): that neighbour contributes nothing and the others are unaffected.  Q == 0: SGX_OK, nothing enqueued.  Q < 0 or a missing array:
 *   SGX_ERR_INVALID for the call, nothing enqueued.
 * sgx_create_new_map_points: one query from host memory, synchronous, a batch of one through the entry above; mp_rows holds n_nb + 1 rows of cap, report n_nb records,
 *   the new_* arrays cap entries, the pair arrays n_nb rows of cap. */
#define SGX_NEWPOINTS_PROCESSED 0
#define SGX_NEWPOINTS_SKIPPED 1
typedef struct sgx_kfstore sgx_kfstore;
typedef struct sgx_newpoints_report {
    int32_t status;                         /* SGX_NEWPOINTS_PROCESSED, SGX_NEWPOINTS_SKIPPED, SGX_ERR_INVALID */
    int32_t kf2;                            /* the neighbour's id as given */
    int32_t n_pairs, n_new;                 /* vMatchedIndices.size() and the points created with this neighbour */
    float baseline;
    float F12[9];                           /* row-major */
    float Ow1[3], Ow2[3];                   /* GetCameraCenter() of the current keyframe and of the neighbour */
} sgx_newpoints_report;
int sgx_kfstore_create(int max_keyframes, int cap, const sgx_camera *cam, const float *scale_factors, const float *level_sigma2, int nlevels, sgx_kfstore **out);
void sgx_kfstore_destroy(sgx_kfstore *h);
int sgx_kfstore_size(const sgx_kfstore *h);                                                                    /* keyframes held */
int sgx_kfstore_info(const sgx_kfstore *h, int64_t *device_bytes, int64_t *workspace_bytes);
int sgx_kfstore_clear(sgx_kfstore *h);
int sgx_kfstore_add(sgx_kfstore *h, int32_t kf_id, int n, const sgx_keypoint *keys_un, const sgx_keypoint *keys, const uint8_t *desc, const float *uright,
                    const float *depth, const int32_t *feat_node, const float *Tcw);
int sgx_kfstore_set_pose(sgx_kfstore *h, int32_t kf_id, const float *Tcw);
int sgx_kfstore_erase(sgx_kfstore *h, int32_t kf_id);
int sgx_create_new_map_points_batch_dev(
    sgx_kfstore *h, int Q, const int32_t *cur_ids_dev, const int32_t *nb_offsets_dev, const int32_t *nb_ids_dev, const int32_t *first_new_id_dev, const float *median_depth_dev,
    int32_t *mp_rows_dev, int32_t *n_new_dev, int32_t *new_kf2_dev, int32_t *new_idx1_dev, int32_t *new_idx2_dev, float *new_x3d_dev, uint8_t *new_desc_dev,
    float *new_normal_dev, float *new_min_dist_dev, float *new_max_dist_dev, sgx_newpoints_report *report_dev,
    int32_t *pair_idx1_dev, int32_t *pair_idx2_dev, uint8_t *pair_ok_dev, void *stream);
int sgx_create_new_map_points(
    sgx_kfstore *h, int32_t cur_id, int n_nb, const int32_t *nb_ids, int32_t first_new_id, const float *median_depth, int32_t *mp_rows,
    int32_t *n_new, int32_t *new_kf2, int32_t *new_idx1, int32_t *new_idx2, float *new_x3d, uint8_t *new_desc, float *new_normal, float *new_min_dist, float *new_max_dist,
    sgx_newpoints_report *report, int32_t *pair_idx1, int32_t *pair_idx2, uint8_t *pair_ok);

/* The colour conversion at the top of Tracking::GrabImageRGBD (src/sg-slam/src/Tracking.cc:214-227): cvtColor(CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY) on
 * 8-bit images, OpenCV's fixed point (R*4899 + G*9617 + B*1868 + 8192) >> 14.  blue_first = !mbRGB.  Pitches in bytes, multiples of 4; pointers 4-byte aligned. */
int sgx_frame_gray_from_color_batch_dev(int batch, int width, int height, const uint8_t *d_src, int src_pitch, int channels, int blue_first,
                                        uint8_t *d_gray, int gray_pitch, void *stream);
/* ---- per-frame glue between the accelerated stages (device resident) -----------------------------
 * Frame::ComputeStereoFromRGBD (Frame.cc:893-914) fused with the u16 -> metres conversion
 * (Tracking.cc:229-230): uright[i] = x - bf/d, zdepth[i] = d, or -1 when depth is 0. */
int sgx_frame_stereo_from_rgbd_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n,
                                         const uint16_t *d_depth, int width, int height, float depth_map_factor,
                                         float bf, float *d_uright, float *d_zdepth, void *stream);
/* ---- lens distortion (Frame::UndistortKeyPoints, Frame.cc:654-684; Frame::ComputeImageBounds, :686-714; mDistCoef, Tracking.cc:66-77) -----------------
 * dist = k1, k2, p1, p2 [, k3 [, k4, k5, k6]] (ndist 4, 5 or 8, else SGX_ERR_INVALID); K4 = fx, fy, cx, cy.  The undistortion restates OpenCV 3.4's
 * cv::undistortPoints(src, dst, K, D, noArray(), K): five fixed-point iterations in fp64, the icdist < 0 guard, float outputs.
 * sgx_undistort_points: n host points (x, y pairs), computed on the device, synchronous; no k1 == 0 shortcut (cv::undistortPoints always iterates). */
int sgx_undistort_points(int n, const float *pts, const float *K4, const float *dist, int ndist, float *out);
/* Frame::UndistortKeyPoints fused with Frame::ComputeStereoFromRGBD: d_keys_un = d_keys with pt undistorted (the other 20 bytes of each record, and rows
 * n..cap-1, are copies), depth read at the distorted pixel, uright = x_un - bf/d; uright / zdepth as sgx_frame_stereo_from_rgbd_batch_dev otherwise.
 * K and bf come from *cam.  dist[0] == 0 is the reference's early-out (Frame.cc:656-660): d_keys_un is a byte copy of d_keys whatever p1, p2, k3 are. */
int sgx_frame_undistort_stereo_rgbd_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n, const float *dist, int ndist,
                                              const sgx_camera *cam, const uint16_t *d_depth, int width, int height, float depth_map_factor,
                                              sgx_keypoint *d_keys_un, float *d_uright, float *d_zdepth, void *stream);
/* Frame::ComputeImageBounds: cam->min_x..max_y from the undistorted image corners (0, cols, 0, rows when dist[0] == 0); the other fields are left alone */
int sgx_frame_image_bounds(int width, int height, const float *K4, const float *dist, int ndist, sgx_camera *cam);

/* Frame::UnprojectStereo (Frame.cc:916-930) for every keypoint: xw = Rwc*x3Dc + Ow, has = depth>0 */
int sgx_frame_unproject_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n, const float *d_zdepth,
                                  const float *d_Tcw, const sgx_camera *cam, float *d_xw, uint8_t *d_has, void *stream);

/* Tracking's constant-velocity prediction (Tracking.cc:463-470, :914): pred = Tcur * inv(Tprev) * Tcur;
 * frames with valid[f]==0 (optional array) copy Tcur. */
int sgx_frame_motion_model_batch_dev(int batch, const float *d_Tcw_cur, const float *d_Tcw_prev, const uint8_t *d_valid,
                                     float *d_Tcw_pred, void *stream);

/* MapPoint::MapPoint(Pos, pMap, pFrame, idxF) (src/sg-slam/src/MapPoint.cc:45-67) for every keypoint with depth — the temporal points of
 * Tracking::UpdateLastFrame (Tracking.cc:840-904): normal, mfMin/MaxDistance, descriptor; written to slice `half` (0/1) of a
 * per-frame ring of 2*cap local-map records (the layout sgx_match_project_local_batch_dev consumes with mcap = 2*cap). */
int sgx_frame_make_map_points_batch_dev(int batch, int cap, int half, const sgx_keypoint *d_keys, const int32_t *d_n, const float *d_xw, const uint8_t *d_has,
                                        const uint8_t *d_desc, const float *d_Tcw, const float *scale_factors, int nlevels,
                                        float *d_m_xw, float *d_m_normal, float *d_m_min_dist, float *d_m_max_dist, uint8_t *d_m_desc, uint8_t *d_m_skip, void *stream);
/* mvpMapPoints after TrackWithMotionModel (+ SearchLocalPoints): merged[k] indexes the combined table xw_all = [last frame's points (cap) |
 * local-map ring (2*cap)]; motion-model outliers are dropped (Tracking.cc:941-956); a local-map match replaces an unobserved point.
 * cur_mp_obs[k] (optional out) = 0 for keypoints holding a visual-odometry point, -1 otherwise (input of the local-map matcher).
 * d_match_local / d_merged / d_xw_all may be NULL (first call of a frame only needs cur_mp_obs). */
int sgx_frame_merge_matches_batch_dev(int batch, int cap, const int32_t *d_n, const int32_t *d_match_last, const uint8_t *d_outlier_last, const int32_t *d_match_local,
                                      const float *d_xw_last, const float *d_m_xw, int32_t *d_merged, int32_t *d_cur_mp_obs, float *d_xw_all, void *stream);

/* ---- pose-only optimisation -------------------------------------------------------------------
 * Replaces `static int Optimizer::PoseOptimization(Frame *pFrame)` (src/sg-slam/include/Optimizer.h:50,
 * src/sg-slam/src/Optimizer.cc:239-451): g2o Levenberg-Marquardt over the frame pose with one
 * mono (mvuRight<0) or stereo reprojection edge per keypoint that holds a map point, Huber kernel,
 * 4 rounds x 10 iterations with chi2 inlier classification between rounds.  fp64 inside, fp32 at the
 * boundary exactly like the reference (Converter.cc:37-71).
 * Flattened Frame: keys_un = mvKeysUn, uright = mvuRight, inv_level_sigma2 = mvInvLevelSigma2;
 * mvpMapPoints[i] is given either per keypoint (has_mp[i], mp_xw[3*i..]) or through mp_index[i]
 * (row of mp_xw, -1 = NULL) so the matcher's output can be consumed without a gather.
 * In/out: Tcw (4x4 row-major float, pFrame->mTcw).  Out: outlier = mvbOutlier, return value in
 * n_inliers (nInitialCorrespondences - nBad; 0 when fewer than 3 correspondences). */
int sgx_pose_optimization_batch_dev(int batch, int cap, const sgx_keypoint *d_keys_un, const float *d_uright, const int32_t *d_n,
                                    const int32_t *d_mp_index, const uint8_t *d_has_mp, const float *d_mp_xw, int xw_pitch,
                                    const float *inv_level_sigma2, int nlevels, const sgx_camera *cam,
                                    float *d_Tcw, uint8_t *d_outlier, int32_t *d_n_inliers, void *stream);
int sgx_pose_optimization(int n, const sgx_keypoint *keys_un, const float *uright, const uint8_t *has_mp, const float *mp_xw,
                          const float *inv_level_sigma2, int nlevels, const sgx_camera *cam,
                          float *Tcw, uint8_t *outlier, int32_t *n_inliers);

/* ---- local bundle adjustment -------------------------------------------------------------------
 * Replaces `static void Optimizer::LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap)`
 * (src/sg-slam/include/Optimizer.h:52, src/sg-slam/src/Optimizer.cc:453-778) from the point where the local
 * graph is known: the caller flattens lLocalKeyFrames + lFixedCameras into `poses` (KeyFrame::mnId order, as g2o
 * orders vertices), lLocalMapPoints into `points`, and the observation edges in insertion order (outer loop over
 * points, Optimizer.cc:572-653).  optimize(5) with Huber -> chi2/depth classification -> optimize(10) without the
 * outliers -> per-edge erase flags (the (KeyFrame, MapPoint) pairs of vToErase, :709-757).  fp64 inside.
 * pose_fixed: 0 = local keyframe (optimised), 1 = fixed camera (lFixedCameras, never rewritten),
 *             2 = local keyframe with mnId==0 (fixed vertex, still rewritten through SE3Quat like :762-768).
 * edge_obs: (u, v, uR) per edge, uR < 0 => monocular edge.  stop_flag mirrors pbStopFlag (polled between trials). */
typedef struct sgx_ba_problem {
    int32_t n_poses, n_points, n_edges;
    float *poses;                 /* n_poses x 16 (Tcw row-major), in/out */
    const uint8_t *pose_fixed;    /* n_poses */
    float *points;                /* n_points x 3, in/out */
    const int32_t *edge_pose;     /* n_edges */
    const int32_t *edge_point;    /* n_edges */
    const float *edge_obs;        /* n_edges x 3 */
    const float *edge_info;       /* n_edges: mvInvLevelSigma2[octave] */
} sgx_ba_problem;
typedef struct sgx_ba_stats { int32_t iterations_first, iterations_second, free_poses, reserved; double chi2_first, chi2_second; } sgx_ba_stats;
int sgx_local_bundle_adjustment(const sgx_ba_problem *problem, const sgx_camera *cam, const volatile int32_t *stop_flag,
                                uint8_t *edge_erase, sgx_ba_stats *stats);
/* Replaces `static void Optimizer::BundleAdjustment(const vector<KeyFrame*> &vpKFs, const vector<MapPoint*> &vpMP, int nIterations, bool *pbStopFlag,
 * const unsigned long nLoopKF, const bool bRobust)` (src/sg-slam/include/Optimizer.h:44-46, src/sg-slam/src/Optimizer.cc:49-237; GlobalBundleAdjustemnt :40-47 is
 * the same call on all keyframes / map points of the Map): every non-bad keyframe is a pose (pose_fixed != 0 exactly for mnId == 0), every non-bad map point a
 * landmark, one edge per observation in a keyframe of the problem; ONE optimizer.optimize(nIterations) with Huber kernels sqrt(5.99) / sqrt(7.815) when bRobust, no
 * outlier classification.  Out: every pose (the fixed one included, :200-214) and every point that has at least one edge (:216-236; the others are
 * vbNotIncludedMP) — the caller stores them with SetPose / SetWorldPos (nLoopKF == 0) or in mTcwGBA / mPosGBA.  stats: iterations_first, chi2_first. */
int sgx_bundle_adjustment(const sgx_ba_problem *problem, const sgx_camera *cam, int n_iterations, const volatile int32_t *stop_flag, int robust, sgx_ba_stats *stats);

/* int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale)
 * (src/sg-slam/include/Optimizer.h:56-57, src/sg-slam/src/Optimizer.cc:1046-1257; caller LoopClosing::ComputeSim3, LoopClosing.cc:326).  The caller lists the n correspondences the
 * reference turns into edge pairs (vpMatches1[i] && both map points good && pMP2 observed in pKF2, :1107-1133) in index order: p1c / p2c = the two map points in their own
 * keyframe's camera frame (R1w*P3D1w + t1w, R2w*P3D2w + t2w), obs1 / obs2 = kpUn.pt, info1 / info2 = mvInvLevelSigma2[octave], K1 / K2 = (fx, fy, cx, cy).
 * S12 in/out = (qx, qy, qz, qw, tx, ty, tz, s) of g2o::Sim3; inlier[i] = 0 where the reference sets vpMatches1[idx] = NULL; iterations (optional) = LM iterations of the two
 * optimize() calls; *n_inliers = return value (0 with S12 untouched when fewer than 10 correspondences survive the first check).  Host pointers, synchronous. */
int sgx_optimize_sim3(int n, const float *p1c, const float *p2c, const float *obs1, const float *obs2, const float *info1, const float *info2,
                      const float *K1, const float *K2, double *S12, float th2, int fix_scale, uint8_t *inlier, int32_t *iterations, int32_t *n_inliers);

/* The optimisation of void Optimizer::OptimizeEssentialGraph(Map*, KeyFrame *pLoopKF, KeyFrame *pCurKF, const KeyFrameAndPose &NonCorrectedSim3, const KeyFrameAndPose &CorrectedSim3,
 * const map<KeyFrame*, set<KeyFrame*>> &LoopConnections, const bool &bFixScale) (src/sg-slam/include/Optimizer.h:49-52, src/sg-slam/src/Optimizer.cc:781-1042; caller
 * LoopClosing::CorrectLoop, LoopClosing.cc:567): solver->setUserLambdaInit(1e-16); optimize(20) on the pose graph the reference builds at :807-958.  The caller flattens that graph:
 * S_in[v] = the vertex estimate (vScw: the corrected Sim3 where CorrectedSim3 holds the keyframe, Sim3(Rcw, tcw, 1) otherwise) as (qx, qy, qz, qw, tx, ty, tz, s); fixed[v] != 0 for
 * pLoopKF; one row per g2o::EdgeSim3 in insertion order: e_i = vertex 0, e_j = vertex 1, e_meas = the measurement Sji.  S_out[v] = the optimised estimates (CorrectedSiw, :970-973);
 * stats (optional, 3 doubles): LM iterations, chi2 before, chi2 after.  EdgeSim3 has no analytic Jacobian in the vendored g2o: numeric differences, as the reference.  Host pointers. */
int sgx_optimize_essential_graph(int nv, const double *S_in, const uint8_t *fixed, int ne, const int32_t *e_i, const int32_t *e_j, const double *e_meas,
                                 int fix_scale, int iterations, double *S_out, double *stats);
/* The map-point correction that follows (Optimizer.cc:1004-1041): xw_out[i] = correctedSwr.map(Srw.map(xw[i])) with r = ref[i], the point's reference keyframe (or mnCorrectedReference);
 * Srw = vScw, corrected_Swr = vCorrectedSwc (nv x 8 each).  The pose recovery [R t/s; 0 1] (:975-985) is three divisions on the host. */
int sgx_correct_map_points(int n, const float *xw, const int32_t *ref, int nv, const double *Srw, const double *corrected_Swr, float *xw_out);
/* The Sim3 arithmetic of loop closing between the index rows of sgx_covis_loop_begin / sgx_covis_essential_graph and the two entries above.  A Sim3 is 8 doubles
 * (qx, qy, qz, qw, tx, ty, tz, s), a pose 12 floats, the rows of [R | t].  Double except where the reference is float; device, emulator and a scalar float64 restatement
 * (tests/loop_ref.py) agree in every bit.  The _dev forms take device pointers and a stream and check nothing they would have to read back: vertex_group in [-1, n_group)
 * and edge ends in [0, nv) are the caller's, as sgx_covis_essential_graph writes them; the host forms check them (SGX_ERR_INVALID) and are synchronous.
 * sgx_loop_propagate_sim3 (LoopClosing::CorrectLoop, LoopClosing.cc:440-469, :503-512): Tcw of the group in group order, the current keyframe last, and its Scw.
 *   noncorrected[g] = Sim3(Riw, tiw, 1); corrected[g] = Sim3(Ric, tic, 1) * Scw with Tic = Tiw * Twc, a float cv::Mat product on cv::gemm's small-matrix path (float dot
 *   product left to right, four terms, the result through double with alpha), Twc as KeyFrame::SetPose builds it (Rwc = Rcw.t(), Ow = -Rwc * tcw: alpha = -1); for the
 *   current keyframe Scw itself; corrected_Tiw[g] = (toRotationMatrix(), t * (1 / s)) cast to float, what :503-512 hands to SetPose.
 *   CorrectLoop's point correction (:491-497) is sgx_correct_map_points with ref = point_ref, Srw = noncorrected, corrected_Swr = the inverses of corrected
 *   (sgx_eg_recover of corrected gives them).
 * sgx_eg_flatten (Optimizer.cc:818-832, :857-867, :889-972): S_in[v] = corrected[vertex_group[v]] for a vertex of the group, Sim3(Rcw, tcw, 1) of Tcw[v] otherwise (Tcw:
 *   nv poses in vertex order; a group vertex's is not read); e_meas[k] = Sjw * Swi, both operands S_in for e_kind 0, noncorrected for a group vertex of kinds 1-3.
 *   The outputs with vertex_fixed, e_i and e_j are what sgx_optimize_essential_graph takes.
 * sgx_eg_recover (:991-1010): Tcw[v] = (toRotationMatrix(), t * (1 / s)) of S_out[v] cast to float, corrected_Swc[v] = S_out[v].inverse(); the point correction of
 *   :1013-1041 is sgx_correct_map_points with Srw = S_in and corrected_Swr = corrected_Swc.
 * sgx_correct_map_points_dev: sgx_correct_map_points on device pointers and a stream (ref in [0, number of Sim3 rows) is the caller's), evaluated as written like the
 *   three above; the host-pointer form lets multiply-adds fuse and may differ from it in the last bit of a float. */
int sgx_loop_propagate_sim3_dev(int n_group, const float *Tcw_dev, const double *Scw_dev, double *noncorrected_dev, double *corrected_dev, float *corrected_Tiw_dev, void *stream);
int sgx_eg_flatten_dev(int nv, const int32_t *vertex_group_dev, const float *Tcw_dev, int n_group, const double *corrected_dev, const double *noncorrected_dev, int ne,
                       const int32_t *e_i_dev, const int32_t *e_j_dev, const uint8_t *e_kind_dev, double *S_in_dev, double *e_meas_dev, void *stream);
int sgx_eg_recover_dev(int nv, const double *S_out_dev, float *Tcw_dev, double *corrected_Swc_dev, void *stream);
int sgx_correct_map_points_dev(int n, const float *xw_dev, const int32_t *ref_dev, const double *Srw_dev, const double *corrected_Swr_dev, float *xw_out_dev, void *stream);
int sgx_loop_propagate_sim3(int n_group, const float *Tcw, const double *Scw, double *noncorrected, double *corrected, float *corrected_Tiw);
int sgx_eg_flatten(int nv, const int32_t *vertex_group, const float *Tcw, int n_group, const double *corrected, const double *noncorrected, int ne, const int32_t *e_i,
                   const int32_t *e_j, const uint8_t *e_kind, double *S_in, double *e_meas);
int sgx_eg_recover(int nv, const double *S_out, float *Tcw, double *corrected_Swc);

/* ---- 2-D detector + dynamic-feature mask --------------------------------------------------------
 * Replaces ORB_SLAM2::Detector2D (src/sg-slam/include/Detector2D.h:45-67, src/sg-slam/src/Detector2D.cc:16-89): the ncnn
 * forward pass of the shipped MobileNetV3-SSDLite graph (Thirdparty/ncnn_model/mobilenetv3_ssdlite_voc.param + .bin) on 300x300,
 * DetectionOutput, and detect()'s filtering into mvObjects2D / mvPotentialDynamicBorderForMapping / ...ForRmDynamicFeature.
 * sgx_det_create takes the .param TEXT and the .bin BYTES (the caller reads the two files Detector2D.cc:24-25 names);
 * pointwise convolutions run as fp32-MFMA GEMMs.  The Run()/isNewImageArrived()/ImageDetectFinished() thread handshake
 * (Detector2D.cc:122-149) becomes stream ordering: the caller launches detect on its own HIP stream / thread. */
#define SGX_DET_MAX 100
typedef struct sgx_detection { float label, score, xmin, ymin, xmax, ymax; } sgx_detection;        /* ncnn DetectionOutput row (normalised coords) */
typedef struct sgx_object2d { int32_t id; float prob, x, y, w, h; } sgx_object2d;                   /* Object2D: class id, prob, cv::Rect_<float> in pixels */
typedef struct sgx_det_result {
    int32_t n_raw; sgx_detection raw[SGX_DET_MAX];
    int32_t n_objects; sgx_object2d objects[SGX_DET_MAX];            /* mvObjects2D (non-person) */
    int32_t have_dynamic_for_mapping, have_dynamic_for_rm_feature;   /* mbHaveDynamicObjectFor{Mapping,RmDynamicFeature} */
    int32_t n_map_boxes; sgx_object2d map_boxes[SGX_DET_MAX];        /* mvPotentialDynamicBorderForMapping */
    int32_t n_rm_boxes; sgx_object2d rm_boxes[SGX_DET_MAX];          /* mvPotentialDynamicBorderForRmDynamicFeature (prob > 0.2) */
} sgx_det_result;
typedef struct sgx_det sgx_det;
int sgx_det_create(const char *param_text, const void *bin, size_t bin_bytes, int width, int height, int max_batch,
                   float detection_confidence_threshold, float dynamic_detection_confidence_threshold, sgx_det **out);
void sgx_det_destroy(sgx_det *h);
int sgx_det_info(const sgx_det *h, int32_t *num_priors, int32_t *num_class, int32_t *num_kernels, double *gmac);
/* Detector2D::detect(const cv::Mat &bgr) for `batch` host images (interleaved 3-channel u8, row pitch in bytes); synchronous */
int sgx_det_detect(sgx_det *h, const uint8_t *images, int pitch, int batch, sgx_det_result *results);
/* Detector2D::detect, device-resident and asynchronous on `stream`: forward + ncnn DetectionOutput (decode, per-class NMS, keep_top_k) + detect()'s
 * filtering, all on the GPU.  d_results: batch structs in device memory (same layout as the host entry fills).  d_boxes / d_nboxes / d_have_dynamic
 * (optional, may be NULL): the person rectangles (max_boxes x (x, y, w, h) per image), their count and mbHaveDynamicObjectForRmDynamicFeature, laid out
 * as sgx_dynamic_mask_batch_dev / sgx_frame_compact_keys_batch_dev take them — Detector2D.cc:53-88 feeding Frame.cc:482-500 without a host round trip.
 * Two documented differences from the reference, both where the reference's own result is not defined:
 *   - Frame.cc:482-491 copies the detector's flags into the Frame only when mvObjects2D (the NON-person list) is not empty; otherwise the Frame's
 *     mbHaveDynamicObjectForRmDynamicFeature (Frame.h:112, never initialised by the constructor) is read indeterminate at :493/:512/:565/:599.  d_have_dynamic[f]
 *     here is always Detector2D's own flag (a person with prob > 0.2 exists), i.e. the value the reference reads whenever it is defined.
 *   - ncnn's DetectionOutput orders candidates with an unstable quicksort (qsort_descent_inplace); rows with EXACTLY equal scores may come out in either order
 *     there.  Here (and in oracle/detector_oracle.py) ties keep class-major, then prior-index order (a stable sort); with distinct scores the outputs agree. */
int sgx_det_detect_batch_dev(sgx_det *h, const uint8_t *d_img, int pitch, int batch, sgx_det_result *d_results,
                             float *d_boxes, int32_t *d_nboxes, int max_boxes, int32_t *d_have_dynamic, void *stream);
/* device-resident batched forward only: leaves mbox_loc (num_priors*4) and softmax conf (num_priors*num_class) per image in HBM */
int sgx_det_forward_batch_dev(sgx_det *h, const uint8_t *d_img, int pitch, int batch, const float **d_loc, const float **d_conf, void *stream);
/* Matrix-product scheme of the detector's 1x1 convolutions (pointwise / expand / project / squeeze-excite), read by the NEXT sgx_det_create: 0 = exact fp32
 * (v_mfma_f32_32x32x2_f32, an ascending-k fmaf chain: bit-identical to the per-layer reference kernels), 1 = bf16x3 (each fp32 operand split exactly into three
 * bf16 terms, the six leading cross products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation: fp32-accurate products in another summation order), -1 = the
 * default (1).  Selected per detector by the test tap sgx_det_debug_set_gemm (include/sgx_debug.h); sgx_det_gemm_mode reports what a detector was built with. */
int sgx_det_gemm_mode(const sgx_det *h);
/* one line of text per plan step i in [0, num_kernels of sgx_det_info): kind, ncnn layers, shapes, ' bf16x3' behind the steps that run on the bf16 matrix pipes (introspection for
 * profilers and the roofline accounting of bench.py); SGX_ERR_INVALID past the last step */
int sgx_det_plan_step(const sgx_det *h, int i, char *buf, int cap);
/* Frame::RmDynamicPointWithSemanticAndGeometry's keep/erase predicate (src/sg-slam/src/Frame.cc:556-597, :613-652): keep[i] = 1 when the
 * epipolar distance of (keypoint i, its LK-tracked previous position) under F (3x3 row-major fp64, cv::findFundamentalMat) is below
 * 0.2 px inside a person box / 1.0 px elsewhere (an all-zero F = "no fundamental matrix": the frame keeps every keypoint).  boxes: max_boxes x (x, y, w, h) per frame.  The caller applies the
 * "restore everything when fewer than 0.1*nFeatures survive" rule (:599-604) and compacts keypoints + descriptor rows. */
int sgx_dynamic_mask_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n, const float *d_prev_xy, const double *d_F,
                               const float *d_boxes, const int32_t *d_nboxes, int max_boxes, uint8_t *d_keep, void *stream);
/* The erase step that follows the mask (Frame.cc:556-604): keypoints with keep == 0 and their descriptor rows are removed, order preserved;
 * when have_dynamic[f] != 0 (a person box with prob > 0.2 exists, Detector2D.cc:80-84) and fewer than 0.1 * nfeatures keypoints survive, all
 * keypoints of the frame are restored (:599-604).  Out of place; d_have_dynamic may be NULL (no dynamic object in any frame). */
int sgx_frame_compact_keys_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const uint8_t *d_desc, const int32_t *d_n, const uint8_t *d_keep,
                                     const int32_t *d_have_dynamic, int nfeatures, sgx_keypoint *d_keys_out, uint8_t *d_desc_out, int32_t *d_n_out, void *stream);
/* The same erase step where descriptors do not exist yet (after sgx_orb_detect_batch_dev): keypoints only; d_src_out[f * cap + j] = index in d_keys of output keypoint j,
 * ascending (the identity when everything is restored) — what sgx_orb_describe_batch_dev takes. */
int sgx_frame_compact_keys_src_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n, const uint8_t *d_keep, const int32_t *d_have_dynamic,
                                         int nfeatures, sgx_keypoint *d_keys_out, int32_t *d_src_out, int32_t *d_n_out, void *stream);


/* ---- inputs of the dynamic-feature mask: optical flow + fundamental matrix ------------------------
 * What Frame::RmDynamicPointWithSemanticAndGeometry computes before its erase loop (src/sg-slam/src/Frame.cc:430-472):
 *   :445     cv::calcOpticalFlowPyrLK(imGray, imGrayPre, Curpoint, Prepoint, State, Err, Size(21,21), 3, TermCriteria(ITER|EPS, 30, 0.01))
 *            — every keypoint of the current frame tracked into the PREVIOUS frame (State / Err are ignored by the caller)
 *   :454-467 the pairs whose previous position lies outside the previous frame's person boxes (vPreFramePotentialDynamicBorder)
 *   :469-472 cv::findFundamentalMat(cur, prev, FM_RANSAC, 1.0, 0.99) on that selection when more than 20 pairs remain, else on all pairs
 * A sgx_flow handle owns the two image pyramids (current / previous) like the file-scope `imGrayPre` of Frame.cc:31,155-163: each
 * sgx_flow_lk_batch_dev call builds the pyramid of the new frames, tracks into the pyramid kept from the previous call, and swaps (the Scharr
 * derivatives are evaluated inside the tracker from the image itself).  OpenCV 3.4 semantics (lkpyramid.cpp, pyramids.cpp).
 * Divergence (stated, with the two undefined reference behaviours documented at sgx_det_detect and sgx_fundamental_ransac_batch_dev): the 2 x 2 gradient matrix and the
 * mismatch vector of every iteration are summed EXACTLY (int32 partial sums recombined in fp64, rounded once to fp32) — the order-free form of OpenCV's accumulation,
 * whose own float summation order depends on the SIMD path the build dispatches to (SSE2 / AVX2 / scalar `acctype`).  Against the oracle's OpenCV-order mode
 * (oracle/flow_oracle.c, acc_mode 0) tracked positions agree to 0.01 px on the test streams; mask decisions of knife-edge keypoints can therefore differ from a
 * given x86 build of the reference (bench.py reports the resulting trajectory difference as `ate_vs_oracle_chain`). */
typedef struct sgx_flow_config {
    int32_t width, height, max_batch;
    int32_t win_size;       /* 21 (only value supported) */
    int32_t max_level;      /* 3  (0..3) */
    int32_t max_count;      /* 30 */
    double epsilon;         /* 0.01 */
} sgx_flow_config;
typedef struct sgx_flow sgx_flow;
int sgx_flow_create(const sgx_flow_config *cfg, sgx_flow **out);
void sgx_flow_destroy(sgx_flow *h);
int sgx_flow_reset(sgx_flow *h);                 /* forget the previous frame (imGrayPre.data == NULL) */
int sgx_flow_levels(const sgx_flow *h);          /* pyramid levels actually used (buildOpticalFlowPyramid stops when a level is not larger than the window) */
/* d_gray: batch frames of height rows x pitch bytes (pitch and pointer multiples of 4).  When the handle holds a previous batch of the same size:
 * d_prev_xy[f*cap + i] = (x, y) of keypoint i of frame f in the previous frame (nextPts), d_status (optional) = State; *have_prev (host, optional) = 1.
 * First call after create / reset: only the pyramid is built, *have_prev = 0 (the reference skips the whole mask step, Frame.cc:155-163).
 * Tracking needs width and height of at least 22 (win_size + 1: the tracker reflects a window index once, which covers a 21-pixel window only on such a side): a call that
 * would track on a smaller handle returns SGX_ERR_UNSUPPORTED and changes nothing.  Pyramid-only calls (the first after create / reset) work at any size from 2 x 2.
 * Asynchronous on `stream`. */
int sgx_flow_lk_batch_dev(sgx_flow *h, const uint8_t *d_gray, int pitch, int batch, const sgx_keypoint *d_keys, const int32_t *d_n, int cap,
                          float *d_prev_xy, uint8_t *d_status, int32_t *have_prev, void *stream);
/* cv::calcOpticalFlowPyrLK(gray_from, gray_to, pts, next_pts, status, ...) on one host image pair (n points, 2 floats each).  Synchronous; resets the streaming state.
 * SGX_ERR_UNSUPPORTED when the handle's width or height is below 22 (see sgx_flow_lk_batch_dev); OpenCV itself accepts such images, the reference never passes one. */
int sgx_flow_lk(sgx_flow *h, const uint8_t *gray_from, const uint8_t *gray_to, int stride, const float *pts, int n, float *next_pts, uint8_t *status);
/* Frame.cc:454-472 for `batch` frames: pair selection against the PREVIOUS frame's person boxes (d_pre_have_dynamic = bPreFrameHavePotentialDynamicObj,
 * d_pre_boxes / d_pre_nboxes = vPreFramePotentialDynamicBorder in the layout sgx_det_detect_batch_dev writes; all three may be NULL) and
 * cv::findFundamentalMat(FM_RANSAC, threshold, confidence): cv::RNG(-1) sampling, 7-point solver, symmetric epipolar error, adaptive iteration count,
 * no refit (fundam.cpp, ptsetreg.cpp).  d_F: 9 doubles per frame, row-major, x_prev^T F x_cur = 0 (what sgx_dynamic_mask_batch_dev takes);
 * d_ok[f] = 0 when OpenCV would return an empty Mat (fewer than 7 pairs, or no model) — F is then all zeros and the mask keeps every keypoint of
 * that frame (the reference indexes the empty Mat: undefined behaviour).  For 8..14 pairs OpenCV switches to LMeDSPointSetRegistrator::run and so does this entry
 * (same subsets from the same RNG, smallest median error, sigma-based inlier count, success = at least 7 inliers).
 * d_stats (optional): 4 ints per frame — RANSAC iterations run, iteration and root index of the returned model, its inlier count. */
int sgx_fundamental_ransac_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n, const float *d_prev_xy,
                                     const int32_t *d_pre_have_dynamic, const float *d_pre_boxes, const int32_t *d_pre_nboxes, int max_boxes,
                                     double threshold, double confidence, double *d_F, int32_t *d_ok, int32_t *d_stats, void *stream);
/* cv::findFundamentalMat(pts1, pts2, FM_RANSAC, threshold, confidence) on host points.  Synchronous. */
int sgx_find_fundamental_mat(const float *pts1, const float *pts2, int n, double threshold, double confidence, double *F, int32_t *ok, int32_t *stats);

/* ---- the pipelined per-frame host (C++ behind this C ABI: sg_slam_amd/csrc/sgx_tracker.cpp) ---------------------------------
 * S independent RGB-D streams tracked in lock-step on one GPU, one frame per stream per step, in the call order of the reference's tracking thread:
 * Tracking::GrabImageRGBD (src/sg-slam/src/Tracking.cc:206-251) -> Frame::Frame (src/sg-slam/src/Frame.cc:100-200: ExtractORB, detector hand-shake :170-176 / :478,
 * RmDynamicPointWithSemanticAndGeometry :430-610, ComputeStereoFromRGBD :893-914) -> Tracking::TrackWithMotionModel / TrackLocalMap (Tracking.cc:906-1013), in
 * visual-odometry form (Tracking::UpdateLastFrame :840-904 points; local map = the points of frames t-2, t-3).  Three HIP streams (detector | extraction + mask |
 * tracking) chained by events, triple-buffered frame state, no host synchronisation inside a step; an optional fourth stream uploads host frames.
 * It is the harness host of bench.py / example_track.cpp / the tests — keyframe decisions, relocalisation and the map stay with ORB_SLAM2::Tracking. */
typedef struct sgx_tracker_config {
    int32_t streams, width, height;
    int32_t nfeatures; float scale_factor; int32_t nlevels, ini_th_fast, min_th_fast;      /* ORBextractor.* of the settings file (TUM3.yaml: 1000, 1.2, 8, 20, 7) */
    sgx_camera cam; float depth_map_factor;                                                 /* Camera.*, DepthMapFactor (5000) */
    float th_projection;                                                                    /* SearchByProjection(cur, last, th): 15 (Tracking.cc:924) */
    int32_t local_map;                                                                      /* 1: TrackLocalMap stage (SearchLocalPoints + second PoseOptimization) */
    int32_t dynamic_mask;                                                                   /* 1: calcOpticalFlowPyrLK + findFundamentalMat + mask + erase (Frame.cc:430-610) */
    int32_t max_boxes;                                                                      /* person rectangles kept per frame (<= SGX_DET_MAX) */
    int32_t pipelined;                                                                      /* 1: own HIP streams; 0: everything on the caller's stream (tests) */
} sgx_tracker_config;
typedef struct sgx_tracker sgx_tracker;
/* *out is NULL after any failed call.  The status is the one that occurred: SGX_ERR_NOMEM for a refused allocation, SGX_ERR_DEVICE for a failed fill, copy, stream or event;
 * whatever had been acquired is released.  sgx_tracker_destroy waits for the tracker's work and releases everything the tracker acquired. */
int sgx_tracker_create(const sgx_tracker_config *cfg, sgx_det *detector /* NULL: no Detector2D::detect; not owned */, sgx_tracker **out);
void sgx_tracker_destroy(sgx_tracker *t);
int sgx_tracker_keypoint_capacity(const sgx_tracker *t);
int sgx_tracker_record_bytes(const sgx_tracker *t);                   /* 16 + cap * 28 + cap * 32 + 64: the per-frame record of BASELINE config 5 */
int sgx_tracker_set_initial_pose(sgx_tracker *t, const float *Tcw /* streams x 16, host */);
/* the camera's distortion coefficients (mDistCoef, Tracking.cc:66-77; ndist 4, 5 or 8), before the first step only (else SGX_ERR_INVALID).  dist[0] == 0: no
 * change (Frame.cc:656-660 / :707-713 skip everything).  Otherwise the grid / frustum bounds become those of sgx_frame_image_bounds (copied to *out_cam when it
 * is not NULL; with dist[0] == 0 *out_cam receives the unchanged camera), every frame's keypoints are undistorted beside ComputeStereoFromRGBD, and the
 * undistorted keypoints (mvKeysUn) feed the matchers, both PoseOptimization calls, the unprojection and the map points; ORB, LK, RANSAC, the dynamic mask
 * and the erase step keep the raw ones.  All or nothing: a call that fails leaves the tracker exactly as it was (no distortion, or the previous coefficients) and may be
 * repeated. */
int sgx_tracker_set_distortion(sgx_tracker *t, const float *dist, int ndist, sgx_camera *out_cam);
/* one frame of every stream from device memory: d_gray streams x height x gray_pitch u8, d_depth streams x height x width raw u16, d_bgr (optional, detector
 * input) streams x height x bgr_pitch interleaved 3-channel u8.  Asynchronous — a step only ENQUEUES work.  The inputs of a step may be rewritten
 * (a) by work enqueued on `caller_stream` after the THIRD following sgx_tracker_step_dev call (that call orders caller_stream behind the step's readers), or
 * (b) from the host after sgx_tracker_wait_inputs(t, steps_back) or sgx_tracker_sync returned.
 * A refused argument (SGX_ERR_INVALID) enqueues nothing and changes nothing.  A step that fails once enqueueing has begun POISONS the tracker: the frame was issued in part,
 * so sgx_tracker_step_dev, sgx_tracker_step_host and sgx_tracker_pack_records_dev return that first status from then on without enqueueing anything;
 * sgx_tracker_sync, _read, _wait_inputs and _destroy keep working. */
int sgx_tracker_step_dev(sgx_tracker *t, const uint8_t *d_gray, int gray_pitch, const uint16_t *d_depth, const uint8_t *d_bgr, int bgr_pitch, void *caller_stream);
/* host input (cv::imread's BGR image + the 16-bit depth map, rgbd_tum.cc:114-115): fill the pinned staging buffers of slot 0 / 1, then step; the tracker uploads
 * them on its own stream and converts to gray on the device (Tracking.cc:214-227; rgb_order = Camera.RGB).  The upload is asynchronous: before REFILLING a slot call
 * sgx_tracker_host_buffers(slot) again — it returns once the slot's pending upload has left the pinned buffers — or sgx_tracker_sync.
 * The first sgx_tracker_host_buffers call sets the staging up, all or nothing: a call that fails has released what it acquired, sgx_tracker_step_host goes on refusing
 * with SGX_ERR_INVALID, and the next call starts from scratch.  A failed sgx_tracker_step_host poisons the tracker as a failed sgx_tracker_step_dev does. */
int sgx_tracker_host_buffers(sgx_tracker *t, int slot, uint8_t **bgr, int *bgr_pitch, uint16_t **depth);
int sgx_tracker_step_host(sgx_tracker *t, int slot, int rgb_order);
/* blocks the host until the device has read the input images of the step issued `steps_back` (0..2) calls ago */
int sgx_tracker_wait_inputs(sgx_tracker *t, int steps_back);
int sgx_tracker_sync(sgx_tracker *t);
/* results of the frame tracked last (synchronises; any pointer may be NULL): Tcw streams x 16, keypoints after the mask, motion-model matches / inliers, local-map
 * matches / inliers of the second PoseOptimization, keypoints before the mask, findFundamentalMat success, its 4 statistics per stream */
int sgx_tracker_read(sgx_tracker *t, float *Tcw, int32_t *nkeys, int32_t *nmatches, int32_t *ninliers, int32_t *nmatches_local, int32_t *ninliers2, int32_t *nkeys_raw,
                     int32_t *f_ok, int32_t *f_stats);
int sgx_tracker_snapshot_pose_dev(sgx_tracker *t, float *d_out /* streams x 16 */);                               /* async copy on the tracking stream */
int sgx_tracker_snapshot_boxes_dev(sgx_tracker *t, int stream_index, float *d_boxes /* max_boxes x 4 */, int32_t *d_nboxes);   /* async copy on the detector stream */
/* (both snapshots copy on the tracker's own non-blocking streams: the destination buffers must have no pending writes on other streams — e.g. a zero-fill — when they are called) */
/* the frame records {n, cv::KeyPoint[cap], descriptors[cap][32], Tcw} of the frame tracked last, packed by one kernel into d_records (streams x record_bytes) on
 * `stream` after the frame's tracking event: what the RCCL gather of BASELINE config 5 sends */
int sgx_tracker_pack_records_dev(sgx_tracker *t, uint8_t *d_records, void *stream);
/* ---- the collective of BASELINE config 5 from the C++ host (round 6): gather of every rank's packed frame records to `root` over RCCL / xGMI ------------------------
 * One process per GPU.  Rank 0 calls sgx_dist_unique_id and hands the 128 bytes to the other ranks (the caller's launcher: MPI, a file, a socket); every rank then calls
 * sgx_dist_create on its own device.  sgx_dist_gather_records enqueues a grouped ncclSend / ncclRecv on `stream` — the stream sgx_tracker_pack_records_dev packed on — and
 * returns without synchronising: every rank sends bytes_per_rank = streams x record_bytes from d_send; root receives world such blocks side by side in d_recv (block r =
 * rank r's), the other ranks pass d_recv = NULL.  RCCL is loaded on first use (dlopen): a single-GPU program never needs it; SGX_ERR_UNSUPPORTED if it is absent.
 * Replaces nothing in the reference (it is single-GPU); the Python harness uses torch.distributed for the same pattern (sg_slam_amd/dist.py). */
typedef struct sgx_dist sgx_dist;
int sgx_dist_unique_id(void *id128 /* 128 bytes out */);
int sgx_dist_create(const void *id128, int world, int rank, sgx_dist **out);
void sgx_dist_destroy(sgx_dist *d);
int sgx_dist_world(const sgx_dist *d, int32_t *world, int32_t *rank);
int sgx_dist_gather_records(sgx_dist *d, const void *d_send, size_t bytes_per_rank, void *d_recv, int root, void *stream);
int sgx_tracker_frame_dev(sgx_tracker *t, const int32_t **d_n, const sgx_keypoint **d_keys, const uint8_t **d_desc, const float **d_Tcw, const float **d_xw, const uint8_t **d_has);
/* the undistorted keypoints (mvKeysUn) of the frame tracked last: the d_keys of sgx_tracker_frame_dev when the tracker has no distortion */
int sgx_tracker_frame_keys_un_dev(sgx_tracker *t, const sgx_keypoint **d_keys_un);
sgx_orb *sgx_tracker_extractor(sgx_tracker *t);

/* ---- Frame::ComputeStereoMatches (Frame.cc:716-890): the stereo constructor's mvuRight / mvDepth from a rectified pair ---------------------------------------------
 * For every left keypoint: the right keypoint of smallest descriptor distance on its row band (+-2 * scale rows, +-1 octave, uL - maxD <= uR <= uL, distance below 75),
 * an 11 x 11 SAD window slid over +-5 px in both pyramids at the left keypoint's level, a parabola through the best offset, depth = bf / disparity, and the cut of
 * every match whose SAD is at least 1.5 * 1.4 times the median.  Results equal the reference bit for bit; three cases it leaves undefined are defined:
 * mb = bf / fx (read before it is assigned there), so maxD = bf / mb; a window or a table row outside the image gives no match; no accepted match, nothing to cut.
 * The handle owns the workspace for max_batch pairs of extractors with the geometry of `geometry_of` (image size, levels, scale factor, nfeatures); nothing is
 * allocated per call. */
typedef struct sgx_stereo sgx_stereo;
int sgx_stereo_create(const sgx_orb *geometry_of, int max_batch, sgx_stereo **out);      /* *out is NULL after a failed call */
void sgx_stereo_destroy(sgx_stereo *h);
/* `batch` pairs on `stream`, asynchronous, nothing read back.  The pyramids are those of the LAST sgx_orb_extract_batch_dev or sgx_orb_detect_batch_dev of each
 * extractor handle, which must have run on the same stream on the same d_gray / pitch: pair f reads frame left_first_frame + f of orb_left and frame
 * right_first_frame + f of orb_right.  orb_left == orb_right is allowed and is the fast form: one extraction of 2 * batch images, the left ones first, and
 * right_first_frame = batch (d_gray_right = d_gray_left; the right key, descriptor and count pointers are those of frame `batch`).  cap: slots per frame of every
 * key / descriptor / output array = sgx_orb_keypoint_capacity of the extractors.  d_uright / d_zdepth: batch x cap as sgx_frame_stereo_from_rgbd_batch_dev writes
 * them, -1 where there is no match; d_nmatched (optional): matches kept per pair.  SGX_ERR_INVALID, with nothing enqueued: a NULL pointer, batch > max_batch, another
 * cap, an extractor of another geometry, an extractor without a pyramid for first_frame + batch frames or with one of another image. */
int sgx_stereo_match_batch_dev(sgx_stereo *h, int batch,
                               sgx_orb *orb_left, int left_first_frame, const uint8_t *d_gray_left, int pitch_left,
                               sgx_orb *orb_right, int right_first_frame, const uint8_t *d_gray_right, int pitch_right,
                               int cap, const sgx_keypoint *d_keys_left, const uint8_t *d_desc_left, const int32_t *d_n_left,
                               const sgx_keypoint *d_keys_right, const uint8_t *d_desc_right, const int32_t *d_n_right,
                               float fx, float bf, float *d_uright, float *d_zdepth, int32_t *d_nmatched /* may be NULL */, void *stream);
/* one pair from host memory, synchronous, as sgx_orb_extract is: orb_left and orb_right are two handles (the reference's two extractors) whose last call was
 * sgx_orb_extract on the left and on the right image; keys / descriptors are what those calls returned.  uright / zdepth: n_left floats each. */
int sgx_stereo_match(sgx_stereo *h, sgx_orb *orb_left, sgx_orb *orb_right, const sgx_keypoint *keys_left, const uint8_t *desc_left, int n_left,
                     const sgx_keypoint *keys_right, const uint8_t *desc_right, int n_right, float fx, float bf, float *uright, float *zdepth, int *nmatched /* may be NULL */);

/* ---- per-kernel HIP-event timing (process-wide) ---------------------------------------------------
 * When enabled, every batched entry point records a hipEvent pair on the caller's stream around each
 * kernel launch.  sgx_profile_read sums the elapsed times per kernel class since the last reset
 * (ms[k], launches[k] for k < sgx_profile_num_classes(); it synchronises the device). */
int sgx_profile_enable(int on);
int sgx_profile_num_classes(void);
const char *sgx_profile_class_name(int k);
int sgx_profile_read(float *ms, int32_t *launches, int reset);

#ifdef __cplusplus
}
#endif
#endif
