// sgx_host.hpp — C++ host-side mirror of the reference operator interfaces over the C-ABI (include/sgx.h).
//
// Same class names, method names, argument meaning and error behaviour as the reference
// (src/sg-slam/include/{ORBextractor,ORBmatcher,Optimizer}.h), expressed on plain views instead of
// cv::Mat / Frame* so this header has no OpenCV dependency.  INTEGRATION.md shows the three-line glue that
// adapts cv::Mat / Frame to these views inside the reference tree.  Header-only; link with -lsgx.
#pragma once
#include <cfloat>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
#include <algorithm>
#include <vector>
#include "../../include/sgx.h"

namespace sgx {

struct GrayView { const uint8_t *data; int rows, cols, step; bool empty() const { return !data || rows <= 0 || cols <= 0; } };

// flattened ORB_SLAM2::Frame: what the matcher / optimiser read and write
struct FrameView {
    int N = 0;
    std::vector<sgx_keypoint> mvKeysUn;     // == mvKeys when the camera has no distortion (Frame.cc:656-660)
    std::vector<uint8_t> mDescriptors;      // N x 32
    std::vector<float> mvuRight, mvDepth;   // -1 when no depth
    std::vector<int32_t> mvpMapPoints;      // index into the owner of the map points (e.g. last frame), -1 = NULL
    std::vector<uint8_t> mvbOutlier;
    float mTcw[16] = {1,0,0,0, 0,1,0,0, 0,0,1,0, 0,0,0,1};
    // map points held by this frame's keypoints (used when this frame is the "LastFrame" of the matcher)
    std::vector<uint8_t> mpValid;           // mvpMapPoints[i] != NULL
    std::vector<float> mpWorldPos;          // N x 3   MapPoint::GetWorldPos()
    std::vector<int32_t> mpObservations;    // MapPoint::Observations()
    std::vector<uint8_t> mpDescriptor;      // N x 32  MapPoint::GetDescriptor()
};

// flattened local map (Tracking::mvpLocalMapPoints): what isInFrustum / SearchByProjection(F, vpMapPoints, th) read from each MapPoint
struct LocalMapView {
    int N = 0;
    std::vector<float> mWorldPos, mNormalVector;    // N x 3   GetWorldPos(), GetNormal()
    std::vector<float> mfMinDistance, mfMaxDistance;
    std::vector<uint8_t> mDescriptor;               // N x 32  GetDescriptor()
    std::vector<int32_t> nObs;                      // Observations()
    std::vector<uint8_t> skip;                      // isBad() || mnLastFrameSeen == F.mnId (Tracking.cc:1288-1291)
    std::vector<uint8_t> mbTrackInView;             // out: isInFrustum result (for IncreaseVisible)
};

inline void check(int rc, const char *what) { if (rc != SGX_OK) throw std::runtime_error(std::string(what) + ": " + sgx_status_string(rc)); }

// ORB_SLAM2::ORBextractor (ORBextractor.h:45-111)
class ORBextractor {
public:
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int width = 640, int height = 480)
        : nfeatures_(nfeatures), scaleFactor_(scaleFactor), nlevels_(nlevels)
    {
        sgx_orb_config c{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, width, height, 1};
        check(sgx_orb_create(&c, &h_), "sgx_orb_create");
        mvScaleFactor.resize(nlevels); mvInvScaleFactor.resize(nlevels); mvLevelSigma2.resize(nlevels); mvInvLevelSigma2.resize(nlevels);
        check(sgx_orb_get_tables(h_, mvScaleFactor.data(), mvInvScaleFactor.data(), mvLevelSigma2.data(), mvInvLevelSigma2.data(), nullptr), "sgx_orb_get_tables");
    }
    ~ORBextractor() { sgx_orb_destroy(h_); }
    ORBextractor(const ORBextractor &) = delete;
    ORBextractor &operator=(const ORBextractor &) = delete;

    // operator()(image, mask, keypoints, descriptors): mask is ignored, as in the reference (Frame.cc:277 passes cv::Mat())
    void operator()(const GrayView &image, const void * /*mask*/, std::vector<sgx_keypoint> &keypoints, std::vector<uint8_t> &descriptors)
    {
        keypoints.clear(); descriptors.clear();
        if (image.empty()) return;                                   // ORBextractor.cc:1048
        const int cap = sgx_orb_keypoint_capacity(h_);
        keypoints.resize(cap); descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(sgx_orb_extract(h_, image.data, image.step, keypoints.data(), descriptors.data(), cap, &n), "sgx_orb_extract");
        keypoints.resize(n); descriptors.resize((size_t)n * 32);
    }
    int GetLevels() { return nlevels_; }
    float GetScaleFactor() { return scaleFactor_; }
    std::vector<float> GetScaleFactors() { return mvScaleFactor; }
    std::vector<float> GetInverseScaleFactors() { return mvInvScaleFactor; }
    std::vector<float> GetScaleSigmaSquares() { return mvLevelSigma2; }
    std::vector<float> GetInverseScaleSigmaSquares() { return mvInvLevelSigma2; }
    int GetnFeatures() { return nfeatures_; }
    sgx_orb *handle() { return h_; }

private:
    sgx_orb *h_ = nullptr;
    int nfeatures_; float scaleFactor_; int nlevels_;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
};

// ORB_SLAM2::ORBmatcher (ORBmatcher.h:41-89) — SearchByProjection(CurrentFrame, LastFrame, th, bMono)
class ORBmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
    ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    static int DescriptorDistance(const uint8_t *a, const uint8_t *b)
    {
        int d = 0;
        for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
        return d;
    }

    // fills CurrentFrame.mvpMapPoints with indices of LastFrame map points; returns nmatches (ORBmatcher.cc:1332-1472)
    int SearchByProjection(FrameView &CurrentFrame, const FrameView &LastFrame, float th, bool bMono,
                           const sgx_camera &cam, const std::vector<float> &scaleFactors)
    {
        CurrentFrame.mvpMapPoints.assign(CurrentFrame.N, -1);
        std::vector<uint8_t> no_outlier(LastFrame.N, 0);
        const uint8_t *outl = LastFrame.mvbOutlier.size() == (size_t)LastFrame.N ? LastFrame.mvbOutlier.data() : no_outlier.data();
        int32_t n = 0;
        check(sgx_match_project_frame(CurrentFrame.N, CurrentFrame.mvKeysUn.data(), CurrentFrame.mDescriptors.data(), CurrentFrame.mvuRight.data(), CurrentFrame.mTcw,
                                      LastFrame.N, LastFrame.mvKeysUn.data(), LastFrame.mpValid.data(), outl, LastFrame.mpWorldPos.data(),
                                      LastFrame.mpObservations.data(), LastFrame.mpDescriptor.data(), LastFrame.mTcw,
                                      &cam, scaleFactors.data(), (int)scaleFactors.size(), th, bMono ? 1 : 0, mbCheckOrientation ? 1 : 0,
                                      CurrentFrame.mvpMapPoints.data(), &n), "sgx_match_project_frame");
        return n;
    }

    // Tracking::SearchLocalPoints' body (Tracking.cc:1284-1311): isInFrustum(pMP, 0.5) for every local point, then SearchByProjection(F, vpMapPoints, th)
    // (ORBmatcher.cc:45-129).  matched[k] = local point newly assigned to keypoint k of F (or -1); F.mvpMapPoints (>= 0 = holds a point) is only read.
    int SearchByProjection(FrameView &F, LocalMapView &M, float th, const sgx_camera &cam, const std::vector<float> &scaleFactors, std::vector<int32_t> &matched,
                           const std::vector<int32_t> *heldObservations = nullptr)
    {
        matched.assign(F.N, -1); M.mbTrackInView.assign(M.N, 0);
        int32_t n = 0;
        check(sgx_match_project_local(F.N, F.mvKeysUn.data(), F.mDescriptors.data(), F.mvuRight.data(), F.mTcw, heldObservations ? heldObservations->data() : nullptr,
                                      M.N, M.mWorldPos.data(), M.mNormalVector.data(), M.mfMinDistance.data(), M.mfMaxDistance.data(), M.mDescriptor.data(), M.nObs.data(), M.skip.data(),
                                      &cam, scaleFactors.data(), (int)scaleFactors.size(), std::log(scaleFactors[1]), th, mfNNratio, 0.5f,
                                      matched.data(), &n, M.mbTrackInView.data()), "sgx_match_project_local");
        return n;
    }

    // ---- LocalMapping / relocalisation gates (tier N2).  KeyFrameView: the flattened keyframe fields the reference reads.
    struct KeyFrameView {
        int N = 0;
        std::vector<sgx_keypoint> mvKeysUn; std::vector<uint8_t> mDescriptors; std::vector<float> mvuRight;
        std::vector<uint8_t> hasMapPoint;        // GetMapPoint(i) != NULL (for SearchByBoW: ... && !isBad())
        std::vector<int32_t> featNode;           // key of mFeatVec under which keypoint i sits (-1: none)
        float Tcw[16]; float Ow[3];
    };
    // int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs, const bool bOnlyStereo) (ORBmatcher.cc:659-827)
    int SearchForTriangulation(const KeyFrameView &KF1, const KeyFrameView &KF2, const float F12[9], const sgx_camera &cam2, const std::vector<float> &scaleFactors2,
                               const std::vector<float> &levelSigma2_2, std::vector<std::pair<size_t, size_t>> &vMatchedPairs, bool bOnlyStereo)
    {
        std::vector<int32_t> pairs((size_t)2 * (KF1.N > 0 ? KF1.N : 1)); int32_t np = 0;
        check(sgx_match_search_for_triangulation(KF1.N, KF1.mvKeysUn.data(), KF1.mDescriptors.data(), KF1.mvuRight.data(), KF1.hasMapPoint.data(), KF1.featNode.data(), KF1.Ow,
                                                 KF2.N, KF2.mvKeysUn.data(), KF2.mDescriptors.data(), KF2.mvuRight.data(), KF2.hasMapPoint.data(), KF2.featNode.data(), KF2.Tcw,
                                                 F12, &cam2, scaleFactors2.data(), levelSigma2_2.data(), (int)scaleFactors2.size(), bOnlyStereo ? 1 : 0, mbCheckOrientation ? 1 : 0,
                                                 pairs.data(), &np), "sgx_match_search_for_triangulation");
        vMatchedPairs.clear();
        for (int i = 0; i < np; i++) vMatchedPairs.emplace_back((size_t)pairs[2 * i], (size_t)pairs[2 * i + 1]);
        return np;
    }
    // int SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches) (ORBmatcher.cc:159-290): matches[j] = keyframe keypoint whose map point keypoint j of F receives
    int SearchByBoW(const KeyFrameView &KF, const FrameView &F, const std::vector<int32_t> &featNodeF, std::vector<int32_t> &matches)
    {
        matches.assign((size_t)(F.N > 0 ? F.N : 1), -1); int32_t n = 0;
        check(sgx_match_search_by_bow(KF.N, KF.mvKeysUn.data(), KF.mDescriptors.data(), KF.hasMapPoint.data(), KF.featNode.data(),
                                      F.N, F.mvKeysUn.data(), F.mDescriptors.data(), featNodeF.data(), mfNNratio, mbCheckOrientation ? 1 : 0, matches.data(), &n), "sgx_match_search_by_bow");
        matches.resize((size_t)F.N);
        return n;
    }
    // the search of int Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th) (ORBmatcher.cc:829-979): bestIdx[i] = keypoint of pKF map point i fuses with (-1: none)
    int Fuse(const KeyFrameView &KF, LocalMapView &M, float th, const sgx_camera &cam, const std::vector<float> &scaleFactors, const std::vector<float> &invLevelSigma2,
             std::vector<int32_t> &bestIdx, std::vector<int32_t> &bestDist)
    {
        bestIdx.assign((size_t)(M.N > 0 ? M.N : 1), -1); bestDist.assign((size_t)(M.N > 0 ? M.N : 1), 256); int32_t n = 0;
        check(sgx_match_fuse_search(KF.N, KF.mvKeysUn.data(), KF.mDescriptors.data(), KF.mvuRight.data(), KF.Tcw, M.N, M.mWorldPos.data(), M.mNormalVector.data(), M.mfMinDistance.data(),
                                    M.mfMaxDistance.data(), M.mDescriptor.data(), M.skip.data(), &cam, scaleFactors.data(), invLevelSigma2.data(), (int)scaleFactors.size(),
                                    std::log(scaleFactors[1]), th, bestIdx.data(), bestDist.data(), &n), "sgx_match_fuse_search");
        bestIdx.resize((size_t)M.N); bestDist.resize((size_t)M.N);
        return n;
    }
    // int SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, const float th, const int ORBdist) (ORBmatcher.cc:1474-1601): M = pKF's map points
    // (M.skip[i] = NULL / isBad() / already found), kfKeysUn = pKF->mvKeysUn; CurrentFrame.mvpMapPoints (>= 0 = holds a point) is read; matched[k] = index into M or -1
    int SearchByProjection(FrameView &CurrentFrame, const std::vector<sgx_keypoint> &kfKeysUn, LocalMapView &M, float th, int ORBdist, const sgx_camera &cam,
                           const std::vector<float> &scaleFactors, std::vector<int32_t> &matched)
    {
        std::vector<uint8_t> held((size_t)(CurrentFrame.N > 0 ? CurrentFrame.N : 1), 0), ok((size_t)(M.N > 0 ? M.N : 1), 0);
        for (int k = 0; k < CurrentFrame.N; k++) held[(size_t)k] = CurrentFrame.mvpMapPoints.size() == (size_t)CurrentFrame.N && CurrentFrame.mvpMapPoints[(size_t)k] >= 0;
        for (int i = 0; i < M.N; i++) ok[(size_t)i] = !M.skip[(size_t)i];
        matched.assign((size_t)(CurrentFrame.N > 0 ? CurrentFrame.N : 1), -1); int32_t n = 0;
        check(sgx_match_project_keyframe(CurrentFrame.N, CurrentFrame.mvKeysUn.data(), CurrentFrame.mDescriptors.data(), held.data(), CurrentFrame.mTcw,
                                         M.N, kfKeysUn.data(), ok.data(), M.mWorldPos.data(), M.mfMinDistance.data(), M.mfMaxDistance.data(), M.mDescriptor.data(),
                                         &cam, scaleFactors.data(), (int)scaleFactors.size(), std::log(scaleFactors[1]), th, ORBdist, mbCheckOrientation ? 1 : 0, matched.data(), &n),
              "sgx_match_project_keyframe");
        matched.resize((size_t)CurrentFrame.N);
        return n;
    }

    // ---- LoopClosing gates (tier N2).  M = candidate map points (M.skip[i] = isBad() / already found / already in pKF); Scw = 4x4 row-major (sRcw | tcw).
    // int SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12) (ORBmatcher.cc:524-655): hasMapPoint = holds a map point that is not bad;
    // vpMatches12[i1] = keypoint of pKF2 whose map point keypoint i1 of pKF1 is matched with (-1: NULL)
    int SearchByBoW(const KeyFrameView &KF1, const KeyFrameView &KF2, std::vector<int32_t> &vpMatches12)
    {
        vpMatches12.assign((size_t)(KF1.N > 0 ? KF1.N : 1), -1); int32_t n = 0;
        check(sgx_match_search_by_bow_kf(KF1.N, KF1.mvKeysUn.data(), KF1.mDescriptors.data(), KF1.hasMapPoint.data(), KF1.featNode.data(),
                                         KF2.N, KF2.mvKeysUn.data(), KF2.mDescriptors.data(), KF2.hasMapPoint.data(), KF2.featNode.data(), mfNNratio, mbCheckOrientation ? 1 : 0,
                                         vpMatches12.data(), &n), "sgx_match_search_by_bow_kf");
        vpMatches12.resize((size_t)KF1.N);
        return n;
    }
    // int SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12, const cv::Mat &t12, const float th)
    // (ORBmatcher.cc:1106-1330).  M1 / M2 = the keyframes' own map points, indexed by keypoint (skip = NULL or bad); vpMatches12 as in include/sgx.h (-1 / >= 0 / -2)
    int SearchBySim3(const KeyFrameView &KF1, LocalMapView &M1, const KeyFrameView &KF2, LocalMapView &M2, std::vector<int32_t> &vpMatches12, float s12, const float R12[9],
                     const float t12[3], float th, const sgx_camera &cam, const std::vector<float> &scaleFactors)
    {
        std::vector<uint8_t> ok1((size_t)(KF1.N > 0 ? KF1.N : 1), 0), ok2((size_t)(KF2.N > 0 ? KF2.N : 1), 0);
        for (int i = 0; i < KF1.N; i++) ok1[(size_t)i] = !M1.skip[(size_t)i];
        for (int i = 0; i < KF2.N; i++) ok2[(size_t)i] = !M2.skip[(size_t)i];
        vpMatches12.resize((size_t)(KF1.N > 0 ? KF1.N : 1), -1); int32_t n = 0;
        check(sgx_match_search_by_sim3(KF1.N, KF1.mvKeysUn.data(), KF1.mDescriptors.data(), KF1.Tcw, ok1.data(), M1.mWorldPos.data(), M1.mfMinDistance.data(), M1.mfMaxDistance.data(), M1.mDescriptor.data(),
                                       KF2.N, KF2.mvKeysUn.data(), KF2.mDescriptors.data(), KF2.Tcw, ok2.data(), M2.mWorldPos.data(), M2.mfMinDistance.data(), M2.mfMaxDistance.data(), M2.mDescriptor.data(),
                                       &cam, scaleFactors.data(), (int)scaleFactors.size(), std::log(scaleFactors[1]), s12, R12, t12, th, vpMatches12.data(), &n), "sgx_match_search_by_sim3");
        vpMatches12.resize((size_t)KF1.N);
        return n;
    }
    // int SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th) (ORBmatcher.cc:292-407):
    // vpMatched[k] >= 0 on entry = slot filled; newly filled slots receive the index into M
    int SearchByProjection(const KeyFrameView &KF, const float Scw[16], LocalMapView &M, std::vector<int32_t> &vpMatched, int th, const sgx_camera &cam, const std::vector<float> &scaleFactors)
    {
        std::vector<uint8_t> held((size_t)(KF.N > 0 ? KF.N : 1), 0);
        for (int k = 0; k < KF.N; k++) held[(size_t)k] = vpMatched.size() == (size_t)KF.N && vpMatched[(size_t)k] >= 0;
        std::vector<int32_t> out((size_t)(KF.N > 0 ? KF.N : 1), -1); int32_t n = 0;
        check(sgx_match_project_sim3(KF.N, KF.mvKeysUn.data(), KF.mDescriptors.data(), held.data(), Scw, M.N, M.mWorldPos.data(), M.mNormalVector.data(), M.mfMinDistance.data(),
                                     M.mfMaxDistance.data(), M.mDescriptor.data(), M.skip.data(), &cam, scaleFactors.data(), (int)scaleFactors.size(), std::log(scaleFactors[1]), th,
                                     out.data(), &n), "sgx_match_project_sim3");
        vpMatched.resize((size_t)KF.N, -1);
        for (int k = 0; k < KF.N; k++) if (out[(size_t)k] >= 0) vpMatched[(size_t)k] = out[(size_t)k];
        return n;
    }
    // the search of int Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, float th, vector<MapPoint*> &vpReplacePoint) (ORBmatcher.cc:981-1101)
    int Fuse(const KeyFrameView &KF, const float Scw[16], LocalMapView &M, float th, const sgx_camera &cam, const std::vector<float> &scaleFactors,
             std::vector<int32_t> &bestIdx, std::vector<int32_t> &bestDist)
    {
        bestIdx.assign((size_t)(M.N > 0 ? M.N : 1), -1); bestDist.assign((size_t)(M.N > 0 ? M.N : 1), 256); int32_t n = 0;
        check(sgx_match_fuse_search_sim3(KF.N, KF.mvKeysUn.data(), KF.mDescriptors.data(), Scw, M.N, M.mWorldPos.data(), M.mNormalVector.data(), M.mfMinDistance.data(),
                                         M.mfMaxDistance.data(), M.mDescriptor.data(), M.skip.data(), &cam, scaleFactors.data(), (int)scaleFactors.size(), std::log(scaleFactors[1]), th,
                                         bestIdx.data(), bestDist.data(), &n), "sgx_match_fuse_search_sim3");
        bestIdx.resize((size_t)M.N); bestDist.resize((size_t)M.N);
        return n;
    }

    // int SearchForInitialization(Frame &F1, Frame &F2, vector<cv::Point2f> &vbPrevMatched, vector<int> &vnMatches12, int windowSize = 10) (ORBmatcher.cc:407-522);
    // vbPrevMatched = N1 x (x, y)
    int SearchForInitialization(const FrameView &F1, const FrameView &F2, std::vector<float> &vbPrevMatched, std::vector<int32_t> &vnMatches12, int windowSize, const sgx_camera &cam)
    {
        vnMatches12.assign((size_t)(F1.N > 0 ? F1.N : 1), -1); int32_t n = 0;
        vbPrevMatched.resize((size_t)2 * (F1.N > 0 ? F1.N : 1));
        check(sgx_match_search_for_initialization(F1.N, F1.mvKeysUn.data(), F1.mDescriptors.data(), F2.N, F2.mvKeysUn.data(), F2.mDescriptors.data(), vbPrevMatched.data(), windowSize,
                                                  mfNNratio, mbCheckOrientation ? 1 : 0, &cam, vnMatches12.data(), &n), "sgx_match_search_for_initialization");
        vnMatches12.resize((size_t)F1.N); vbPrevMatched.resize((size_t)2 * F1.N);
        return n;
    }

protected:
    float mfNNratio; bool mbCheckOrientation;
};

// The numeric steps of LocalMapping / MapPoint that surround the matcher gates and the optimisers, on flattened data
namespace LocalMappingSteps {
    // the per-pair body of LocalMapping::CreateNewMapPoints (LocalMapping.cc:283-421); mvKeys / mvDepth per keyframe; returns nnew, ok[q], x3D[q]
    inline int CreateNewMapPoints(const std::vector<std::pair<size_t, size_t>> &vMatchedIndices,
                                  const ORBmatcher::KeyFrameView &KF1, const std::vector<sgx_keypoint> &mvKeys1, const std::vector<float> &mvDepth1,
                                  const ORBmatcher::KeyFrameView &KF2, const std::vector<sgx_keypoint> &mvKeys2, const std::vector<float> &mvDepth2,
                                  const sgx_camera &cam, const std::vector<float> &scaleFactors, const std::vector<float> &levelSigma2, std::vector<uint8_t> &ok, std::vector<float> &x3D)
    {
        const int np = (int)vMatchedIndices.size();
        std::vector<int32_t> pairs((size_t)2 * (np > 0 ? np : 1));
        for (int i = 0; i < np; i++) { pairs[(size_t)2 * i] = (int32_t)vMatchedIndices[(size_t)i].first; pairs[(size_t)2 * i + 1] = (int32_t)vMatchedIndices[(size_t)i].second; }
        ok.assign((size_t)(np > 0 ? np : 1), 0); x3D.assign((size_t)3 * (np > 0 ? np : 1), 0.f); int32_t nnew = 0;
        check(sgx_triangulate_new_map_points(np, pairs.data(), KF1.N, KF1.mvKeysUn.data(), mvKeys1.data(), KF1.mvuRight.data(), mvDepth1.data(), KF1.Tcw,
                                             KF2.N, KF2.mvKeysUn.data(), mvKeys2.data(), KF2.mvuRight.data(), mvDepth2.data(), KF2.Tcw, &cam, scaleFactors.data(), levelSigma2.data(),
                                             (int)scaleFactors.size(), ok.data(), x3D.data(), &nnew), "sgx_triangulate_new_map_points");
        ok.resize((size_t)np); x3D.resize((size_t)3 * np);
        return nnew;
    }
    // MapPoint::UpdateNormalAndDepth / ComputeDistinctiveDescriptors for a batch of points (MapPoint.cc:330-371, :242-307); observations as CSR in mObservations order
    inline void UpdateNormalAndDepth(const std::vector<float> &xw, const std::vector<int32_t> &obsStart, const std::vector<float> &obsCenter, const std::vector<float> &refCenter,
                                     const std::vector<int32_t> &refLevel, const std::vector<float> &scaleFactors, std::vector<float> &normal, std::vector<float> &minDist, std::vector<float> &maxDist)
    {
        const size_t np_ = refLevel.size();                          // outputs sized here, seeded with the caller's values (points without observations keep them, MapPoint.cc:335-336)
        normal.resize(3 * np_, 0.f); minDist.resize(np_, 0.f); maxDist.resize(np_, 0.f);
        check(sgx_mappoint_update_normal_and_depth((int)refLevel.size(), xw.data(), obsStart.data(), obsCenter.data(), refCenter.data(), refLevel.data(), scaleFactors.data(),
                                                   (int)scaleFactors.size(), normal.data(), minDist.data(), maxDist.data()), "sgx_mappoint_update_normal_and_depth");
    }
    inline void ComputeDistinctiveDescriptors(const std::vector<int32_t> &obsStart, const std::vector<uint8_t> &obsDesc, std::vector<int32_t> &best, std::vector<uint8_t> &mDescriptor)
    {
        const int n = (int)obsStart.size() - 1;
        best.assign((size_t)(n > 0 ? n : 1), -1); mDescriptor.assign((size_t)32 * (n > 0 ? n : 1), 0);
        check(sgx_mappoint_distinctive_descriptors(n, obsStart.data(), obsDesc.data(), best.data(), mDescriptor.data()), "sgx_mappoint_distinctive_descriptors");
        best.resize((size_t)(n > 0 ? n : 0)); mDescriptor.resize((size_t)32 * (n > 0 ? n : 0));
    }
}

// Sim3Solver (src/sg-slam/include/Sim3Solver.h:36-130): constructed from the flattened usable correspondences (what Sim3Solver.cc:40-111 gathers), then the reference's calls
class Sim3Solver {
public:
    // x3dc1 / x3dc2: n x 3 camera-frame points, maxErr1 / maxErr2: 9.210 * mvLevelSigma2[octave], K = (fx, fy, cx, cy), indices1[i] = the i1 of pair i (mvnIndices1), N1 = vpMatched12.size()
    Sim3Solver(const std::vector<float> &x3dc1, const std::vector<float> &x3dc2, const std::vector<float> &maxErr1, const std::vector<float> &maxErr2, const float K1[4], const float K2[4],
               const std::vector<int32_t> &indices1, int N1, bool bFixScale, unsigned randSeed = 0) : idx1_(indices1), N1_(N1), n_((int)maxErr1.size())
    { check(sgx_sim3_solver_create(n_, x3dc1.data(), x3dc2.data(), maxErr1.data(), maxErr2.data(), K1, K2, bFixScale ? 1 : 0, randSeed, &h_), "sgx_sim3_solver_create"); }
    ~Sim3Solver() { if (h_) sgx_sim3_solver_destroy(h_); }
    Sim3Solver(const Sim3Solver &) = delete; Sim3Solver &operator=(const Sim3Solver &) = delete;
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) { check(sgx_sim3_solver_set_ransac_parameters(h_, probability, minInliers, maxIterations), "sgx_sim3_solver_set_ransac_parameters"); }
    // cv::Mat iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers): returns true and fills T12 (4x4 row-major) when a model is found.
    // randDraws (optional): 3 raw rand() values per iteration for callers that share the process-global stream; otherwise the solver's glibc-compatible replica is used.
    bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, float T12[16], const std::vector<int32_t> *randDraws = nullptr)
    {
        std::vector<uint8_t> inl((size_t)(n_ > 0 ? n_ : 1), 0); int32_t nm = 0, ni = 0, fnd = 0;
        check(sgx_sim3_solver_iterate(h_, nIterations, randDraws ? randDraws->data() : nullptr, T12, &nm, inl.data(), &ni, &fnd, nullptr), "sgx_sim3_solver_iterate");
        bNoMore = nm != 0; nInliers = ni; vbInliers.assign((size_t)N1_, false);
        if (fnd) for (int i = 0; i < n_; i++) if (inl[(size_t)i]) vbInliers[(size_t)idx1_[(size_t)i]] = true;           // vbInliers[mvnIndices1[i]] = true (:196-198)
        return fnd != 0;
    }
    void GetEstimate(float R12[9], float t12[3], float &scale) const { check(sgx_sim3_solver_get_estimate(h_, R12, t12, &scale, nullptr), "sgx_sim3_solver_get_estimate"); }
private:
    sgx_sim3_solver *h_ = nullptr; std::vector<int32_t> idx1_; int N1_, n_;
};

// PnPsolver (src/sg-slam/src/PnPsolver.cc), the EPnP RANSAC of Tracking::Relocalization (Tracking.cc:1504-1530), on the device
class PnPsolver {
public:
    // the constructor's flattening (:78-101): p2d = mvKeysUn[i].pt (n x 2), sigma2 = mvLevelSigma2[octave], p3dw = GetWorldPos() (n x 3), keyPointIndices[k] = i
    // (mvKeyPointIndices), N = vpMapPointMatches.size(); cam = fx, fy, cx, cy.  Ends with SetRansacParameters() and its defaults, as the reference does.
    PnPsolver(const std::vector<float> &p2d, const std::vector<float> &sigma2, const std::vector<float> &p3dw, const float cam[4], const std::vector<int32_t> &keyPointIndices,
              int N, unsigned randSeed = 0) : idx_(keyPointIndices), N_(N), n_((int)sigma2.size())
    { check(sgx_pnp_solver_create(n_, p2d.data(), sigma2.data(), p3dw.data(), cam, randSeed, &h_), "sgx_pnp_solver_create"); }
    ~PnPsolver() { if (h_) sgx_pnp_solver_destroy(h_); }
    PnPsolver(const PnPsolver &) = delete; PnPsolver &operator=(const PnPsolver &) = delete;
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f, float th2 = 5.991f)
    { check(sgx_pnp_solver_set_ransac_parameters(h_, probability, minInliers, maxIterations, minSet, epsilon, th2), "sgx_pnp_solver_set_ransac_parameters"); }
    // cv::Mat iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers): returns true and fills Tcw (4x4 row-major) when a model is returned.
    // randDraws (optional): 4 raw rand() values per hypothesis of the call; otherwise the solver's glibc-compatible replica is used.
    bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, float Tcw[16], const std::vector<int32_t> *randDraws = nullptr)
    {
        std::vector<uint8_t> inl((size_t)(n_ > 0 ? n_ : 1), 0); int32_t nm = 0, ni = 0, fnd = 0;
        check(sgx_pnp_solver_iterate(h_, nIterations, randDraws ? randDraws->data() : nullptr, Tcw, &nm, inl.data(), &ni, &fnd, nullptr), "sgx_pnp_solver_iterate");
        bNoMore = nm != 0; nInliers = ni; vbInliers.assign((size_t)N_, false);
        if (fnd) for (int i = 0; i < n_; i++) if (inl[(size_t)i]) vbInliers[(size_t)idx_[(size_t)i]] = true;            // vbInliers[mvKeyPointIndices[i]] = true (:229-234)
        return fnd != 0;
    }
    // cv::Mat find(vector<bool> &vbInliers, int &nInliers) (:159-163)
    bool find(std::vector<bool> &vbInliers, int &nInliers, float Tcw[16])
    {
        int32_t maxIts = 0; check(sgx_pnp_solver_get_estimate(h_, nullptr, &maxIts, nullptr, nullptr, nullptr), "sgx_pnp_solver_get_estimate");
        bool bFlag = false; return iterate(maxIts, bFlag, vbInliers, nInliers, Tcw);
    }
private:
    sgx_pnp_solver *h_ = nullptr; std::vector<int32_t> idx_; int N_, n_;
};

// Initializer (src/sg-slam/include/Initializer.h:32-96), the two-view initialisation of Tracking::MonocularInitialization (Tracking.cc:605-671), on the device
class Initializer {
public:
    // Initializer(const Frame &ReferenceFrame, float sigma = 1.0, int iterations = 200): K = (fx, fy, cx, cy) is ReferenceFrame.mK, mvKeys1 = ReferenceFrame.mvKeysUn
    Initializer(const FrameView &ReferenceFrame, const float K[4], float sigma = 1.0f, int iterations = 200, unsigned randSeed = 0) : n1_(ReferenceFrame.N)
    { check(sgx_initializer_create(n1_, ReferenceFrame.mvKeysUn.data(), K, sigma, iterations, randSeed, &h_), "sgx_initializer_create"); }
    ~Initializer() { if (h_) sgx_initializer_destroy(h_); }
    Initializer(const Initializer &) = delete; Initializer &operator=(const Initializer &) = delete;
    // bool Initialize(const Frame &CurrentFrame, const vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21, vector<cv::Point3f> &vP3D, vector<bool> &vbTriangulated):
    // R21 3 x 3 row-major, vP3D n1 x 3; the outputs are written on success only, as in the reference.  randDraws (optional): the 8 x iterations raw rand() values of
    // mvSets for callers that share the process-global stream; otherwise the object's glibc-compatible replica is used.  report (optional): scores, model, per-hypothesis counts.
    bool Initialize(const FrameView &CurrentFrame, const std::vector<int32_t> &vMatches12, float R21[9], float t21[3], std::vector<float> &vP3D, std::vector<bool> &vbTriangulated,
                    const std::vector<int32_t> *randDraws = nullptr, sgx_init_report *report = nullptr)
    {
        if ((int)vMatches12.size() != n1_) throw std::runtime_error("Initializer::Initialize: vMatches12 has one entry per key of the reference frame");
        const size_t n = (size_t)(n1_ > 0 ? n1_ : 1);
        std::vector<float> p3d(3 * n, 0.f); std::vector<uint8_t> tri(n, 0), inl(n, 0); float R[9], t[3]; int32_t ok = 0;
        check(sgx_initializer_initialize(h_, CurrentFrame.N, CurrentFrame.mvKeysUn.data(), vMatches12.data(), randDraws ? randDraws->data() : nullptr, R, t, p3d.data(), tri.data(),
                                         inl.data(), &ok, report), "sgx_initializer_initialize");
        if (!ok) return false;
        std::memcpy(R21, R, sizeof R); std::memcpy(t21, t, sizeof t);
        vP3D.assign(p3d.begin(), p3d.begin() + 3 * (size_t)n1_); vbTriangulated.assign((size_t)n1_, false);
        for (int i = 0; i < n1_; i++) vbTriangulated[(size_t)i] = tri[(size_t)i] != 0;
        return true;
    }
private:
    sgx_initializer *h_ = nullptr; int n1_;
};

// ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (src/sg-slam/include/ORBVocabulary.h:31-32): the members the reference calls
class ORBVocabulary {
public:
    typedef std::vector<std::pair<int32_t, double>> BowVector;       // DBoW2::BowVector (std::map<WordId, WordValue>) in key order
    ORBVocabulary() {}
    ~ORBVocabulary() { if (h_) sgx_voc_destroy(h_); }
    ORBVocabulary(const ORBVocabulary &) = delete; ORBVocabulary &operator=(const ORBVocabulary &) = delete;
    bool loadFromTextFile(const std::string &filename) { return filename.size() >= 4 && filename.compare(filename.size() - 4, 4, ".txt") == 0 && load(filename); }
    bool loadFromBinaryFile(const std::string &filename) { return !(filename.size() >= 4 && filename.compare(filename.size() - 4, 4, ".txt") == 0) && load(filename); }
    bool empty() const { return size() == 0; }
    unsigned size() const { int32_t nw = 0; if (h_) sgx_voc_info(h_, nullptr, nullptr, nullptr, nullptr, nullptr, &nw); return (unsigned)nw; }
    // void transform(const vector<TDescriptor>& features, BowVector &v, FeatureVector &fv, int levelsup) (TemplatedVocabulary.h:1139-1206); descriptors = N x 32 bytes;
    // featNode[i] = the key of fv under which feature i sits (-1: stopped word) — KeyFrameView::featNode / the featNodeF argument of SearchByBoW
    void transform(const std::vector<uint8_t> &descriptors, BowVector &v, std::vector<int32_t> &featNode, int levelsup) const
    {
        const int n = (int)(descriptors.size() / 32);
        std::vector<int32_t> ids((size_t)(n > 0 ? n : 1)); std::vector<double> w((size_t)(n > 0 ? n : 1)); int32_t nb = 0;
        featNode.assign((size_t)(n > 0 ? n : 1), -1);
        check(sgx_voc_transform(h_, n, descriptors.data(), levelsup, ids.data(), w.data(), &nb, featNode.data(), nullptr), "sgx_voc_transform");
        featNode.resize((size_t)n); v.clear();
        for (int i = 0; i < nb; i++) v.emplace_back(ids[(size_t)i], w[(size_t)i]);
    }
    // double score(const BowVector &a, const BowVector &b) (:1210-1215)
    double score(const BowVector &a, const BowVector &b) const
    {
        std::vector<int32_t> ia, ib; std::vector<double> wa, wb;
        for (auto &e : a) { ia.push_back(e.first); wa.push_back(e.second); }
        for (auto &e : b) { ib.push_back(e.first); wb.push_back(e.second); }
        double s = 0;
        check(sgx_voc_score(h_, (int)ia.size(), ia.data(), wa.data(), (int)ib.size(), ib.data(), wb.data(), &s), "sgx_voc_score");
        return s;
    }
    sgx_voc *handle() const { return h_; }
private:
    bool load(const std::string &f) { sgx_voc *h = nullptr; if (sgx_voc_load(f.c_str(), &h) != SGX_OK) return false; if (h_) sgx_voc_destroy(h_); h_ = h; return true; }
    sgx_voc *h_ = nullptr;
};

// KeyFrameDatabase (src/sg-slam/include/KeyFrameDatabase.h:41-68) over sgx_kfdb_*: the database on the device.  Where the reference passes KeyFrame* / Frame*, this mirror
// takes what it reads of them: the keyframe's mnId and mBowVec, the query's mBowVec and, for a loop query, pKF->GetConnectedKeyFrames() as ids.  Candidates come back as
// mnIds in the reference's order.  The covisibility the accumulation reads (pKFi->GetBestCovisibilityKeyFrames(10), KeyFrameDatabase.cc:151, :265) lives in the caller's
// graph: setBestCovisibilityKeyFrames hands it over whenever the graph changes (KeyFrame::UpdateBestCovisibles, KeyFrame.cc:139-173).
class KeyFrameDatabase {
public:
    typedef ORBVocabulary::BowVector BowVector;
    KeyFrameDatabase(const ORBVocabulary &voc, int maxKeyFrames = 4096, int maxBowEntries = 0, int maxQueryWords = 0, int maxQueries = 64) : cap_(maxKeyFrames)
    { check(sgx_kfdb_create(voc.handle(), maxKeyFrames, maxBowEntries > 0 ? maxBowEntries : 1024 * maxKeyFrames, maxQueryWords, maxQueries, &h_), "sgx_kfdb_create"); }
    ~KeyFrameDatabase() { if (h_) sgx_kfdb_destroy(h_); }
    KeyFrameDatabase(const KeyFrameDatabase &) = delete; KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;
    void add(int32_t mnId, const BowVector &mBowVec)                           // void add(KeyFrame *pKF) (:40-46)
    { std::vector<int32_t> i; std::vector<double> w; split(mBowVec, i, w); check(sgx_kfdb_add(h_, mnId, (int)i.size(), i.data(), w.data()), "sgx_kfdb_add"); }
    void erase(int32_t mnId) { check(sgx_kfdb_erase(h_, mnId), "sgx_kfdb_erase"); }      // void erase(KeyFrame *pKF) (:48-67)
    void clear() { check(sgx_kfdb_clear(h_), "sgx_kfdb_clear"); }                          // (:69-73)
    int size() const { return sgx_kfdb_size(h_); }
    void setBestCovisibilityKeyFrames(int32_t mnId, const std::vector<int32_t> &vpNeighs)
    { check(sgx_kfdb_set_covisibility(h_, mnId, (int)vpNeighs.size(), vpNeighs.data()), "sgx_kfdb_set_covisibility"); }
    // std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame *pKF, float minScore) (:76-197)
    std::vector<int32_t> DetectLoopCandidates(const BowVector &mBowVec, const std::vector<int32_t> &spConnectedKeyFrames, float minScore, sgx_kfdb_report *report = nullptr)
    {
        std::vector<int32_t> i; std::vector<double> w; split(mBowVec, i, w);
        std::vector<int32_t> cand((size_t)cap_); int32_t n = 0;
        check(sgx_kfdb_detect_loop_candidates(h_, (int)i.size(), i.data(), w.data(), (int)spConnectedKeyFrames.size(), spConnectedKeyFrames.data(), minScore, cand.data(), &n, report),
              "sgx_kfdb_detect_loop_candidates");
        cand.resize((size_t)n); return cand;
    }
    // std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame *F) (:199-309)
    std::vector<int32_t> DetectRelocalizationCandidates(const BowVector &mBowVec, sgx_kfdb_report *report = nullptr)
    {
        std::vector<int32_t> i; std::vector<double> w; split(mBowVec, i, w);
        std::vector<int32_t> cand((size_t)cap_); int32_t n = 0;
        check(sgx_kfdb_detect_relocalization_candidates(h_, (int)i.size(), i.data(), w.data(), cand.data(), &n, report), "sgx_kfdb_detect_relocalization_candidates");
        cand.resize((size_t)n); return cand;
    }
    // the minScore of LoopClosing::DetectLoop (LoopClosing.cc:126-138) over the covisible keyframes that are not isBad()
    float MinScore(const BowVector &mBowVec, const std::vector<int32_t> &vpConnectedKeyFrames)
    {
        std::vector<int32_t> i; std::vector<double> w; split(mBowVec, i, w); float m = 1.0f;
        check(sgx_kfdb_min_score(h_, (int)i.size(), i.data(), w.data(), (int)vpConnectedKeyFrames.size(), vpConnectedKeyFrames.data(), &m), "sgx_kfdb_min_score");
        return m;
    }
    sgx_kfdb *handle() const { return h_; }
private:
    static void split(const BowVector &v, std::vector<int32_t> &i, std::vector<double> &w) { for (auto &e : v) { i.push_back(e.first); w.push_back(e.second); } }
    sgx_kfdb *h_ = nullptr; int cap_;
};

// The covisibility graph over sgx_covis_*: what KeyFrame / MapPoint keep of the relation "keyframe observes map point at keypoint index" (mvpMapPoints, mObservations,
// nObs, mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, the spanning tree) on the device.  Where the reference passes KeyFrame* / MapPoint*, this mirror takes
// the keyframe's mnId and the point's dense handle.  The host-array queries below run a batch of one; the *_batch_dev entries take device arrays through handle().
class CovisibilityGraph {
public:
    struct LocalMap { std::vector<int32_t> mvpMapPoints, mvpLocalKeyFrames, mvpLocalMapPoints, observations; int32_t mpReferenceKF = -1, trackedMapPoints = 0; sgx_covis_report report{}; };
    struct CullingVote { int32_t mnId, nRedundantObservations, nMPs, cull; };
    CovisibilityGraph(int maxKeyFrames, int cap, int maxPoints, int maxObservations, int maxQueries = 64, bool mbMonocular = false, float mThDepth = 40.0f)
        : maxkf_(maxKeyFrames), cap_(cap)
    { check(sgx_covis_create(maxKeyFrames, cap, maxPoints, maxObservations, maxQueries, mbMonocular ? 1 : 0, mThDepth, &h_), "sgx_covis_create"); }
    ~CovisibilityGraph() { if (h_) sgx_covis_destroy(h_); }
    CovisibilityGraph(const CovisibilityGraph &) = delete; CovisibilityGraph &operator=(const CovisibilityGraph &) = delete;
    // ---- mutations
    void AddKeyFrame(int32_t mnId, const std::vector<int32_t> &octave, const std::vector<float> &mvuRight, const std::vector<float> &mvDepth)
    { check(sgx_covis_add_keyframe(h_, mnId, (int)octave.size(), octave.data(), mvuRight.data(), mvDepth.data()), "sgx_covis_add_keyframe"); }
    void AddMapPoint(int32_t mnId, int32_t idx, int32_t point) { check(sgx_covis_set_observations(h_, mnId, 1, &idx, &point), "sgx_covis_set_observations"); }      // KeyFrame::AddMapPoint + MapPoint::AddObservation
    void EraseMapPointMatch(int32_t mnId, int32_t idx) { const int32_t none = -1; check(sgx_covis_set_observations(h_, mnId, 1, &idx, &none), "sgx_covis_set_observations"); }
    void SetObservations(int32_t mnId, const std::vector<int32_t> &idx, const std::vector<int32_t> &points)
    { check(idx.size() == points.size() ? sgx_covis_set_observations(h_, mnId, (int)idx.size(), idx.data(), points.data()) : SGX_ERR_INVALID, "sgx_covis_set_observations"); }
    void SetBadFlag(const std::vector<int32_t> &points) { check(sgx_covis_set_points_bad(h_, (int)points.size(), points.data()), "sgx_covis_set_points_bad"); }      // MapPoint::SetBadFlag
    void Replace(int32_t oldPoint, int32_t newPoint) { check(sgx_covis_replace_point(h_, oldPoint, newPoint), "sgx_covis_replace_point"); }                          // MapPoint::Replace
    void EraseKeyFrame(int32_t mnId) { check(sgx_covis_erase_keyframe(h_, mnId), "sgx_covis_erase_keyframe"); }                                                      // KeyFrame::SetBadFlag
    void clear() { check(sgx_covis_clear(h_), "sgx_covis_clear"); }
    int size() const { return sgx_covis_size(h_); }
    // ---- getters
    std::vector<std::pair<int32_t, int32_t>> GetConnectedKeyFrameWeights(int32_t mnId) { return pairs(sgx_covis_get_weights, mnId, "sgx_covis_get_weights"); }
    std::vector<std::pair<int32_t, int32_t>> GetOrderedConnectedKeyFrames(int32_t mnId) { return pairs(sgx_covis_get_ordered, mnId, "sgx_covis_get_ordered"); }      // (keyframe, weight)
    std::vector<int32_t> GetBestCovisibilityKeyFrames(int32_t mnId, int N)
    {
        std::vector<int32_t> v((size_t)(N > 0 ? N : 1)); int32_t n = 0;
        check(sgx_covis_best_covisibles(h_, mnId, N, v.data(), &n), "sgx_covis_best_covisibles");
        v.resize((size_t)n); return v;
    }
    int32_t GetParent(int32_t mnId) { int32_t p = -1; check(sgx_covis_get_tree(h_, mnId, &p, nullptr, nullptr, nullptr), "sgx_covis_get_tree"); return p; }
    std::vector<int32_t> GetChilds(int32_t mnId)
    {
        std::vector<int32_t> c((size_t)maxkf_); int32_t n = 0;
        check(sgx_covis_get_tree(h_, mnId, nullptr, nullptr, c.data(), &n), "sgx_covis_get_tree");
        c.resize((size_t)n); return c;
    }
    std::vector<std::pair<int32_t, int32_t>> GetObservations(int32_t point, int32_t *nObs = nullptr)                                                              // (keyframe, index)
    {
        std::vector<int32_t> a((size_t)maxkf_), b((size_t)maxkf_); int32_t n = 0;
        check(sgx_covis_get_observations(h_, point, a.data(), b.data(), &n, nObs), "sgx_covis_get_observations");
        std::vector<std::pair<int32_t, int32_t>> v; for (int32_t j = 0; j < n; j++) v.emplace_back(a[(size_t)j], b[(size_t)j]);
        return v;
    }
    // ---- the queries, a batch of one from host arrays (device arrays: the sgx_covis_*_batch_dev entries on handle())
    sgx_covis_report UpdateConnections(int32_t mnId)                            // KeyFrame::UpdateConnections (KeyFrame.cc:290-380)
    { sgx_covis_report r{}; check(sgx_covis_update_connections(h_, mnId, &r), "sgx_covis_update_connections"); return r; }
    // Tracking::UpdateLocalMap (Tracking.cc:1314-1458): the frame's mvpMapPoints, mvpLocalKeyFrames and mpReferenceKF go in and come back; more than mcap local points throw
    LocalMap UpdateLocalMap(const std::vector<int32_t> &mvpMapPoints, int minObs, const std::vector<int32_t> &mvpLocalKeyFrames, int32_t mpReferenceKF, int mcap = 4096)
    {
        LocalMap L; L.mvpMapPoints = mvpMapPoints; L.mvpLocalKeyFrames = mvpLocalKeyFrames; L.mpReferenceKF = mpReferenceKF;
        int32_t nk = (int32_t)mvpLocalKeyFrames.size(), np = 0;
        if (nk > maxkf_ || mcap < 1) check(SGX_ERR_INVALID, "UpdateLocalMap");
        L.mvpLocalKeyFrames.resize((size_t)maxkf_); L.mvpLocalMapPoints.resize((size_t)mcap); L.observations.resize((size_t)mcap);
        check(sgx_covis_local_map(h_, (int)L.mvpMapPoints.size(), L.mvpMapPoints.data(), minObs, L.mvpLocalKeyFrames.data(), &nk, &L.mpReferenceKF, &L.trackedMapPoints, mcap,
                                  L.mvpLocalMapPoints.data(), L.observations.data(), &np, &L.report), "sgx_covis_local_map");
        L.mvpLocalKeyFrames.resize((size_t)nk); L.mvpLocalMapPoints.resize((size_t)np); L.observations.resize((size_t)np);
        return L;
    }
    // the votes of LocalMapping::KeyFrameCulling (LocalMapping.cc:632-696) for the current keyframe against the map as it stands
    std::vector<CullingVote> KeyFrameCullingVotes(int32_t mnId)
    {
        std::vector<int32_t> a((size_t)maxkf_), b((size_t)maxkf_), c((size_t)maxkf_), d((size_t)maxkf_); int32_t n = 0;
        check(sgx_covis_keyframe_culling(h_, mnId, maxkf_, a.data(), &n, b.data(), c.data(), d.data()), "sgx_covis_keyframe_culling");
        std::vector<CullingVote> v; for (int32_t j = 0; j < n; j++) v.push_back(CullingVote{a[(size_t)j], b[(size_t)j], c[(size_t)j], d[(size_t)j]});
        return v;
    }
    // LocalMapping::KeyFrameCulling with its SetBadFlag between the candidates: query, erase the first voted candidate, query again, go on behind it in the first list
    std::vector<int32_t> KeyFrameCulling(int32_t mnId)
    {
        std::vector<CullingVote> votes = KeyFrameCullingVotes(mnId);
        std::vector<int32_t> first, erased; for (const CullingVote &v : votes) first.push_back(v.mnId);
        for (size_t pos = 0; pos < first.size(); pos++) {
            bool voted = false;
            for (const CullingVote &v : votes) if (v.mnId == first[pos] && v.cull) voted = true;
            if (!voted) continue;
            EraseKeyFrame(first[pos]); erased.push_back(first[pos]);
            votes = KeyFrameCullingVotes(mnId);
        }
        return erased;
    }
    // The graph of Optimizer::LocalBundleAdjustment(keyframe mnId) (Optimizer.cc:453-504, :572-653), or with mode = SGX_COVIS_BA_GLOBAL that of
    // Optimizer::BundleAdjustment over the whole map (:49-150; mnId is not read): the index arrays of sgx_ba_problem.  Two calls: the counts, then rows of exactly the need.
    struct BaGraph {
        std::vector<int32_t> pose_id, point_id, point_edge_begin, edge_pose, edge_point, edge_kp; std::vector<uint8_t> pose_fixed, edge_attr; sgx_covis_ba_report report{};
    };
    BaGraph ba_graph(int32_t mnId, int mode = SGX_COVIS_BA_LOCAL)
    {
        BaGraph g; g.pose_id.resize((size_t)maxkf_); g.pose_fixed.resize((size_t)maxkf_); g.point_edge_begin.resize(1);
        int rc = sgx_covis_ba_graph(h_, mode, mnId, g.pose_id.data(), g.pose_fixed.data(), 0, nullptr, g.point_edge_begin.data(), 0, nullptr, nullptr, nullptr, nullptr, &g.report);
        if (rc != SGX_OK && rc != SGX_ERR_NOMEM) check(rc, "sgx_covis_ba_graph");
        const size_t np = (size_t)g.report.n_points, ne = (size_t)g.report.n_edges;
        g.point_id.resize(np); g.point_edge_begin.resize(np + 1); g.edge_pose.resize(ne); g.edge_point.resize(ne); g.edge_kp.resize(ne); g.edge_attr.resize(ne);
        if (rc != SGX_OK)
            check(sgx_covis_ba_graph(h_, mode, mnId, g.pose_id.data(), g.pose_fixed.data(), (int)np, g.point_id.data(), g.point_edge_begin.data(), (int)ne, g.edge_pose.data(),
                                     g.edge_point.data(), g.edge_kp.data(), g.edge_attr.data(), &g.report), "sgx_covis_ba_graph");
        g.pose_id.resize((size_t)g.report.n_poses); g.pose_fixed.resize((size_t)g.report.n_poses);
        return g;
    }
    // vToErase (Optimizer.cc:711-757) into the relation: the flagged monocular edges in edge order, then the flagged stereo ones, each EraseMapPointMatch +
    // EraseObservation with its SetBadFlag at nObs <= 2.  erase: the flags sgx_local_bundle_adjustment returned for the problem flattened from g.
    void apply_ba_erase(const BaGraph &g, const std::vector<uint8_t> &erase)
    {
        if (erase.size() != g.edge_pose.size()) check(SGX_ERR_INVALID, "apply_ba_erase");
        for (int stereo = 0; stereo < 2; stereo++)
            for (size_t j = 0; j < erase.size(); j++)
                if (erase[j] && ((g.edge_attr[j] & SGX_COVIS_ATTR_RIGHT) != 0) == (stereo != 0)) EraseMapPointMatch(g.pose_id[(size_t)g.edge_pose[j]], g.edge_kp[j]);
    }
    // Loop closing (LoopClosing::CorrectLoop, LoopClosing.cc:432-573, and the graph of Optimizer::OptimizeEssentialGraph, Optimizer.cc:797-983): mspLoopEdges, the group
    // with the point marks, LoopConnections after the caller's fusion, and the vertices and edges of the essential graph.  Two calls where a need is not known.
    void AddLoopEdge(int32_t a, int32_t b) { check(sgx_covis_add_loop_edge(h_, a, b), "sgx_covis_add_loop_edge"); }
    std::vector<int32_t> GetLoopEdges(int32_t mnId)
    {
        std::vector<int32_t> v((size_t)maxkf_); int32_t n = 0;
        check(sgx_covis_get_loop_edges(h_, mnId, v.data(), &n), "sgx_covis_get_loop_edges"); v.resize((size_t)n);
        return v;
    }
    // LoopClosing::DetectLoop (LoopClosing.cc:103-229) on the handle: GetConnectedKeyFrames() of a keyframe in ascending id (what DetectLoopCandidates excludes), the
    // consistency groups mvConsistentGroups as state of the handle, and the map update of RunGlobalBundleAdjustment (:676-737).
    std::vector<int32_t> GetConnectedKeyFrames(int32_t mnId)
    {
        int32_t off[2] = { 0, 0 }; sgx_covis_report rep{};
        int rc = sgx_covis_connected_batch(h_, 1, &mnId, off, nullptr, 0, &rep);
        if (rc != SGX_OK && rc != SGX_ERR_NOMEM) check(rc, "sgx_covis_connected_batch");
        std::vector<int32_t> ids((size_t)off[1]);
        if (off[1]) check(sgx_covis_connected_batch(h_, 1, &mnId, off, ids.data(), off[1], &rep), "sgx_covis_connected_batch");
        return ids;
    }
    struct ConsistentGroup { std::vector<int32_t> first; int32_t second = 0; };      // ConsistentGroup = pair<set<KeyFrame*>, int>
    void ReserveConsistentGroups(int maxGroups) { check(sgx_covis_consistency_reserve(h_, maxGroups), "sgx_covis_consistency_reserve"); }
    void ClearConsistentGroups() { check(sgx_covis_consistency_clear(h_), "sgx_covis_consistency_clear"); }
    // :152-211 for vpCandidateKFs; returns mvpEnoughConsistentCandidates (an empty candidate list clears the groups, :147)
    std::vector<int32_t> CheckConsistency(const std::vector<int32_t> &vpCandidateKFs, int mnCovisibilityConsistencyTh = 3, sgx_covis_consistency_report *report = nullptr)
    {
        std::vector<int32_t> enough(vpCandidateKFs.size() + 1); int32_t n = 0;
        check(sgx_covis_consistency(h_, (int)vpCandidateKFs.size(), vpCandidateKFs.data(), mnCovisibilityConsistencyTh, enough.data(), &n, report), "sgx_covis_consistency");
        enough.resize((size_t)n);
        return enough;
    }
    std::vector<ConsistentGroup> GetConsistentGroups()
    {
        int64_t bytes = 0; int32_t n = 0, G = 0;
        check(sgx_covis_consistency_info(h_, &bytes, &n, &G), "sgx_covis_consistency_info");
        std::vector<int32_t> cnt((size_t)G + 1), off((size_t)G + 1), ids((size_t)n * (size_t)maxkf_ + 1);
        check(sgx_covis_get_consistent_groups(h_, &n, cnt.data(), off.data(), (int)ids.size(), ids.data()), "sgx_covis_get_consistent_groups");
        std::vector<ConsistentGroup> out((size_t)n);
        for (int g = 0; g < n; g++) { out[(size_t)g].first.assign(ids.begin() + off[(size_t)g], ids.begin() + off[(size_t)g + 1]); out[(size_t)g].second = cnt[(size_t)g]; }
        return out;
    }
    // :676-737: kf_ids lists every live keyframe once; Tcw / TcwGBA 12 floats per row; point rows as sgx_gba_correct_points takes them (ref = a row or -1)
    struct GbaUpdate { std::vector<float> Tcw, TcwBef, xw; std::vector<uint8_t> kf_state; sgx_covis_gba_report report{}; };
    GbaUpdate GlobalBundleAdjustmentUpdate(const std::vector<int32_t> &origins, const std::vector<int32_t> &kf_ids, const std::vector<uint8_t> &in_gba, const std::vector<float> &Tcw,
                                           const std::vector<float> &TcwGBA, const std::vector<float> &xw, const std::vector<uint8_t> &point_in_gba, const std::vector<float> &xw_gba,
                                           const std::vector<int32_t> &point_ref)
    {
        GbaUpdate u; const size_t nk = kf_ids.size(), np = point_ref.size();
        if (in_gba.size() != nk || Tcw.size() != 12 * nk || TcwGBA.size() != 12 * nk || xw.size() != 3 * np || xw_gba.size() != 3 * np || point_in_gba.size() != np) check(SGX_ERR_INVALID, "GlobalBundleAdjustmentUpdate");
        u.Tcw.assign(12 * nk, 0.f); u.TcwBef.assign(12 * nk, 0.f); u.kf_state.assign(nk, 0); u.xw = xw;
        check(sgx_covis_gba_update(h_, (int)origins.size(), origins.data(), (int)nk, kf_ids.data(), in_gba.data(), Tcw.data(), TcwGBA.data(), u.Tcw.data(), u.TcwBef.data(),
                                   u.kf_state.data(), &u.report), "sgx_covis_gba_update");
        if (np) check(sgx_gba_correct_points((int)np, xw.data(), point_in_gba.data(), xw_gba.data(), point_ref.data(), (int)nk, u.kf_state.data(), u.TcwBef.data(), u.Tcw.data(),
                                             u.xw.data()), "sgx_gba_correct_points");      // :705-736 through sgx_gba_correct_points_dev
        return u;
    }
    struct LoopGroup { std::vector<int32_t> group_id, group_vertex, point_id, point_ref; sgx_covis_loop_report report{}; };
    LoopGroup loop_begin(int32_t cur)
    {
        LoopGroup g; g.group_id.resize((size_t)maxkf_); g.group_vertex.resize((size_t)maxkf_);
        int rc = sgx_covis_loop_begin(h_, cur, g.group_id.data(), g.group_vertex.data(), 0, nullptr, nullptr, &g.report);
        if (rc != SGX_OK && rc != SGX_ERR_NOMEM) check(rc, "sgx_covis_loop_begin");
        const size_t np = (size_t)g.report.n_points;
        g.point_id.resize(np); g.point_ref.resize(np);
        if (rc != SGX_OK) check(sgx_covis_loop_begin(h_, cur, g.group_id.data(), g.group_vertex.data(), (int)np, g.point_id.data(), g.point_ref.data(), &g.report), "sgx_covis_loop_begin");
        g.group_id.resize((size_t)g.report.n_group); g.group_vertex.resize((size_t)g.report.n_group);
        return g;
    }
    struct LoopConnections { std::vector<int32_t> lc_begin, lc_j; sgx_covis_loop_report report{}; };
    LoopConnections loop_connections(int32_t cur, const std::vector<int32_t> &group_id)      // one call: a second one would find the lists the first one left
    {
        LoopConnections c; c.lc_begin.resize(group_id.size() + 1); c.lc_j.resize(group_id.size() * (size_t)maxkf_);
        check(sgx_covis_loop_connections(h_, cur, (int)group_id.size(), group_id.data(), (int)c.lc_j.size(), c.lc_begin.data(), c.lc_j.data(), &c.report), "sgx_covis_loop_connections");
        c.lc_j.resize((size_t)c.report.n_connections);
        return c;
    }
    struct EssentialGraph { std::vector<int32_t> vertex_id, vertex_group, e_i, e_j; std::vector<uint8_t> vertex_fixed, e_kind; sgx_covis_loop_report report{}; };
    EssentialGraph essential_graph(int32_t cur, int32_t loop, const std::vector<int32_t> &group_id, const std::vector<int32_t> &lc_begin, const std::vector<int32_t> &lc_j)
    {
        EssentialGraph g; g.vertex_id.resize((size_t)maxkf_); g.vertex_group.resize((size_t)maxkf_); g.vertex_fixed.resize((size_t)maxkf_);
        if (lc_begin.size() != group_id.size() + 1 || (size_t)lc_begin.back() != lc_j.size()) check(SGX_ERR_INVALID, "essential_graph");
        int rc = sgx_covis_essential_graph(h_, cur, loop, (int)group_id.size(), group_id.data(), lc_begin.data(), lc_j.data(), g.vertex_id.data(), g.vertex_fixed.data(),
                                           g.vertex_group.data(), 0, nullptr, nullptr, nullptr, &g.report);
        if (rc != SGX_OK && rc != SGX_ERR_NOMEM) check(rc, "sgx_covis_essential_graph");
        const size_t ne = (size_t)g.report.n_edges;
        g.e_i.resize(ne); g.e_j.resize(ne); g.e_kind.resize(ne);
        if (rc != SGX_OK)
            check(sgx_covis_essential_graph(h_, cur, loop, (int)group_id.size(), group_id.data(), lc_begin.data(), lc_j.data(), g.vertex_id.data(), g.vertex_fixed.data(),
                                            g.vertex_group.data(), (int)ne, g.e_i.data(), g.e_j.data(), g.e_kind.data(), &g.report), "sgx_covis_essential_graph");
        g.vertex_id.resize((size_t)g.report.n_vertices); g.vertex_group.resize((size_t)g.report.n_vertices); g.vertex_fixed.resize((size_t)g.report.n_vertices);
        return g;
    }
    sgx_covis *handle() const { return h_; }
private:
    template <class F> std::vector<std::pair<int32_t, int32_t>> pairs(F fn, int32_t mnId, const char *what)
    {
        std::vector<int32_t> a((size_t)maxkf_), b((size_t)maxkf_); int32_t n = 0;
        check(fn(h_, mnId, a.data(), b.data(), &n), what);
        std::vector<std::pair<int32_t, int32_t>> v; for (int32_t j = 0; j < n; j++) v.emplace_back(a[(size_t)j], b[(size_t)j]);
        return v;
    }
    sgx_covis *h_ = nullptr; int maxkf_, cap_;
};

// the two OpenCV calls of Frame::RmDynamicPointWithSemanticAndGeometry (Frame.cc:445, :469-472)
class OpticalFlowLK {                                                // cv::calcOpticalFlowPyrLK(cur, prev, pts, nextPts, status, err, Size(21,21), 3, TermCriteria(ITER|EPS, 30, 0.01))
public:
    OpticalFlowLK(int width, int height) : w_(width) { sgx_flow_config c{width, height, 1, 21, 3, 30, 0.01}; check(sgx_flow_create(&c, &h_), "sgx_flow_create"); }
    ~OpticalFlowLK() { if (h_) sgx_flow_destroy(h_); }
    OpticalFlowLK(const OpticalFlowLK &) = delete; OpticalFlowLK &operator=(const OpticalFlowLK &) = delete;
    void operator()(const uint8_t *imFrom, const uint8_t *imTo, const std::vector<float> &pts /* x0 y0 x1 y1 .. */, std::vector<float> &nextPts, std::vector<uint8_t> &status)
    {
        const int n = (int)(pts.size() / 2);
        nextPts.assign(pts.size() ? pts.size() : 2, 0.f); status.assign((size_t)(n > 0 ? n : 1), 0);
        check(sgx_flow_lk(h_, imFrom, imTo, w_, pts.data(), n, nextPts.data(), status.data()), "sgx_flow_lk");
        nextPts.resize(pts.size()); status.resize((size_t)n);
    }
private:
    sgx_flow *h_ = nullptr; int w_;
};
// cv::findFundamentalMat(points1, points2, cv::FM_RANSAC, 1.0, 0.99): returns false for OpenCV's empty Mat
inline bool findFundamentalMat(const std::vector<float> &points1, const std::vector<float> &points2, double F[9], double param1 = 1.0, double param2 = 0.99)
{
    int32_t ok = 0;
    check(sgx_find_fundamental_mat(points1.data(), points2.data(), (int)(points1.size() / 2), param1, param2, F, &ok, nullptr), "sgx_find_fundamental_mat");
    return ok != 0;
}

// ORB_SLAM2::Optimizer (Optimizer.h:40-58) — static int PoseOptimization(Frame *pFrame)
class Optimizer {
public:
    // map points of pFrame->mvpMapPoints[i] live in `owner` (the frame the matcher matched against)
    static int PoseOptimization(FrameView *pFrame, const FrameView &owner, const sgx_camera &cam, const std::vector<float> &invLevelSigma2)
    {
        const int N = pFrame->N;
        std::vector<uint8_t> has(N, 0); std::vector<float> xw((size_t)N * 3, 0.f);
        for (int i = 0; i < N; i++) {
            const int m = pFrame->mvpMapPoints[i];
            if (m >= 0) { has[i] = 1; std::memcpy(&xw[3 * (size_t)i], &owner.mpWorldPos[3 * (size_t)m], 12); }
        }
        pFrame->mvbOutlier.assign(N, 0);
        int32_t ninl = 0;
        check(sgx_pose_optimization(N, pFrame->mvKeysUn.data(), pFrame->mvuRight.data(), has.data(), xw.data(), invLevelSigma2.data(),
                                    (int)invLevelSigma2.size(), &cam, pFrame->mTcw, pFrame->mvbOutlier.data(), &ninl), "sgx_pose_optimization");
        return ninl;
    }

    // static void LocalBundleAdjustment(KeyFrame *pKF, bool *pbStopFlag, Map *pMap) (Optimizer.cc:453-778) on the flattened local graph the caller
    // collects at Optimizer.cc:455-653: poses / points are updated in place, the return value lists the erased observations.
    struct LocalGraph {
        std::vector<float> poses;            // n_poses x 16 (Tcw)
        std::vector<uint8_t> pose_fixed;     // 0 local keyframe, 1 fixed camera, 2 local keyframe with mnId == 0
        std::vector<float> points;           // n_points x 3
        std::vector<int32_t> edge_pose, edge_point;
        std::vector<float> edge_obs;         // n_edges x 3 (u, v, uR; uR < 0 = monocular)
        std::vector<float> edge_info;        // mvInvLevelSigma2[octave]
    };
    static std::vector<uint8_t> LocalBundleAdjustment(LocalGraph &g, const sgx_camera &cam, const volatile int32_t *pbStopFlag = nullptr, sgx_ba_stats *stats = nullptr)
    {
        sgx_ba_problem P{(int32_t)g.pose_fixed.size(), (int32_t)(g.points.size() / 3), (int32_t)g.edge_pose.size(), g.poses.data(), g.pose_fixed.data(), g.points.data(),
                         g.edge_pose.data(), g.edge_point.data(), g.edge_obs.data(), g.edge_info.data()};
        std::vector<uint8_t> erase(g.edge_pose.size(), 0);
        check(sgx_local_bundle_adjustment(&P, &cam, pbStopFlag, erase.data(), stats), "sgx_local_bundle_adjustment");
        return erase;
    }
    // static void BundleAdjustment(const vector<KeyFrame*> &vpKFs, const vector<MapPoint*> &vpMP, int nIterations, bool *pbStopFlag, const unsigned long nLoopKF, const bool bRobust)
    // (Optimizer.cc:49-237) on the flattened graph (pose_fixed != 0 for mnId == 0): poses / points updated in place
    static void BundleAdjustment(LocalGraph &g, const sgx_camera &cam, int nIterations = 5, const volatile int32_t *pbStopFlag = nullptr, bool bRobust = true, sgx_ba_stats *stats = nullptr)
    {
        sgx_ba_problem P{(int32_t)g.pose_fixed.size(), (int32_t)(g.points.size() / 3), (int32_t)g.edge_pose.size(), g.poses.data(), g.pose_fixed.data(), g.points.data(),
                         g.edge_pose.data(), g.edge_point.data(), g.edge_obs.data(), g.edge_info.data()};
        check(sgx_bundle_adjustment(&P, &cam, nIterations, pbStopFlag, bRobust ? 1 : 0, stats), "sgx_bundle_adjustment");
    }
    // g2o::Sim3 as (qx, qy, qz, qw, tx, ty, tz, s)
    struct Sim3 { double v[8]; };
    // static int OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale) (Optimizer.cc:1046-1257)
    // on the correspondences the reference turns into edge pairs (include/sgx.h); inlier[i] == 0 <=> vpMatches1[idx] = NULL
    struct Sim3Pairs { std::vector<float> p1c, p2c, obs1, obs2, info1, info2; };
    static int OptimizeSim3(const Sim3Pairs &c, const float K1[4], const float K2[4], Sim3 &g2oS12, float th2, bool bFixScale, std::vector<uint8_t> &inlier)
    {
        const int n = (int)c.info1.size();
        inlier.assign((size_t)(n > 0 ? n : 1), 0); int32_t nin = 0;
        check(sgx_optimize_sim3(n, c.p1c.data(), c.p2c.data(), c.obs1.data(), c.obs2.data(), c.info1.data(), c.info2.data(), K1, K2, g2oS12.v, th2, bFixScale ? 1 : 0, inlier.data(), nullptr, &nin),
              "sgx_optimize_sim3");
        inlier.resize((size_t)n);
        return nin;
    }
    // the optimisation of static void OptimizeEssentialGraph(...) (Optimizer.cc:781-1042) on the flattened pose graph; vertices are updated in place
    struct PoseGraph { std::vector<Sim3> vScw; std::vector<uint8_t> fixed; std::vector<int32_t> e_i, e_j; std::vector<Sim3> e_meas; };
    static void OptimizeEssentialGraph(PoseGraph &g, bool bFixScale, int iterations = 20, double stats[3] = nullptr)
    {
        std::vector<Sim3> out(g.vScw.size() ? g.vScw.size() : 1);
        check(sgx_optimize_essential_graph((int)g.vScw.size(), g.vScw.empty() ? nullptr : g.vScw[0].v, g.fixed.data(), (int)g.e_i.size(), g.e_i.data(), g.e_j.data(),
                                           g.e_meas.empty() ? nullptr : g.e_meas[0].v, bFixScale ? 1 : 0, iterations, out[0].v, stats), "sgx_optimize_essential_graph");
        out.resize(g.vScw.size()); g.vScw = out;
    }
    // The Sim3 glue of loop closing (include/sgx.h).  A pose is 12 floats, the rows of [R | t].
    // LoopClosing::CorrectLoop :440-469, :503-512: the poses of the group in group order (the current keyframe last) and its Scw
    struct LoopSim3 { std::vector<Sim3> NonCorrectedSim3, CorrectedSim3; std::vector<float> correctedTiw; };
    static LoopSim3 PropagateLoopSim3(const std::vector<float> &Tcw_group, const Sim3 &Scw)
    {
        const size_t n = Tcw_group.size() / 12; LoopSim3 r; r.NonCorrectedSim3.resize(n ? n : 1); r.CorrectedSim3.resize(n ? n : 1); r.correctedTiw.resize(12 * (n ? n : 1));
        check(sgx_loop_propagate_sim3((int)n, Tcw_group.data(), Scw.v, r.NonCorrectedSim3[0].v, r.CorrectedSim3[0].v, r.correctedTiw.data()), "sgx_loop_propagate_sim3");
        return r;
    }
    // Optimizer.cc:818-832, :857-867, :889-972: vScw and the measurements for the graph of CovisibilityGraph::essential_graph; Tcw_vertices: the poses in vertex order
    static PoseGraph FlattenEssentialGraph(const CovisibilityGraph::EssentialGraph &e, const std::vector<float> &Tcw_vertices, const LoopSim3 &l)
    {
        PoseGraph g; const size_t nv = e.vertex_id.size(), ne = e.e_i.size();
        if (Tcw_vertices.size() != 12 * nv) check(SGX_ERR_INVALID, "FlattenEssentialGraph");
        g.vScw.resize(nv ? nv : 1); g.e_meas.resize(ne ? ne : 1); g.fixed = e.vertex_fixed; g.e_i = e.e_i; g.e_j = e.e_j;
        check(sgx_eg_flatten((int)nv, e.vertex_group.data(), Tcw_vertices.data(), (int)l.CorrectedSim3.size(), l.CorrectedSim3[0].v, l.NonCorrectedSim3[0].v, (int)ne, e.e_i.data(),
                             e.e_j.data(), e.e_kind.data(), g.vScw[0].v, g.e_meas[0].v), "sgx_eg_flatten");
        g.vScw.resize(nv); g.e_meas.resize(ne);
        return g;
    }
    // Optimizer.cc:991-1010: the poses and vCorrectedSwc of the optimised vertices
    static void RecoverEssentialGraph(const std::vector<Sim3> &S, std::vector<float> &Tcw, std::vector<Sim3> &vCorrectedSwc)
    {
        const size_t n = S.size(); Tcw.assign(12 * (n ? n : 1), 0.f); vCorrectedSwc.resize(n ? n : 1);
        check(sgx_eg_recover((int)n, n ? S[0].v : nullptr, Tcw.data(), vCorrectedSwc[0].v), "sgx_eg_recover");
        Tcw.resize(12 * n); vCorrectedSwc.resize(n);
    }
    static void CorrectMapPoints(std::vector<float> &xw, const std::vector<int32_t> &ref, const std::vector<Sim3> &Srw, const std::vector<Sim3> &correctedSwr)
    {
        std::vector<float> out(xw.size() ? xw.size() : 3);
        check(sgx_correct_map_points((int)ref.size(), xw.data(), ref.data(), (int)Srw.size(), Srw.empty() ? nullptr : Srw[0].v, correctedSwr.empty() ? nullptr : correctedSwr[0].v, out.data()),
              "sgx_correct_map_points");
        out.resize(xw.size()); xw = out;
    }
    // LoopClosing::CorrectLoop (LoopClosing.cc:432-573) with OptimizeEssentialGraph, in the reference's order.  pose(mnId, float[12]) reads a keyframe's Tcw, set_pose
    // writes one back; xw: the world positions by point id, corrected in place (the group's points; the points outside it by their reference keyframe are the caller's,
    // with the S_in / vCorrectedSwc returned); fuse(group, CorrectedSim3): the caller's fusion through covis.Replace / SetObservations.
    struct LoopResult { CovisibilityGraph::LoopGroup group; CovisibilityGraph::LoopConnections connections; CovisibilityGraph::EssentialGraph graph; LoopSim3 sim3; PoseGraph problem;
                        std::vector<Sim3> S_in, vCorrectedSwc; double stats[3] = { 0, 0, 0 }; };
    template <class GetPose, class SetPose, class Fuse>
    static LoopResult CorrectLoop(CovisibilityGraph &covis, int32_t cur, int32_t loop, const Sim3 &Scw, GetPose pose, SetPose set_pose, std::vector<float> &xw, Fuse fuse, bool bFixScale = true)
    {
        LoopResult r; r.group = covis.loop_begin(cur);
        const size_t ng = r.group.group_id.size();
        std::vector<float> Tg(12 * ng);
        for (size_t k = 0; k < ng; k++) pose(r.group.group_id[k], &Tg[12 * k]);
        r.sim3 = PropagateLoopSim3(Tg, Scw);
        std::vector<float> unused; std::vector<Sim3> cSwi; RecoverEssentialGraph(r.sim3.CorrectedSim3, unused, cSwi);
        auto correct = [&](const std::vector<int32_t> &ref, const std::vector<Sim3> &a, const std::vector<Sim3> &c) {
            std::vector<float> p(3 * r.group.point_id.size());
            for (size_t i = 0; i < r.group.point_id.size(); i++) memcpy(&p[3 * i], &xw[3 * (size_t)r.group.point_id[i]], 12);
            CorrectMapPoints(p, ref, a, c);
            for (size_t i = 0; i < r.group.point_id.size(); i++) memcpy(&xw[3 * (size_t)r.group.point_id[i]], &p[3 * i], 12);
        };
        if (!r.group.point_id.empty()) correct(r.group.point_ref, r.sim3.NonCorrectedSim3, cSwi);
        for (size_t k = 0; k < ng; k++) set_pose(r.group.group_id[k], &r.sim3.correctedTiw[12 * k]);
        fuse(r.group, r.sim3.CorrectedSim3);
        r.connections = covis.loop_connections(cur, r.group.group_id);
        r.graph = covis.essential_graph(cur, loop, r.group.group_id, r.connections.lc_begin, r.connections.lc_j);
        const size_t nv = r.graph.vertex_id.size();
        std::vector<float> Tv(12 * nv);
        for (size_t v = 0; v < nv; v++) pose(r.graph.vertex_id[v], &Tv[12 * v]);
        r.problem = FlattenEssentialGraph(r.graph, Tv, r.sim3);
        r.S_in = r.problem.vScw;
        OptimizeEssentialGraph(r.problem, bFixScale, 20, r.stats);
        std::vector<float> Tn; RecoverEssentialGraph(r.problem.vScw, Tn, r.vCorrectedSwc);
        for (size_t v = 0; v < nv; v++) set_pose(r.graph.vertex_id[v], &Tn[12 * v]);
        if (!r.group.point_id.empty()) {
            std::vector<int32_t> ref(r.group.point_ref.size());
            for (size_t i = 0; i < ref.size(); i++) ref[i] = r.group.group_vertex[(size_t)r.group.point_ref[i]];
            correct(ref, r.S_in, r.vCorrectedSwc);
        }
        if (cur != loop) covis.AddLoopEdge(loop, cur);
        return r;
    }
};

// ORB_SLAM2::LoopClosing (LoopClosing.h, src/sg-slam/src/LoopClosing.cc) over the covisibility graph, the keyframe database and the optimiser: DetectLoop (:103-229),
// CorrectLoop (:402-585) and RunGlobalBundleAdjustment (:645-749).  ComputeSim3's orchestration (:231-400), SetNotErase / SetErase and InformNewBigChange stay the caller's.
class LoopClosing {
public:
    typedef ORBVocabulary::BowVector BowVector;
    LoopClosing(CovisibilityGraph &covis, KeyFrameDatabase &db, bool bFixScale = true, int nCovisibilityConsistencyTh = 3)
        : covis_(covis), db_(db), mbFixScale(bFixScale), mnCovisibilityConsistencyTh(nCovisibilityConsistencyTh) {}
    long mLastLoopKFid = 0;
    std::vector<int32_t> mvpEnoughConsistentCandidates, vpCandidateKFs;
    bool early = false; float minScore = 1.0f;                                   // what the last DetectLoop saw
    // bool DetectLoop() for mpCurrentKF = mnId with its mBowVec; the keyframe enters the database on every exit (:116, :146, :215)
    bool DetectLoop(int32_t mnId, const BowVector &mBowVec)
    {
        struct Add { KeyFrameDatabase &db; int32_t id; const BowVector &v; ~Add() { db.add(id, v); } } add{db_, mnId, mBowVec};
        mvpEnoughConsistentCandidates.clear(); vpCandidateKFs.clear();
        early = mnId < mLastLoopKFid + 10;                                       // :114
        if (early) return false;
        std::vector<int32_t> listed;
        for (const auto &e : covis_.GetOrderedConnectedKeyFrames(mnId)) listed.push_back(e.first);      // GetVectorCovisibleKeyFrames()
        minScore = db_.MinScore(mBowVec, listed);                                // :126-138
        vpCandidateKFs = db_.DetectLoopCandidates(mBowVec, covis_.GetConnectedKeyFrames(mnId), minScore);      // :141
        mvpEnoughConsistentCandidates = covis_.CheckConsistency(vpCandidateKFs, mnCovisibilityConsistencyTh);    // :144-211; no candidate clears the groups
        return !mvpEnoughConsistentCandidates.empty();
    }
    // void CorrectLoop() through Optimizer::CorrectLoop; mLastLoopKFid = mpCurrentKF->mnId (:584)
    template <class GetPose, class SetPose, class Fuse>
    Optimizer::LoopResult CorrectLoop(int32_t cur, int32_t loop, const Optimizer::Sim3 &Scw, GetPose pose, SetPose set_pose, std::vector<float> &xw, Fuse fuse)
    {
        Optimizer::LoopResult r = Optimizer::CorrectLoop(covis_, cur, loop, Scw, pose, set_pose, xw, fuse, mbFixScale);
        mLastLoopKFid = cur;
        return r;
    }
    // void RunGlobalBundleAdjustment(unsigned long nLoopKF): the global graph of the handle, gathered by the caller's callbacks, Optimizer::BundleAdjustment with the
    // results kept apart (mTcwGBA / mPosGBA), then the map update (:676-737) for the map as it stands after while_running() (what LocalMapping did meanwhile).
    //   pose(mnId, float[12]) = Tcw now; observation(mnId, idx, float[3]) = (u, v, uR); invSigma2(octave); point(id, float[3]) = GetWorldPos() now;
    //   reference(id) = GetReferenceKeyFrame()->mnId or -1.  Returns the update; ids / points name its rows.
    struct GbaResult { CovisibilityGraph::GbaUpdate update; std::vector<int32_t> kf_ids, point_ids; sgx_ba_stats stats{}; };
    template <class GetPose, class GetObs, class InvSigma2, class GetPoint, class GetRef, class Meanwhile>
    GbaResult RunGlobalBundleAdjustment(unsigned long nLoopKF, const sgx_camera &cam, const std::vector<int32_t> &origins, GetPose pose, GetObs observation, InvSigma2 invSigma2,
                                        GetPoint point, GetRef reference, Meanwhile while_running, int nIterations = 10)
    {
        (void)nLoopKF;
        const CovisibilityGraph::BaGraph g = covis_.ba_graph(0, SGX_COVIS_BA_GLOBAL);
        Optimizer::LocalGraph P; const size_t nkf = g.pose_id.size(), npt = g.point_id.size(), ne = g.edge_pose.size();
        P.poses.assign(16 * nkf, 0.f); P.pose_fixed = g.pose_fixed; P.points.resize(3 * npt); P.edge_pose = g.edge_pose; P.edge_point = g.edge_point; P.edge_obs.resize(3 * ne); P.edge_info.resize(ne);
        for (size_t k = 0; k < nkf; k++) { pose(g.pose_id[k], &P.poses[16 * k]); P.poses[16 * k + 15] = 1.f; }
        for (size_t i = 0; i < npt; i++) point(g.point_id[i], &P.points[3 * i]);
        for (size_t e = 0; e < ne; e++) {
            observation(g.pose_id[(size_t)g.edge_pose[e]], g.edge_kp[e], &P.edge_obs[3 * e]);
            if (!(g.edge_attr[e] & SGX_COVIS_ATTR_RIGHT)) P.edge_obs[3 * e + 2] = -1.f;      // Optimizer.cc:594
            P.edge_info[e] = invSigma2(g.edge_attr[e] & SGX_COVIS_ATTR_OCTAVE);
        }
        const Optimizer::LocalGraph before = P;
        GbaResult R;
        Optimizer::BundleAdjustment(P, cam, nIterations, nullptr, false, &R.stats);      // GlobalBundleAdjustemnt(mpMap, 10, &mbStopGBA, nLoopKF, false)
        while_running();
        const CovisibilityGraph::BaGraph now = covis_.ba_graph(0, SGX_COVIS_BA_GLOBAL);
        R.kf_ids = now.pose_id; R.point_ids = now.point_id;
        const size_t nk = R.kf_ids.size(), np = R.point_ids.size();
        std::vector<uint8_t> in_gba(nk, 0), pin(np, 0); std::vector<float> T(12 * nk), TG(12 * nk, 0.f), X(3 * np), XG(3 * np, 0.f); std::vector<int32_t> ref(np, -1);
        for (size_t r = 0, j = 0; r < nk; r++) {                                 // both rows ascend in id
            while (j < nkf && g.pose_id[j] < R.kf_ids[r]) j++;
            if (j < nkf && g.pose_id[j] == R.kf_ids[r]) { in_gba[r] = 1; memcpy(&T[12 * r], &before.poses[16 * j], 48); memcpy(&TG[12 * r], &P.poses[16 * j], 48); }
            else pose(R.kf_ids[r], &T[12 * r]);
        }
        for (size_t i = 0, j = 0; i < np; i++) {
            while (j < npt && g.point_id[j] < R.point_ids[i]) j++;
            if (j < npt && g.point_id[j] == R.point_ids[i]) { pin[i] = 1; memcpy(&X[3 * i], &before.points[3 * j], 12); memcpy(&XG[3 * i], &P.points[3 * j], 12); }
            else point(R.point_ids[i], &X[3 * i]);
            const int32_t k = reference(R.point_ids[i]);
            const auto it = std::lower_bound(R.kf_ids.begin(), R.kf_ids.end(), k);
            ref[i] = (k >= 0 && it != R.kf_ids.end() && *it == k) ? (int32_t)(it - R.kf_ids.begin()) : -1;
        }
        R.update = covis_.GlobalBundleAdjustmentUpdate(origins, R.kf_ids, in_gba, T, TG, X, pin, XG, ref);
        return R;
    }
private:
    CovisibilityGraph &covis_; KeyFrameDatabase &db_; bool mbFixScale; int mnCovisibilityConsistencyTh;
};

// ORB_SLAM2::Detector2D (Detector2D.h:45-67): same public result members as the reference (read by Frame.cc:482-500)
struct Object2D { float x, y, w, h; float prob; int id; };          // cv::Rect_<float> rect; float prob; int id (name = class_names[id])
class Detector2D {
public:
    // param_text / bin: the contents of ./Thirdparty/ncnn_model/mobilenetv3_ssdlite_voc.{param,bin} (Detector2D.cc:24-25 reads them from the CWD)
    Detector2D(float detection_confidence_threshold, float dynamic_detection_confidence_threshold, const std::string &param_text, const std::vector<uint8_t> &bin,
               int width = 640, int height = 480)
    {
        check(sgx_det_create(param_text.c_str(), bin.data(), bin.size(), width, height, 1, detection_confidence_threshold, dynamic_detection_confidence_threshold, &h_), "sgx_det_create");
    }
    ~Detector2D() { if (h_) sgx_det_destroy(h_); }
    Detector2D(const Detector2D &) = delete; Detector2D &operator=(const Detector2D &) = delete;

    void detect(const uint8_t *bgr, int step)                       // void detect(const cv::Mat &bgr) (Detector2D.cc:34-89)
    {
        sgx_det_result r;
        check(sgx_det_detect(h_, bgr, step, 1, &r), "sgx_det_detect");
        auto conv = [](const sgx_object2d &o) { return Object2D{o.x, o.y, o.w, o.h, o.prob, o.id}; };
        mvObjects2D.clear(); mvPotentialDynamicBorderForMapping.clear(); mvPotentialDynamicBorderForRmDynamicFeature.clear(); raw.assign(r.raw, r.raw + r.n_raw);
        for (int i = 0; i < r.n_objects; i++) mvObjects2D.push_back(conv(r.objects[i]));
        for (int i = 0; i < r.n_map_boxes; i++) mvPotentialDynamicBorderForMapping.push_back(conv(r.map_boxes[i]));
        for (int i = 0; i < r.n_rm_boxes; i++) mvPotentialDynamicBorderForRmDynamicFeature.push_back(conv(r.rm_boxes[i]));
        mbHaveDynamicObjectForMapping = r.have_dynamic_for_mapping != 0; mbHaveDynamicObjectForRmDynamicFeature = r.have_dynamic_for_rm_feature != 0;
    }
    std::vector<Object2D> mvObjects2D, mvPotentialDynamicBorderForMapping, mvPotentialDynamicBorderForRmDynamicFeature;
    bool mbHaveDynamicObjectForMapping = false, mbHaveDynamicObjectForRmDynamicFeature = false;
    std::vector<sgx_detection> raw;                                  // ncnn detection_out rows (test tap)
private:
    sgx_det *h_ = nullptr;
public:
    sgx_det *handle() { return h_; }
};

// ObjectDatabase (ObjectDatabase.h:12-45) and Detector3D (Detector3D.h:46-76): the semantic objects of a keyframe from its Object2D boxes, its depth image and its pose
struct SemanticObject { float centroid[3], size[3]; float prob; int class_id, object_id; };      // object_name = class_names[class_id]
class ObjectDatabase {
public:
    ObjectDatabase() { check(sgx_objdb_create(&h_), "sgx_objdb_create"); }
    ~ObjectDatabase() { if (h_) sgx_objdb_destroy(h_); }
    ObjectDatabase(const ObjectDatabase &) = delete; ObjectDatabase &operator=(const ObjectDatabase &) = delete;
    void addObject(SemanticObject &cluster)                          // void addObject(SemanticObject& cluster): cluster.object_id is set when the object is appended
    {
        sgx_semantic_object o; o.class_id = cluster.class_id; o.object_id = 0; o.prob = cluster.prob;
        for (int i = 0; i < 3; i++) { o.centroid[i] = cluster.centroid[i]; o.size[i] = cluster.size[i]; }
        int32_t id = 0, merged = 0;
        check(sgx_objdb_add(h_, &o, &id, &merged), "sgx_objdb_add");
        if (!merged) cluster.object_id = id;
    }
    int getDataBaseSize() const { return sgx_objdb_size(h_); }
    SemanticObject getObjectByID(int objectID) const                 // mvSemanticObject[objectID - 1]
    {
        sgx_semantic_object o; check(sgx_objdb_get(h_, objectID - 1, &o), "sgx_objdb_get");
        SemanticObject s; s.class_id = o.class_id; s.object_id = o.object_id; s.prob = o.prob;
        for (int i = 0; i < 3; i++) { s.centroid[i] = o.centroid[i]; s.size[i] = o.size[i]; }
        return s;
    }
private:
    sgx_objdb *h_ = nullptr;
};

class Detector3D {
public:
    // the reference's constructor arguments (Detector3D.h:49-51) plus what it reads from its members and the keyframe: the valid depth range, the image size and
    // the camera (fx, fy, cx, cy)
    Detector3D(int Detect3D_Sor_MeanK_, double Detect3D_Sor_StddevMulThresh_, float Detect3D_Voxel_LeafSize_, float EuclideanClusterTolerance_, int EuclideanClusterMinSize_,
               int EuclideanClusterMaxSize_, float DetectSimilarCompareRatio_, float camera_valid_depth_Min_, float camera_valid_depth_Max_, int width, int height,
               const float cam[4], int max_crop_points = 0 /* the crop of a box that is the whole image */)
    {
        sgx_obj3d_params p; p.sor_stddev_mul = Detect3D_Sor_StddevMulThresh_; p.sor_mean_k = Detect3D_Sor_MeanK_; p.cluster_min_size = EuclideanClusterMinSize_;
        p.cluster_max_size = EuclideanClusterMaxSize_; p.voxel_leaf_size = Detect3D_Voxel_LeafSize_; p.cluster_tolerance = EuclideanClusterTolerance_;
        p.similar_compare_ratio = DetectSimilarCompareRatio_; p.camera_valid_depth_min = camera_valid_depth_Min_; p.camera_valid_depth_max = camera_valid_depth_Max_;
        for (int i = 0; i < 4; i++) cam_[i] = cam[i];
        check(sgx_obj3d_create(width, height, 1, 1, max_crop_points, &p, &h_), "sgx_obj3d_create");
        mpObjectDatabase = new ObjectDatabase;
    }
    ~Detector3D() { delete mpObjectDatabase; if (h_) sgx_obj3d_destroy(h_); }
    Detector3D(const Detector3D &) = delete; Detector3D &operator=(const Detector3D &) = delete;
    // void Detect(vector<Object2D>&, cv::Mat &depth, PointCloud::ConstPtr): depth = mImDep (float metres, height x width, tight), Twc = the 4 x 4 double matrix the
    // caller passes to pcl::transformPointCloud (row-major) in place of the transformed cloud
    void Detect(const std::vector<Object2D> &vobject2d, const float *depth, const double Twc[16])
    {
        for (const Object2D &o : vobject2d) { SemanticObject s; if (DetectOne(o, s, depth, Twc)) mpObjectDatabase->addObject(s); }
    }
    bool DetectOne(const Object2D &object2d, SemanticObject &semantic_object, const float *depth, const double Twc[16], sgx_obj3d_result *record = nullptr)
    {
        sgx_obj3d_job j; j.image = 0; j.class_id = object2d.id; j.prob = object2d.prob; j.x = object2d.x; j.y = object2d.y; j.w = object2d.w; j.h = object2d.h;
        sgx_obj3d_result r;
        check(sgx_obj3d_detect(h_, depth, cam_, Twc, &j, &r), "sgx_obj3d_detect");
        if (record) *record = r;
        if (!r.found) return false;
        semantic_object.class_id = r.class_id; semantic_object.prob = r.prob; semantic_object.object_id = 0;
        for (int i = 0; i < 3; i++) { semantic_object.centroid[i] = r.centroid[i]; semantic_object.size[i] = r.size[i]; }
        return true;
    }
    ObjectDatabase *mpObjectDatabase = nullptr;
private:
    sgx_obj3d *h_ = nullptr; float cam_[4];
};

// PointCloudMapping (PointcloudMapping.h): the filtered local-map cloud of a keyframe (generatePointCloud*, voxel_local, sor_local, slam_to_ros_mode_transform) and
// camera_to_map_tf, as MapViewer publishes them for octomap_server; thin over sgx_cloud_*.  The semantic objects of the keyframe are Detector3D::Detect's (above).
struct LocalMap { std::vector<sgx_cloud_point> points; sgx_cloud_result record; double origin[3], rotation[4]; };     // rotation = x, y, z, w
class PointCloudMapping {
public:
    // the reference's constructor arguments that the local map reads (PointcloudMapping.h) plus the image size and the camera (fx, fy, cx, cy)
    PointCloudMapping(bool is_map_construction_consider_dynamic_, float camera_valid_depth_Min_, float camera_valid_depth_Max_, int Sor_Local_MeanK_,
                      double Sor_Local_StddevMulThresh_, float Voxel_Local_LeafSize_, int width, int height, const float cam[4], int max_boxes = SGX_CLOUD_MAX_BOXES)
        : N_(width * height)
    {
        sgx_cloud_params p; std::memset(&p, 0, sizeof p);
        p.sor_stddev_mul = Sor_Local_StddevMulThresh_; p.sor_mean_k = Sor_Local_MeanK_; p.consider_dynamic = is_map_construction_consider_dynamic_ ? 1 : 0;
        p.voxel_leaf_size = Voxel_Local_LeafSize_; p.camera_valid_depth_min = camera_valid_depth_Min_; p.camera_valid_depth_max = camera_valid_depth_Max_;
        for (int i = 0; i < 4; i++) cam_[i] = cam[i];
        check(sgx_cloud_create(width, height, 1, max_boxes, SGX_CLOUD_LOCAL, &p, &h_), "sgx_cloud_create");
    }
    ~PointCloudMapping() { if (h_) sgx_cloud_destroy(h_); }
    PointCloudMapping(const PointCloudMapping &) = delete; PointCloudMapping &operator=(const PointCloudMapping &) = delete;
    // void insertKeyFrame(KeyFrame*, cv::Mat &color, cv::Mat &depth) and the MapViewer pass over it: color = mImRGB (height x width x 3 bytes, tight), depth = mImDep
    // (float metres), Tcw = the keyframe's float pose (row-major), boxes = mvPotentialDynamicBorderForMapping as (x, y, w, h), haveDynamic = mbHaveDynamicObjectForMapping
    void insertKeyFrame(const uint8_t *color, const float *depth, const float Tcw[16], const std::vector<float> &boxes, bool haveDynamic, LocalMap &out)
    {
        out.points.resize((size_t)N_);
        check(sgx_cloud_build(h_, depth, color, cam_, nullptr, boxes.data(), (int)(boxes.size() / 4), haveDynamic ? 1 : 0, out.points.data(), N_, &out.record), "sgx_cloud_build");
        out.points.resize((size_t)out.record.n_points);
        check(sgx_cloud_camera_to_map_tf(Tcw, out.origin, out.rotation), "sgx_cloud_camera_to_map_tf");
    }
    sgx_cloud *handle() { return h_; }
private:
    sgx_cloud *h_ = nullptr; int N_; float cam_[4];
};

// octomap_server's OctomapServer (src/octomap_server/src/OctomapServer.cpp) over sgx_octomap_*: insertCloudCallback for the local map of a keyframe (:261-354, the
// non-ground branch, and insertScan :356-480) and what publishAll derives from the tree (:484-): the occupied / free cell centres in the order of octomap's leaf
// iterator and the projected nav_msgs::OccupancyGrid.  Occupancy only; the parameters are octomap_server's, with its defaults.
struct OccupancyGrid { sgx_octomap_grid_header_t info; std::vector<int8_t> data; };       // data: row-major x + y * width, -1 / 0 / 100
class OctomapServer {
public:
    static sgx_octomap_params defaults()
    {
        sgx_octomap_params p; std::memset(&p, 0, sizeof p);
        p.res = 0.05; p.prob_hit = 0.7; p.prob_miss = 0.4; p.thres_min = 0.12; p.thres_max = 0.97; p.max_range = -1.0;
        p.pointcloud_min_x = p.pointcloud_min_y = p.pointcloud_min_z = p.occupancy_min_z = -DBL_MAX;
        p.pointcloud_max_x = p.pointcloud_max_y = p.pointcloud_max_z = p.occupancy_max_z = DBL_MAX;
        return p;
    }
    explicit OctomapServer(const sgx_octomap_params &p = defaults(), int max_bricks = 1 << 14, int max_points_per_scan = 1 << 16)
    { check(sgx_octomap_create(&p, max_bricks, max_points_per_scan, &h_), "sgx_octomap_create"); }
    ~OctomapServer() { if (h_) sgx_octomap_destroy(h_); }
    OctomapServer(const OctomapServer &) = delete; OctomapServer &operator=(const OctomapServer &) = delete;
    // one cloud in the sensor frame with the transform camera_to_map_tf gave for its keyframe (tf + pcl_ros::transformAsMatrix)
    sgx_octomap_record insertCloud(const std::vector<sgx_cloud_point> &cloud, const double origin[3], const double rotation[4])
    {
        float m[16]; sgx_octomap_record rec;
        check(sgx_octomap_sensor_to_world(origin, rotation, m), "sgx_octomap_sensor_to_world");
        check(sgx_octomap_insert(h_, cloud.data(), (int)cloud.size(), m, &rec), "sgx_octomap_insert");
        return rec;
    }
    sgx_octomap_record insertCloud(const LocalMap &m) { return insertCloud(m.points, m.origin, m.rotation); }
    sgx_octomap_bounds_t bounds() { sgx_octomap_bounds_t b; check(sgx_octomap_bounds(h_, &b), "sgx_octomap_bounds"); return b; }
    std::vector<sgx_octomap_cell> cells(bool occupied)
    {
        const sgx_octomap_bounds_t b = bounds();
        std::vector<sgx_octomap_cell> out((size_t)(occupied ? b.n_occupied : b.n_free)); int32_t n = 0;
        check(sgx_octomap_cells(h_, occupied ? 1 : 0, out.data(), (int)out.size(), &n), "sgx_octomap_cells");
        out.resize((size_t)n);
        return out;
    }
    OccupancyGrid projectedMap()
    {
        OccupancyGrid g;                                                                     // one call when the grid still fits the last size, two when it has grown
        g.data.resize(grid_cells_);
        int rc = sgx_octomap_project(h_, &g.info, g.data.data(), (int64_t)g.data.size());
        grid_cells_ = (size_t)g.info.width * (size_t)g.info.height;
        if (rc == SGX_ERR_OVERFLOW) { g.data.resize(grid_cells_); rc = sgx_octomap_project(h_, &g.info, g.data.data(), (int64_t)g.data.size()); }
        check(rc, "sgx_octomap_project");
        g.data.resize(grid_cells_);
        return g;
    }
    void reset() { check(sgx_octomap_reset(h_), "sgx_octomap_reset"); }
    sgx_octomap *handle() { return h_; }
private:
    sgx_octomap *h_ = nullptr; size_t grid_cells_ = 0;
};

// MapViewer's globalMap (PointcloudMapping.cc:332-360, /SG_SLAM/Global_Point_Clouds) over sgx_globalmap_*: `*globalMap += *temp_globalMap` for every keyframe and
// voxel_global + sor_global over the whole accumulated map on the reference's schedule.  temp_globalMap is the cloud sgx_cloud builds in SGX_CLOUD_WORLD mode.
class GlobalMap {
public:
    // Voxel_Global_LeafSize, Sor_Global_MeanK, Sor_Global_StddevMulThresh, global_pc_update_kf_threshold of the reference's settings, and the map's capacity
    GlobalMap(float Voxel_Global_LeafSize_, int Sor_Global_MeanK_, double Sor_Global_StddevMulThresh_, int global_pc_update_kf_threshold_, int max_points = 1 << 20)
        : threshold_(global_pc_update_kf_threshold_)
    {
        sgx_globalmap_params p; std::memset(&p, 0, sizeof p);
        p.sor_stddev_mul = Sor_Global_StddevMulThresh_; p.sor_mean_k = Sor_Global_MeanK_; p.voxel_leaf_size = Voxel_Global_LeafSize_;
        check(sgx_globalmap_create(max_points, &p, &h_), "sgx_globalmap_create");
    }
    ~GlobalMap() { if (h_) sgx_globalmap_destroy(h_); }
    GlobalMap(const GlobalMap &) = delete; GlobalMap &operator=(const GlobalMap &) = delete;
    // *globalMap += *temp_globalMap (:339); a cloud that does not fit is refused whole (SGX_GMAP_FULL in the record)
    sgx_globalmap_append_record append(const std::vector<sgx_cloud_point> &temp_globalMap)
    {
        sgx_globalmap_append_record r;
        check(sgx_globalmap_append(h_, temp_globalMap.data(), (int)temp_globalMap.size(), &r), "sgx_globalmap_append");
        return r;
    }
    sgx_globalmap_result consolidate() { sgx_globalmap_result r; check(sgx_globalmap_consolidate(h_, &r), "sgx_globalmap_consolidate"); return r; }
    int size() { int32_t n = 0; check(sgx_globalmap_size(h_, &n), "sgx_globalmap_size"); return n; }
    std::vector<sgx_cloud_point> points()
    {
        std::vector<sgx_cloud_point> out((size_t)size()); int32_t n = 0;
        check(sgx_globalmap_read(h_, out.data(), (int)out.size(), &n), "sgx_globalmap_read");
        out.resize((size_t)n);
        return out;
    }
    // :340-359 after append: pending = CheckNewKeyFrames().  True when the map was consolidated and published into `published` (which may be empty: count is then
    // not reset); count++ in every case
    bool update(bool pending, std::vector<sgx_cloud_point> &published, sgx_globalmap_result *record = nullptr)
    {
        bool pub = false;
        if (!pending || count_ > threshold_) {
            const sgx_globalmap_result r = consolidate();
            if (record) *record = r;
            published = points(); pub = true;
            if (!published.empty()) count_ = 0;
        }
        count_++;
        return pub;
    }
    int count() const { return count_; }
    void reset() { check(sgx_globalmap_reset(h_), "sgx_globalmap_reset"); count_ = 0; }
    sgx_globalmap *handle() { return h_; }
private:
    sgx_globalmap *h_ = nullptr; int threshold_, count_ = 0;
};

// Frame::ComputeStereoMatches (Frame.cc:716-890) as the stereo constructor Frame::Frame(imLeft, imRight, ...) calls it (:70-99): the two extractors of the reference
// (mpORBextractorLeft / Right, of one geometry) run on the two images, then mvuRight / mvDepth come from their keys, descriptors and pyramids; thin over sgx_stereo_*.
// mvuRight is computed from the raw keypoints, as in the reference.
struct StereoMatches { std::vector<sgx_keypoint> mvKeys, mvKeysRight; std::vector<uint8_t> mDescriptors, mDescriptorsRight; std::vector<float> mvuRight, mvDepth; int nmatched = 0; };
class StereoMatcher {
public:
    StereoMatcher(ORBextractor &extractorLeft, ORBextractor &extractorRight) : left_(extractorLeft), right_(extractorRight)
    {
        check(sgx_stereo_create(left_.handle(), 1, &h_), "sgx_stereo_create");
    }
    ~StereoMatcher() { if (h_) sgx_stereo_destroy(h_); }
    StereoMatcher(const StereoMatcher &) = delete; StereoMatcher &operator=(const StereoMatcher &) = delete;
    // ExtractORB(0, imLeft), ExtractORB(1, imRight), ComputeStereoMatches(); fx = K(0, 0), bf = mbf
    void operator()(const GrayView &imLeft, const GrayView &imRight, float fx, float bf, StereoMatches &out)
    {
        left_(imLeft, nullptr, out.mvKeys, out.mDescriptors); right_(imRight, nullptr, out.mvKeysRight, out.mDescriptorsRight);
        const size_t N = out.mvKeys.size();
        out.mvuRight.assign(N, -1.0f); out.mvDepth.assign(N, -1.0f); out.nmatched = 0;
        if (N == 0) return;                                          // Frame.cc:94-95
        check(sgx_stereo_match(h_, left_.handle(), right_.handle(), out.mvKeys.data(), out.mDescriptors.data(), (int)N, out.mvKeysRight.data(), out.mDescriptorsRight.data(),
                               (int)out.mvKeysRight.size(), fx, bf, out.mvuRight.data(), out.mvDepth.data(), &out.nmatched), "sgx_stereo_match");
    }
    sgx_stereo *handle() { return h_; }
private:
    ORBextractor &left_, &right_; sgx_stereo *h_ = nullptr;
};

// cv::undistortPoints(points, out, K, D, noArray(), K) as Frame::UndistortKeyPoints calls it (Frame.cc:654-684), and Frame::ComputeImageBounds (:686-714);
// K4 = fx, fy, cx, cy, distCoef = 4, 5 or 8 coefficients.  Points are (x, y) pairs.
inline std::vector<float> UndistortPoints(const std::vector<float> &points, const float K4[4], const std::vector<float> &distCoef)
{
    std::vector<float> out(points.size());
    check(sgx_undistort_points((int)(points.size() / 2), points.data(), K4, distCoef.data(), (int)distCoef.size(), out.data()), "sgx_undistort_points");
    return out;
}
inline void ComputeImageBounds(int cols, int rows, const float K4[4], const std::vector<float> &distCoef, sgx_camera &cam)
{
    check(sgx_frame_image_bounds(cols, rows, K4, distCoef.data(), (int)distCoef.size(), &cam), "sgx_frame_image_bounds");
}

// The pipelined per-frame host (sgx_tracker_*): S RGB-D streams tracked in lock-step with Tracking::GrabImageRGBD's call order (src/sg-slam/src/Tracking.cc:206-251,
// :906-1013) on three event-chained HIP streams inside the library.  GrabImagesRGBD(slot) = one frame of every stream from the pinned staging buffers of `slot`
// (imRGB as cv::imread delivers it — interleaved 8-bit BGR — and the raw 16-bit depth map, rgbd_tum.cc:114-115), asynchronous; Pose() synchronises.
class TrackingPipeline {
public:
    TrackingPipeline(int streams, const sgx_camera &cam, float depthMapFactor, Detector2D *detector = nullptr, int width = 640, int height = 480, int nFeatures = 1000,
                     float scaleFactor = 1.2f, int nLevels = 8, int iniThFAST = 20, int minThFAST = 7, bool localMap = true, bool dynamicMask = true, int maxBoxes = 8)
        : S_(streams), W_(width), H_(height)
    {
        sgx_tracker_config c; std::memset(&c, 0, sizeof c);
        c.streams = streams; c.width = width; c.height = height; c.nfeatures = nFeatures; c.scale_factor = scaleFactor; c.nlevels = nLevels; c.ini_th_fast = iniThFAST; c.min_th_fast = minThFAST;
        c.cam = cam; c.depth_map_factor = depthMapFactor; c.th_projection = 15.f; c.local_map = localMap; c.dynamic_mask = dynamicMask; c.max_boxes = maxBoxes; c.pipelined = 1;
        check(sgx_tracker_create(&c, detector ? detector->handle() : nullptr, &h_), "sgx_tracker_create");
    }
    ~TrackingPipeline() { if (h_) sgx_tracker_destroy(h_); }
    TrackingPipeline(const TrackingPipeline &) = delete;
    TrackingPipeline &operator=(const TrackingPipeline &) = delete;
    void SetInitialPose(const std::vector<float> &Tcw) { if ((int)Tcw.size() != 16 * S_) throw std::invalid_argument("SetInitialPose: streams x 16 floats"); check(sgx_tracker_set_initial_pose(h_, Tcw.data()), "sgx_tracker_set_initial_pose"); }
    // mDistCoef (Tracking.cc:66-77: k1, k2, p1, p2 [, k3]), before the first frame: Frame::UndistortKeyPoints / ComputeImageBounds from then on (k1 == 0: nothing changes).
    // Returns the camera with the grid / frustum bounds the pipeline uses (mnMinX, mnMaxX, mnMinY, mnMaxY).
    sgx_camera SetDistortion(const std::vector<float> &distCoef)
    {
        sgx_camera cam; std::memset(&cam, 0, sizeof cam);
        check(sgx_tracker_set_distortion(h_, distCoef.data(), (int)distCoef.size(), &cam), "sgx_tracker_set_distortion");
        return cam;
    }
    // staging buffers of slot 0 / 1: bgr = streams x height rows of `pitch` bytes (3 * width used), depth = streams x height x width uint16
    void HostBuffers(int slot, uint8_t **bgr, int *pitch, uint16_t **depth) { check(sgx_tracker_host_buffers(h_, slot, bgr, pitch, depth), "sgx_tracker_host_buffers"); }
    void GrabImagesRGBD(int slot, bool rgbOrder = true) { check(sgx_tracker_step_host(h_, slot, rgbOrder ? 1 : 0), "sgx_tracker_step_host"); }
    void Synchronize() { check(sgx_tracker_sync(h_), "sgx_tracker_sync"); }
    // blocks until the device has read the input images of the step issued stepsBack (0..2) calls ago; HostBuffers(slot) does the same for a pinned staging slot
    void WaitInputs(int stepsBack = 0) { check(sgx_tracker_wait_inputs(h_, stepsBack), "sgx_tracker_wait_inputs"); }
    // mCurrentFrame.mTcw of every stream (streams x 16) and the tracking counts of the frame tracked last (synchronises)
    void Pose(std::vector<float> &Tcw, std::vector<int32_t> *nKeys = nullptr, std::vector<int32_t> *nMatches = nullptr, std::vector<int32_t> *nInliers = nullptr)
    {
        Tcw.resize((size_t)16 * S_);
        if (nKeys) nKeys->resize(S_);
        if (nMatches) nMatches->resize(S_);
        if (nInliers) nInliers->resize(S_);
        check(sgx_tracker_read(h_, Tcw.data(), nKeys ? nKeys->data() : nullptr, nMatches ? nMatches->data() : nullptr, nullptr, nullptr, nInliers ? nInliers->data() : nullptr, nullptr, nullptr, nullptr),
              "sgx_tracker_read");
    }
    int streams() const { return S_; }
    sgx_tracker *handle() { return h_; }
private:
    sgx_tracker *h_ = nullptr; int S_, W_, H_;
};

}  // namespace sgx
