/* sgx_debug.h — TEST / TUNING TAPS of libsgx.  NOT part of the product: the default build of sg_slam_amd/libsgx.so exports none of these symbols and reads no
 * SGX_* environment variable (every sgx_getenv() in csrc/ is a constant NULL there).  They exist only in builds with -DSGX_DEBUG_TAPS:
 *   tests/taps/libsgx_taps.so   (hipcc, gfx950; `make -C sg_slam_amd/csrc taps`)  — the GPU tests that read intermediate blobs / pyramid levels / force a plan, and the A/B tools
 *   tests/emu/libsgx_emu.so     (g++, -DSGX_EMU)                                   — the kernel-logic emulator of the CPU tests
 * Same sources, same kernels; the taps only add read-backs and plan selection.  Every sgx_*_debug_set_* setting is PER CALLING THREAD (thread_local): it affects the
 * next create / call made by the same thread only. */
#ifndef SGX_DEBUG_H
#define SGX_DEBUG_H
#include "sgx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* test/diagnostic taps (synchronous, host destination) */
int sgx_orb_debug_level_geometry(const sgx_orb *h, int level, int32_t *w, int32_t *hgt, int32_t *stride);
int sgx_orb_debug_set_unfused_pyramid(int on);   /* test tap: 1 = per-level k_resize launches instead of the fused pyramid kernel (must give identical bytes) */
int sgx_orb_debug_read_level(sgx_orb *h, int frame, int level, uint8_t *dst /* w*h, tight */);
/* candidates of (frame, level) after per-cell FAST+NMS, unordered: x,y relative to the
 * (16,16) border origin exactly as pushed at ORBextractor.cc:823-825; returns count in *n */
int sgx_orb_debug_read_candidates(sgx_orb *h, int frame, int level, int32_t *x, int32_t *y, int32_t *score, int cap, int *n);
/* Harness helper (bench.py / tests), NOT a reference entry point: the previous-frame position of every keypoint under a per-frame affine flow
 * (prev = A * (x, y, 1), A = 6 floats), optionally displaced by shift[2] inside the frame's first box.  Stands in for cv::calcOpticalFlowPyrLK
 * (Frame.cc:445, tier N1) when the dynamic-feature mask is exercised on synthetic streams whose flow is known exactly. */
int sgx_debug_flow_affine_batch_dev(int batch, int cap, const sgx_keypoint *d_keys, const int32_t *d_n, const float *d_A, const float *d_shift, const float *d_boxes,
                                    int max_boxes, float *d_prev_xy, void *stream);
int sgx_pose_opt_debug_set_threads(int threads_per_frame);   /* tuning / test tap: 0 = default (256 threads = four waves per frame), 64 = one wave per frame, 256 */
int sgx_ba_debug_last_plan(int32_t plan[4]);    /* test tap: solver plan of the last bundle adjustment of this process: { 0 dense / 1 envelope, column steps of branch A, of branch B (0 = one branch), unknowns of their separator } */
int sgx_ba_debug_set_init(int mode);               /* test tap: initialisation of the reduced camera system when the envelope solver runs: 0 only the solver's tiles (default), 1 the whole matrix, 2 the whole matrix NaN first, then the tiles, 3 as 2 and every double / float array of the arena that is not an input filled with 0xFF bytes (NaN) after the upload and before the first kernel, whichever solver runs; the integer arrays are left alone */
int sgx_ba_debug_set_jobs(int host);               /* test tap: 1 = the bundle adjustments of this thread build their Schur job list on the host (A/B arm of the device builder), 0 = on the device (default) */
int sgx_ba_debug_set_solver(int mode);             /* test / tuning tap: reduced-camera-system solver of the bundle adjustments: -1 default (SGX_BA_SOLVER or auto), 0 auto, 1 dense blocked Cholesky, 2 envelope solver */
int sgx_det_debug_read_blob(sgx_det *h, const char *blob_name, int image, float *dst, int cap, int *n);
int sgx_flow_debug_read_level(sgx_flow *h, int slot, int frame, int level, uint8_t *img);     /* test tap: pyramid level, w*h tight */
int sgx_flow_debug_read_slot(sgx_flow *h, int slot, int frame, int level, uint8_t *img, int32_t *pitch);   /* test tap: the level as stored (pitch*h, padding columns included); img == NULL: pitch only */
int sgx_flow_debug_level_size(const sgx_flow *h, int level, int32_t *w, int32_t *hgt);
/* test tap: one step of the device EPnP (sg_slam_amd/csrc/sgx_pnp_kernels.h) on caller values, on one lane: which = 0 runs gauss_newton (five steps, no update on a singular
 * qr_solve) on betas in place; which = 1..3 writes find_betas_approx_<which> (IEEE division by betas[0]).  L = 6 x 10, rho = 6, betas = 4 doubles (host arrays). */
int sgx_pnp_debug_betas(int which, const double *L, const double *rho, double *betas);
/* test tap: the per-point state of job `job` of the handle's last batch, over its *n crop points in the reference's order (ascending flat index): kept[i] = the
 * outlier filter kept point i, labels[i] = the smallest point of its component (-1 when the point was removed).  Synchronises; SGX_ERR_OVERFLOW when *n > cap. */
int sgx_obj3d_debug_read(sgx_obj3d *h, int job, uint8_t *kept, int32_t *labels, int cap, int *n);
/* test tap: keyframe `image` of the handle's last batch before the outlier filter: its *n voxel points in ascending idx (mode's frame: camera axes in SGX_CLOUD_LOCAL,
 * ROS axes in SGX_CLOUD_WORLD), dist[i] = the mean distance of point i to its mean_k nearest neighbours, kept[i] = the filter kept it (each destination may be NULL).
 * Synchronises; SGX_ERR_OVERFLOW when *n > cap. */
int sgx_cloud_debug_read(sgx_cloud *h, int image, sgx_cloud_point *voxels, float *dist, uint8_t *kept, int cap, int *n);
/* test tap: the handle's last consolidation before the outlier filter: its *n voxel points in ascending idx, dist and kept as above, tier[i] = the cell radius of the
 * window that was proven for point i (the first window's radius, or a doubled one up to SGX_GMAP_MAX_RADIUS), 0 when the point searched the whole voxel cloud (each
 * destination may be NULL).  Synchronises; SGX_ERR_OVERFLOW when *n > cap. */
int sgx_globalmap_debug_read(sgx_globalmap *h, sgx_cloud_point *voxels, float *dist, uint8_t *kept, uint8_t *tier, int cap, int *n);
/* test / tuning tap: the widest window the second search tier may try, 0 .. SGX_GMAP_MAX_RADIUS (the default).  At or below the first window's radius every point
 * that the first window does not prove searches the whole voxel cloud, as the keyframe path does: the A/B of DESIGN.md 9j, and the tests of that path. */
int sgx_globalmap_debug_max_radius(sgx_globalmap *h, int max_radius);
int sgx_debug_corun_bf16(int blocks, int iters, int launches, void *stream);      /* test tap: `launches` launches of a kernel that only issues bf16 matrix products, asynchronous on `stream` (co-runner of the packed-fp32 regression test) */
/* test tap: DetectionOutput + detect() filtering alone on caller-supplied head outputs (host arrays: loc batch x num_priors x 4, conf batch x num_priors x num_class) */
int sgx_det_debug_detection_output(sgx_det *h, const float *loc, const float *conf, int batch, sgx_det_result *results);
/* test tap: number of (frame, class) pairs of this handle's last DetectionOutput that the per-frame cut sent through the continuation (0 with SGX_DET_OUT_SINGLE) */
int sgx_det_debug_continued(sgx_det *h, int *count);
/* test / tuning taps.  Every sgx_*_debug_set_* setting is PER CALLING THREAD (thread_local): it affects the next create / call made by the same thread only, so the taps
 * cannot leak into the Tracking, Detector2D or LocalMapping thread of a host program; the SGX_* environment switches are read once and never written.
 * set_fusion(0) makes the NEXT sgx_det_create build the unfused plan (one kernel per ncnn layer, every blob
 * materialised) — the fused plan (default) must reproduce it bit for bit.  time_ops: HIP-event time per plan step (ms[0] = pre-processing). */
int sgx_det_debug_set_fusion(int on);
int sgx_det_debug_set_irb(int on);                 /* the NEXT sgx_det_create: matrix-core inverted-residual block kernels (sgx_det_irb.h) 0 off, 1 on the shapes where they beat the per-layer kernels, 2 on every supported shape, -1 = default (1, or SGX_DET_IRB); bit-identical either way */
int sgx_det_debug_set_block_fusion(int on);        /* 1: the NEXT sgx_det_create also fuses every expand -> depthwise -> project triple into one kernel (bit-identical; opt-in: slower at batch 256) */
int sgx_det_debug_set_gemm(int mode);
int sgx_det_debug_set_legacy_kernels(int on);      /* 1: run the simple reference kernels (one thread per output / 64x64 GEMM tile) instead of the tuned ones */
int sgx_det_debug_time_ops(sgx_det *h, const uint8_t *d_img, int pitch, int batch, int reps, float *ms, int cap, int *nops);
int sgx_det_debug_run_step(sgx_det *h, const uint8_t *d_img, int pitch, int batch, int step, int reps, void *stream);      /* plan step `step` launched reps times on `stream`, asynchronously (interference experiments) */
/* run the octree-distribution kernel alone on packed candidates (x | y<<12 | score<<24, coordinates
 * relative to the (16,16) border origin) for `level`; returns the selected packed entries in list order */
int sgx_orb_debug_run_octree(sgx_orb *h, int level, const uint32_t *packed, int n, uint32_t *out_sel, int cap, int *nsel);
/* test tap: what sgx_orb_create decided (sgx_orb_plan.h), one section per call; the tables are read back from the handle's device copies.  section: 0 SgxOrbGeom,
 * 1 SgxRun list, 2 SgxBlurTile list, 3 the levels' SgxXTab tables (levels 1.. in order), 4 the levels' SgxYTab tables as k_resize sees them, 5 SgxXGroup list,
 * 6 the concatenated SgxYTab table of the fused pyramid, 7 SgxPyrRect list, 8 { SgxPyrTabs, pyr_tiles, pyr_lds, oct_maxlim, 0, packed umax (64 bits) }.
 * *bytes = the section's size; dst == NULL asks for the size only, cap < *bytes is SGX_ERR_OVERFLOW.  Synchronises. */
int sgx_orb_debug_read_plan(const sgx_orb *h, int section, void *dst, size_t cap, size_t *bytes);
/* test / A-B tap: 1 = the NEXT sgx_tracker_create of this thread builds a tracker that orients and describes every raw keypoint before the dynamic mask (one-shot
 * extraction, descriptor rows moved by the erase step) instead of the survivors after it; 0 = the product order; -1 = default (SGX_TRK_DESCRIBE_EARLY set, or the product
 * order).  Bit-identical results either way. */
int sgx_tracker_debug_set_describe_early(int on);
/* test tap: person rectangles for the following steps of a tracker created WITHOUT a detector (host arrays: streams x max_boxes x (x, y, w, h), streams counts, streams
 * have-dynamic flags), in place of the empty set it would mask with.  Synchronises. */
int sgx_tracker_debug_set_boxes(sgx_tracker *t, const float *boxes, const int32_t *nboxes, const int32_t *have_dynamic);
/* test tap: reads and clears the tracker's log of everything that orders its streams since it was created, three int32 per entry: (op, stream, event).  op: 0 event
 * record, 1 stream waits for event, 2 host waits for event, 3 host waits for stream, 4 device synchronisation, 5 mark — a fixed point of the step's schedule on `stream`,
 * whose id stands in the event field: 1 before the detector forward, 2 ORB detect / extract, 3 the dynamic mask, 4 the stereo / undistort kernel, 5 the motion model,
 * 6 unproject, 7 the two upload copies, 8 the gray conversion, 9 the pack kernel.  Streams and events are numbered in order of their first appearance in the tracker's
 * log (caller streams included); the host is stream -1, and an entry without an event has -1 there.  *n = the number of int32 values; dst == NULL asks for the size only
 * and keeps the log, cap < *n is SGX_ERR_OVERFLOW.  The emulator gives the numbers of the device build: its streams and events are distinct tokens there. */
int sgx_tracker_debug_sync_trace(sgx_tracker *t, int32_t *dst, int cap, int *n);
/* test tap, PER CALLING THREAD: the n-th acquisition or checked call made by the sgx_tracker_* entries of this thread from now on fails as if the runtime had refused it —
 * a device or pinned allocation with SGX_ERR_NOMEM, a stream or event creation or a checked launch / copy / synchronisation with SGX_ERR_DEVICE.  n <= 0 turns it off.
 * Returns the status that the previous arming delivered, SGX_OK when it never fired. */
int sgx_tracker_debug_fail_after(int n);
/* test tap, PER CALLING THREAD: the same for the handles whose device buffers one owner holds (sg_slam_amd/csrc/sgx_devmem.h: the ORB extractor, the detector, the
 * vocabulary, the keyframe database, PnP, Initializer, Sim3Solver and Detector3D handles).  The n-th acquisition from now on fails as if the runtime had refused it — an
 * allocation with SGX_ERR_NOMEM, the copy of a table or input uploaded at creation with SGX_ERR_DEVICE.  n <= 0 turns it off.  Returns the status that the previous
 * arming delivered, SGX_OK when it never fired. */
int sgx_debug_devmem_fail_after(int n);
/* test tap: left frame `frame` of the handle's last sgx_stereo_match_batch_dev, one entry per keypoint slot (cap of them; each destination may be NULL): bestIdxR and
 * the Hamming bestDist of the row-table search (0 / 100 where it found none), the exit the keypoint took (-1 no keypoint, 0 no candidates on its row, 1 maxU < 0,
 * 2 bestDist >= 75, 3 the reference's border test, 4 a window outside its level, 5 bestincR at the end of the range, 6 deltaR outside [-1, 1], 7 disparity outside
 * [0, maxD), 8 accepted, 9 accepted with the disparity == 0 clamp, 10 accepted and reset by the median cut), bestincR (0 where the window search did not run) and the
 * 11 SAD values (cap x 11, -1 where it did not run).  Synchronises. */
int sgx_stereo_debug_read(sgx_stereo *h, int frame, int32_t *best_idx, int32_t *best_dist, int32_t *exit_code, int32_t *best_inc, int32_t *sads);

#ifdef __cplusplus
}
#endif
#endif
