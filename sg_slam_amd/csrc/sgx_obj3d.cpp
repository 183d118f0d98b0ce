// sgx_obj3d.cpp — host side of Detector3D (src/sg-slam/src/Detector3D.cc) and ObjectDatabase (src/sg-slam/src/ObjectDatabase.cc) behind the C ABI: the handle owns the
// per-job workspace; detect_batch_dev validates the jobs, stages their records and enqueues the kernels of sgx_obj3d_kernels.h on the caller's stream; the single
// detect is a batch of one fed from host memory.  ObjectDatabase::addObject is host code.
#include "sgx_obj3d_kernels.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#ifdef SGX_DEBUG_TAPS
#include "../../include/sgx_debug.h"      // test taps: compiled into tests/taps/libsgx_taps.so and the emulator only
#endif

static_assert(sizeof(SgxObjResult) == sizeof(sgx_obj3d_result), "the kernels write sgx_obj3d_result");

struct sgx_obj3d {
    int width = 0, height = 0, max_images = 0, max_jobs = 0, cap = 0, slot_cap = 0;
    sgx_obj3d_params p;
    std::vector<SgxObjJob> jobs_h;                       // the jobs of the last batch (the tap reads their geometry)
    SgxObjJob *jobs = nullptr;
#ifndef SGX_EMU
    SgxObjJob *pinned = nullptr; hipEvent_t staged = nullptr; bool pending = false;      // host staging of the job records: refilled only after the previous upload has left it
#endif
    float *wx = nullptr, *wy = nullptr, *wz = nullptr, *dist = nullptr, *scen = nullptr;
    int *state = nullptr, *parent = nullptr, *label = nullptr, *csize = nullptr, *ji = nullptr, *sroot = nullptr, *ssize = nullptr, *smm = nullptr, *sorder = nullptr;
    double *jd = nullptr;
    float *one_depth = nullptr; double *one_twc = nullptr; SgxObjResult *one_result = nullptr;      // the synchronous entry's staging
    SgxDevMem mem;
#ifndef SGX_EMU
    ~sgx_obj3d()
    {
        if (pinned) (void)hipHostFree(pinned);
        if (staged) (void)hipEventDestroy(staged);
    }
#endif
};

static bool obj_finite(double v) { return v == v && v - v == 0; }

// the per-job workspace, the synchronous entry's staging, the pinned job records and their event
static int obj_allocate(sgx_obj3d *h)
{
    const size_t J = (size_t)h->max_jobs, P = J * (size_t)h->cap, S = J * (size_t)h->slot_cap;
    SgxDevMem &m = h->mem;
    int rc;
    if ((rc = m.alloc(&h->jobs, J)) || (rc = m.alloc(&h->wx, P)) || (rc = m.alloc(&h->wy, P)) || (rc = m.alloc(&h->wz, P)) || (rc = m.alloc(&h->dist, P)) ||
        (rc = m.alloc(&h->state, P)) || (rc = m.alloc(&h->parent, P)) || (rc = m.alloc(&h->label, P)) || (rc = m.alloc(&h->csize, P)) || (rc = m.alloc(&h->ji, SGX_OBJ_JI * J)) ||
        (rc = m.alloc(&h->jd, SGX_OBJ_JD * J)) || (rc = m.alloc(&h->sroot, S)) || (rc = m.alloc(&h->ssize, S)) || (rc = m.alloc(&h->smm, SGX_OBJ_MM * S)) ||
        (rc = m.alloc(&h->sorder, S)) || (rc = m.alloc(&h->scen, 3 * S)) ||
        (rc = m.alloc(&h->one_depth, (size_t)h->width * h->height)) || (rc = m.alloc(&h->one_twc, 16)) || (rc = m.alloc(&h->one_result, 1))) return rc;
#ifndef SGX_EMU
    if (hipHostMalloc((void **)&h->pinned, sizeof(SgxObjJob) * J, hipHostMallocDefault) != hipSuccess) return SGX_ERR_NOMEM;
    if (hipEventCreateWithFlags(&h->staged, hipEventDisableTiming) != hipSuccess) return SGX_ERR_DEVICE;
#endif
    return SGX_OK;
}

extern "C" int sgx_obj3d_create(int width, int height, int max_images, int max_jobs, int max_crop_points, const sgx_obj3d_params *params, sgx_obj3d **out)
{
    if (out) *out = nullptr;
    if (!out || !params || width < 1 || height < 1 || max_images < 1 || max_jobs < 1 || max_crop_points < 0) return SGX_ERR_INVALID;
    if (params->sor_mean_k < 1 || !obj_finite(params->camera_valid_depth_min) || !obj_finite(params->camera_valid_depth_max) || !obj_finite(params->cluster_tolerance))
        return SGX_ERR_INVALID;
    if (max_crop_points == 0) {                          // the largest crop: Detector2D only clamps its boxes to the image, so a box can be the whole image
        const long long cw = (long long)((double)width * 0.8) - (long long)((double)width * 0.2), ch = (long long)((double)height * 0.8) - (long long)((double)height * 0.2);
        max_crop_points = cw * ch > 0 ? (int)(cw * ch) : 1;
    }
    sgx_obj3d *h = new sgx_obj3d;
    h->width = width; h->height = height; h->max_images = max_images; h->max_jobs = max_jobs; h->cap = max_crop_points; h->p = *params;
    h->slot_cap = max_crop_points / (params->cluster_min_size > 1 ? params->cluster_min_size : 1) + 1;       // a surviving cluster has at least min_size points
    const int rc = obj_allocate(h);
    if (rc != SGX_OK) { delete h; return rc; }
    *out = h;
    return SGX_OK;
}

extern "C" void sgx_obj3d_destroy(sgx_obj3d *h) { delete h; }

// the crop of Detector3D.cc:47-58 as a cell grid; a rect that is not inside the image is an error (Detector2D's clamp keeps every rect inside)
static int obj_job(const sgx_obj3d *h, const sgx_obj3d_job &in, int n_images, SgxObjJob *o)
{
    if (in.image < 0 || in.image >= n_images) return SGX_ERR_INVALID;
    if (!(in.x >= 0 && in.y >= 0 && in.w >= 0 && in.h >= 0 && in.x + in.w <= (float)h->width && in.y + in.h <= (float)h->height)) return SGX_ERR_INVALID;
    const size_t row_beg = (size_t)((double)(size_t)in.h * 0.2), row_end = (size_t)((double)(size_t)in.h * 0.8);       // (size_t)rect2d.height*0.2: the cast binds first
    const size_t col_beg = (size_t)((double)(size_t)in.w * 0.2), col_end = (size_t)((double)(size_t)in.w * 0.8);
    o->image = in.image; o->class_id = in.class_id; o->prob = in.prob; o->rx = in.x; o->ry = in.y; o->rw = in.w; o->rh = in.h;
    o->x0 = (int)((size_t)in.x + col_beg); o->y0 = (int)((size_t)in.y + row_beg);
    o->cw = (int)(col_end - col_beg); o->ch = (int)(row_end - row_beg);
    if (o->x0 + o->cw > h->width || o->y0 + o->ch > h->height) return SGX_ERR_INVALID;
    if ((long long)o->cw * o->ch > h->cap) return SGX_ERR_INVALID;
    return SGX_OK;
}

static SgxObjArgs obj_args(sgx_obj3d *h, const float *cam4)
{
    SgxObjArgs A; memset(&A, 0, sizeof A);
    const sgx_obj3d_params &p = h->p;
    A.width = h->width; A.height = h->height; A.cap = h->cap; A.slot_cap = h->slot_cap;
    A.mean_k = p.sor_mean_k; A.min_size = p.cluster_min_size; A.max_size = p.cluster_max_size;
    int w0 = 1; while ((2 * w0 + 1) * (2 * w0 + 1) < 2 * (p.sor_mean_k + 1)) w0++;                  // the first window holds twice the neighbours asked for
    A.w0 = w0;
    A.fx = cam4[0]; A.fy = cam4[1]; A.cx = cam4[2]; A.cy = cam4[3]; A.dmin = p.camera_valid_depth_min; A.dmax = p.camera_valid_depth_max;
    A.tol2 = (float)((double)p.cluster_tolerance * (double)p.cluster_tolerance); A.ratio = p.similar_compare_ratio;
    A.mul = p.sor_stddev_mul; A.tol = (double)p.cluster_tolerance;
    // Rmax = the longest ray (x, y, 1) of the image, in normalised coordinates
    const double fx = fabs((double)A.fx), fy = fabs((double)A.fy);
    const double xm = fmax(fabs(0.0 - (double)A.cx), fabs((double)(h->width - 1) - (double)A.cx)) / fx, ym = fmax(fabs(0.0 - (double)A.cy), fabs((double)(h->height - 1) - (double)A.cy)) / fy;
    const double rmax = sqrt(1.0 + xm * xm + ym * ym);
    A.inv_fr = 1.0 / (fmax(fx, fy) * rmax);
    A.dabs_r = fmax(fabs((double)A.dmin), fabs((double)A.dmax)) * rmax;
    if (!obj_finite(A.inv_fr) || !obj_finite(A.dabs_r)) { A.inv_fr = 0; A.dabs_r = 0; }             // a degenerate camera: no window is ever proven
    A.jobs = h->jobs; A.wx = h->wx; A.wy = h->wy; A.wz = h->wz; A.dist = h->dist; A.scen = h->scen; A.state = h->state; A.parent = h->parent; A.label = h->label;
    A.csize = h->csize; A.ji = h->ji; A.sroot = h->sroot; A.ssize = h->ssize; A.smm = h->smm; A.sorder = h->sorder; A.jd = h->jd;
    return A;
}

extern "C" int sgx_obj3d_detect_batch_dev(sgx_obj3d *h, const float *depth_dev, int pitch, int n_images, const float *cam4, const double *twc_dev, const sgx_obj3d_job *jobs,
                                          int n_jobs, sgx_obj3d_result *results_dev, void *stream)
{
    if (!h || !depth_dev || !cam4 || !twc_dev || n_images < 1 || n_images > h->max_images || n_jobs < 0 || n_jobs > h->max_jobs || pitch < h->width) return SGX_ERR_INVALID;
    if (n_jobs == 0) return SGX_OK;
    if (!jobs || !results_dev) return SGX_ERR_INVALID;
    std::vector<SgxObjJob> jh((size_t)n_jobs);
    int cells = 1;
    for (int j = 0; j < n_jobs; j++) {
        const int r = obj_job(h, jobs[j], n_images, &jh[(size_t)j]);
        if (r != SGX_OK) return r;
        if (jh[(size_t)j].cw * jh[(size_t)j].ch > cells) cells = jh[(size_t)j].cw * jh[(size_t)j].ch;
    }
    const sgx_stream_t s = (sgx_stream_t)stream;
    h->jobs_h.swap(jh);
#ifndef SGX_EMU
    if (h->pending) SGX_CHECK_HIP(hipEventSynchronize(h->staged));           // the previous call's upload (not its kernels) has read the staging buffer
    memcpy(h->pinned, h->jobs_h.data(), sizeof(SgxObjJob) * (size_t)n_jobs);
    SGX_CHECK_HIP(hipMemcpyAsync(h->jobs, h->pinned, sizeof(SgxObjJob) * (size_t)n_jobs, hipMemcpyHostToDevice, s));
    SGX_CHECK_HIP(hipEventRecord(h->staged, s)); h->pending = true;
#else
    SGX_CHECK_HIP(hipMemcpyAsync(h->jobs, h->jobs_h.data(), sizeof(SgxObjJob) * (size_t)n_jobs, hipMemcpyHostToDevice, s));
#endif
    SgxObjArgs A = obj_args(h, cam4);
    A.J = n_jobs; A.pitch = pitch; A.depth = depth_dev; A.twc = twc_dev; A.results = (SgxObjResult *)results_dev;
    const dim3 cellgrid((unsigned)((cells + 255) / 256), (unsigned)n_jobs), jobgrid((unsigned)n_jobs);
    SGX_LAUNCH(k_obj3d_prep, dim3((unsigned)((n_jobs + 63) / 64)), dim3(64), s, A);
    SGX_LAUNCH(k_obj3d_points, cellgrid, dim3(256), s, A);
    SGX_LAUNCH(k_obj3d_sor, cellgrid, dim3(256), s, A);
    SGX_LAUNCH(k_obj3d_stats, jobgrid, dim3(256), s, A);
    SGX_LAUNCH(k_obj3d_keep, cellgrid, dim3(256), s, A);
    SGX_LAUNCH(k_obj3d_union, cellgrid, dim3(256), s, A);
    SGX_LAUNCH(k_obj3d_label, cellgrid, dim3(256), s, A);
    SGX_LAUNCH(k_obj3d_slots, cellgrid, dim3(256), s, A);
    SGX_LAUNCH(k_obj3d_minmax, cellgrid, dim3(256), s, A);
    SGX_LAUNCH(k_obj3d_centroid, dim3((unsigned)((h->slot_cap + 63) / 64), (unsigned)n_jobs), dim3(64), s, A);
    SGX_LAUNCH(k_obj3d_select, jobgrid, dim3(64), s, A);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_obj3d_detect(sgx_obj3d *h, const float *depth, const float *cam4, const double *twc, const sgx_obj3d_job *job, sgx_obj3d_result *result)
{
    if (!h || !depth || !cam4 || !twc || !job || !result || job->image != 0) return SGX_ERR_INVALID;
    const size_t px = (size_t)h->width * h->height;
    SGX_CHECK_HIP(hipMemcpy(h->one_depth, depth, 4 * px, hipMemcpyHostToDevice));
    SGX_CHECK_HIP(hipMemcpy(h->one_twc, twc, 8 * 16, hipMemcpyHostToDevice));
    const int r = sgx_obj3d_detect_batch_dev(h, h->one_depth, h->width, 1, cam4, h->one_twc, job, 1, (sgx_obj3d_result *)h->one_result, nullptr);
    if (r != SGX_OK) return r;
    SGX_CHECK_HIP(hipStreamSynchronize((sgx_stream_t)0));
    SGX_CHECK_HIP(hipMemcpy(result, h->one_result, sizeof(SgxObjResult), hipMemcpyDeviceToHost));
    return SGX_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------ ObjectDatabase
struct sgx_objdb {
    int DataBaseSize = 0;
    std::vector<sgx_semantic_object> objs;
    float mvSizes[21];
    sgx_objdb() { for (int i = 0; i < 21; i++) mvSizes[i] = 0.6f; mvSizes[5] = 0.2f; mvSizes[9] = 1.0f; mvSizes[20] = 0.5f; }       // ObjectDatabase.cc:21-27
};

extern "C" int sgx_objdb_create(sgx_objdb **out)
{
    if (!out) return SGX_ERR_INVALID;
    *out = new sgx_objdb;
    return SGX_OK;
}

extern "C" void sgx_objdb_destroy(sgx_objdb *db) { delete db; }

extern "C" int sgx_objdb_size(const sgx_objdb *db) { return db ? (int)db->objs.size() : SGX_ERR_INVALID; }

extern "C" int sgx_objdb_get(const sgx_objdb *db, int index, sgx_semantic_object *out)
{
    if (!db || !out || index < 0 || index >= (int)db->objs.size()) return SGX_ERR_INVALID;
    *out = db->objs[(size_t)index];
    return SGX_OK;
}

// ObjectDatabase::addObject (:44-112).  The reference matches by object_name = class_names[class_id], which is one to one with the class id
extern "C" int sgx_objdb_add(sgx_objdb *db, const sgx_semantic_object *obj, int32_t *object_id, int32_t *merged)
{
    if (!db || !obj || obj->class_id < 0 || obj->class_id > 20) return SGX_ERR_INVALID;         // mvSizes has 21 entries
    sgx_semantic_object c = *obj;
    int best = -1; float center_distance = 100;
    for (size_t i = 0; i < db->objs.size(); i++) {
        const sgx_semantic_object &t = db->objs[i];
        if (t.class_id != c.class_id) continue;
        const float dx = c.centroid[0] - t.centroid[0], dy = c.centroid[1] - t.centroid[1], dz = c.centroid[2] - t.centroid[2];
        const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
        if (dist < center_distance) { center_distance = dist; best = (int)i; }
    }
    if (best >= 0 && center_distance < db->mvSizes[c.class_id]) {                               // the same object: a mean of the old and the new
        sgx_semantic_object &b = db->objs[(size_t)best];
        b.prob = (float)((double)(b.prob + c.prob) / 2.0);
        for (int i = 0; i < 3; i++) { b.centroid[i] = (b.centroid[i] + c.centroid[i]) / 2.0f; b.size[i] = (b.size[i] + c.size[i]) / 2.0f; }
        if (object_id) *object_id = b.object_id;
        if (merged) *merged = 1;
        return SGX_OK;
    }
    db->DataBaseSize++;
    c.object_id = db->DataBaseSize;
    db->objs.push_back(c);
    if (object_id) *object_id = c.object_id;
    if (merged) *merged = 0;
    return SGX_OK;
}

#ifdef SGX_DEBUG_TAPS
// test tap: the per-point results of job `job` of the handle's last batch, over its crop points in the reference's order: kept[i] = the filter kept point i,
// labels[i] = the smallest point of its component (-1 when not kept).  Synchronises the device.
SGX_TAP int sgx_obj3d_debug_read(sgx_obj3d *h, int job, uint8_t *kept, int32_t *labels, int cap, int *n)
{
    if (!h || job < 0 || job >= (int)h->jobs_h.size() || !n || cap < 0) return SGX_ERR_INVALID;
    SGX_CHECK_HIP(hipDeviceSynchronize());
    const int G = h->jobs_h[(size_t)job].cw * h->jobs_h[(size_t)job].ch;
    std::vector<int> st((size_t)(G > 0 ? G : 1)), lb(st.size()), rank(st.size(), -1);
    if (G > 0) {
        SGX_CHECK_HIP(hipMemcpy(st.data(), h->state + (size_t)job * h->cap, 4 * (size_t)G, hipMemcpyDeviceToHost));
        SGX_CHECK_HIP(hipMemcpy(lb.data(), h->label + (size_t)job * h->cap, 4 * (size_t)G, hipMemcpyDeviceToHost));
    }
    int m = 0;
    for (int c = 0; c < G; c++) if (st[(size_t)c] & SGX_OBJ_VALID) rank[(size_t)c] = m++;
    *n = m;
    if (m > cap) return SGX_ERR_OVERFLOW;
    for (int c = 0; c < G; c++) {
        const int i = rank[(size_t)c];
        if (i < 0) continue;
        const bool k = (st[(size_t)c] & SGX_OBJ_KEEP) != 0;
        if (kept) kept[i] = k ? 1 : 0;
        if (labels) labels[i] = k ? rank[(size_t)lb[(size_t)c]] : -1;
    }
    return SGX_OK;
}
#endif
