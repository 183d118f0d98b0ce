// sgx_loop_sim3.cpp — the Sim3 glue of loop closing behind the C ABI (sgx_loop_propagate_sim3, sgx_eg_flatten, sgx_eg_recover, sgx_correct_map_points_dev): the kernels
// of sgx_loop_sim3_kernels.h, built with -ffp-contract=off like every bit-exact feature unit.
#include "sgx_loop_sim3_kernels.h"
#include "sgx_devmem.h"
#include "../../include/sgx.h"
#include <stdio.h>

// the device buffers of one host-pointer call
struct DevBufs {
    SgxDevMem m; int rc = SGX_OK;                          // rc: the first failure; requests after it do nothing, so the caller checks once after the last
    template <class T> void get(T **out, size_t n) { *out = nullptr; if (rc == SGX_OK) rc = m.alloc(out, n); }
    template <class T> void put(T **out, const T *src, size_t n) { *out = nullptr; if (rc == SGX_OK) rc = m.upload(out, src, n); }
};

// ---- device pointers on a stream, and the same from host memory
#define EG_GRID(n) dim3((unsigned)(((n) + SGX_EG_THREADS - 1) / SGX_EG_THREADS))
extern "C" int sgx_loop_propagate_sim3_dev(int n_group, const float *Tcw_dev, const double *Scw_dev, double *noncorrected_dev, double *corrected_dev, float *corrected_Tiw_dev, void *stream)
{
    if (n_group < 1 || !Tcw_dev || !Scw_dev || !noncorrected_dev || !corrected_dev || !corrected_Tiw_dev) return SGX_ERR_INVALID;
    SGX_LAUNCH(k_loop_propagate, EG_GRID(n_group), dim3(SGX_EG_THREADS), (sgx_stream_t)stream, n_group, Tcw_dev, Scw_dev, noncorrected_dev, corrected_dev, corrected_Tiw_dev);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_eg_flatten_dev(int nv, const int32_t *vertex_group_dev, const float *Tcw_dev, int n_group, const double *corrected_dev, const double *noncorrected_dev, int ne,
                                  const int32_t *e_i_dev, const int32_t *e_j_dev, const uint8_t *e_kind_dev, double *S_in_dev, double *e_meas_dev, void *stream)
{
    if (nv < 0 || ne < 0 || n_group < 0 || (nv > 0 && (!vertex_group_dev || !Tcw_dev || !S_in_dev)) || (n_group > 0 && (!corrected_dev || !noncorrected_dev)) ||
        (ne > 0 && (nv == 0 || !e_i_dev || !e_j_dev || !e_kind_dev || !e_meas_dev))) return SGX_ERR_INVALID;
    const sgx_stream_t s = (sgx_stream_t)stream;
    if (nv) SGX_LAUNCH(k_loop_flatten_vertices, EG_GRID(nv), dim3(SGX_EG_THREADS), s, nv, (const int *)vertex_group_dev, Tcw_dev, corrected_dev, S_in_dev);
    if (ne) SGX_LAUNCH(k_loop_flatten_edges, EG_GRID(ne), dim3(SGX_EG_THREADS), s, ne, (const int *)e_i_dev, (const int *)e_j_dev, e_kind_dev, (const int *)vertex_group_dev,
                       (const double *)S_in_dev, noncorrected_dev, e_meas_dev);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_eg_recover_dev(int nv, const double *S_out_dev, float *Tcw_dev, double *corrected_Swc_dev, void *stream)
{
    if (nv < 0 || (nv > 0 && (!S_out_dev || !Tcw_dev || !corrected_Swc_dev))) return SGX_ERR_INVALID;
    if (nv) SGX_LAUNCH(k_loop_recover, EG_GRID(nv), dim3(SGX_EG_THREADS), (sgx_stream_t)stream, nv, S_out_dev, Tcw_dev, corrected_Swc_dev);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_correct_map_points_dev(int n, const float *xw_dev, const int32_t *ref_dev, const double *Srw_dev, const double *corrected_Swr_dev, float *xw_out_dev, void *stream)
{
    if (n < 0 || (n > 0 && (!xw_dev || !ref_dev || !Srw_dev || !corrected_Swr_dev || !xw_out_dev))) return SGX_ERR_INVALID;
    if (n) SGX_LAUNCH(k_loop_correct_points, EG_GRID(n), dim3(SGX_EG_THREADS), (sgx_stream_t)stream, n, xw_dev, (const int *)ref_dev, Srw_dev, corrected_Swr_dev, xw_out_dev);
    SGX_CHECK_HIP(hipGetLastError());
    return SGX_OK;
}

extern "C" int sgx_loop_propagate_sim3(int n_group, const float *Tcw, const double *Scw, double *noncorrected, double *corrected, float *corrected_Tiw)
{
    if (n_group < 1 || !Tcw || !Scw || !noncorrected || !corrected || !corrected_Tiw) return SGX_ERR_INVALID;
    const size_t n = (size_t)n_group;
    DevBufs D; float *dT, *dO; double *dS, *dn, *dc;
    D.put(&dT, Tcw, 12 * n); D.put(&dS, Scw, 8); D.get(&dn, 8 * n); D.get(&dc, 8 * n); D.get(&dO, 12 * n);
    if (D.rc != SGX_OK) return D.rc;
    const int rc = sgx_loop_propagate_sim3_dev(n_group, dT, dS, dn, dc, dO, nullptr);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_HIP(hipMemcpy(noncorrected, dn, sizeof(double) * 8 * n, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(corrected, dc, sizeof(double) * 8 * n, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(corrected_Tiw, dO, sizeof(float) * 12 * n, hipMemcpyDeviceToHost));
    return SGX_OK;
}

extern "C" int sgx_eg_flatten(int nv, const int32_t *vertex_group, const float *Tcw, int n_group, const double *corrected, const double *noncorrected, int ne, const int32_t *e_i,
                              const int32_t *e_j, const uint8_t *e_kind, double *S_in, double *e_meas)
{
    if (nv < 0 || ne < 0 || n_group < 0 || (nv > 0 && (!vertex_group || !Tcw || !S_in)) || (n_group > 0 && (!corrected || !noncorrected)) ||
        (ne > 0 && (!e_i || !e_j || !e_kind || !e_meas))) return SGX_ERR_INVALID;
    for (int v = 0; v < nv; v++) if (vertex_group[v] < -1 || vertex_group[v] >= n_group) return SGX_ERR_INVALID;
    for (int k = 0; k < ne; k++) if (e_i[k] < 0 || e_i[k] >= nv || e_j[k] < 0 || e_j[k] >= nv || e_kind[k] > 3) return SGX_ERR_INVALID;
    DevBufs D; int32_t *dg, *di, *dj; uint8_t *dk; float *dT; double *dc, *dn, *dS, *dm;
    D.put(&dg, vertex_group, (size_t)nv); D.put(&dT, Tcw, 12 * (size_t)nv); D.put(&dc, corrected, 8 * (size_t)n_group); D.put(&dn, noncorrected, 8 * (size_t)n_group);
    D.put(&di, e_i, (size_t)ne); D.put(&dj, e_j, (size_t)ne); D.put(&dk, e_kind, (size_t)ne); D.get(&dS, 8 * (size_t)nv); D.get(&dm, 8 * (size_t)ne);
    if (D.rc != SGX_OK) return D.rc;
    const int rc = sgx_eg_flatten_dev(nv, dg, dT, n_group, dc, dn, ne, di, dj, dk, dS, dm, nullptr);
    if (rc != SGX_OK) return rc;
    if (nv) SGX_CHECK_HIP(hipMemcpy(S_in, dS, sizeof(double) * 8 * (size_t)nv, hipMemcpyDeviceToHost));
    if (ne) SGX_CHECK_HIP(hipMemcpy(e_meas, dm, sizeof(double) * 8 * (size_t)ne, hipMemcpyDeviceToHost));
    return SGX_OK;
}

extern "C" int sgx_eg_recover(int nv, const double *S_out, float *Tcw, double *corrected_Swc)
{
    if (nv < 0 || (nv > 0 && (!S_out || !Tcw || !corrected_Swc))) return SGX_ERR_INVALID;
    if (nv == 0) return SGX_OK;
    DevBufs D; double *dS, *dc; float *dT;
    D.put(&dS, S_out, 8 * (size_t)nv); D.get(&dT, 12 * (size_t)nv); D.get(&dc, 8 * (size_t)nv);
    if (D.rc != SGX_OK) return D.rc;
    const int rc = sgx_eg_recover_dev(nv, dS, dT, dc, nullptr);
    if (rc != SGX_OK) return rc;
    SGX_CHECK_HIP(hipMemcpy(Tcw, dT, sizeof(float) * 12 * (size_t)nv, hipMemcpyDeviceToHost));
    SGX_CHECK_HIP(hipMemcpy(corrected_Swc, dc, sizeof(double) * 8 * (size_t)nv, hipMemcpyDeviceToHost));
    return SGX_OK;
}
