// sgx_covis_loop_kernels.h — loop closing on the covisibility handle: the group and the point marks of LoopClosing::CorrectLoop (src/sg-slam/src/LoopClosing.cc:432-436,
// :472-516), its LoopConnections (:546-564), and the vertex and edge loops of Optimizer::OptimizeEssentialGraph (Optimizer.cc:797-983) with sInsertedEdges and
// KeyFrame::GetCovisiblesByWeight (KeyFrame.cc:185-200) as written.  Everything is integer.  Orders come from keys: a group member's place in a map<KeyFrame*, ...> is its
// rank by id, a target's place in a set<KeyFrame*> is its id, a list entry's place is its rank by (weight, id); nothing is taken from arrival.
//
// The UpdateConnections calls of the two CorrectLoop phases are k_covis_count for all members at once (a count reads the relation only) and then sgx_covis_apply_one for
// the members in the reference's order by ONE workgroup, the scheme of k_covis_apply: a later member's overwrite of its row and an earlier member's AddConnection into it
// touch the same words.
#pragma once
#include "sgx_covis_kernels.h"

enum { SGX_COVIS_EG_MINFEAT = 100 };                                                      // minFeat of Optimizer.cc:807
enum { LS_VALID = 0, LS_NGROUP, LS_E0, LS_K1, LS_K2, LS_K3, LS_TMP, LS_FIELDS = 8 };      // scalars between the kernels of one sequence

struct SgxCovisLoopReport {               // sgx_covis_loop_report
    int status, n_group, n_points, n_connections, n_vertices, n_edges, n_kind[4];
};

struct SgxCovisLoopArgs {
    int cur, loop, n_group, n_le, lcap, pcap, ecap;
    const int *le;                        // mspLoopEdges as slot pairs, n_le of them
    int *s;                               // LS_*
    int *qkf, *ord;                       // the ids of the UpdateConnections queries; a scratch ordered list
    int *gslot, *grank, *rowg, *gof;      // group index -> slot, group index -> rank by id, rank -> group index, slot -> group index (-1 none)
    int *vidx, *vcnt, *vbase;             // slot -> vertex; per vertex (per rank in loop_connections) a count and its exclusive prefix
    int *flags;                           // max_kf rows of max_kf: the count rows of the UpdateConnections queries, then the LoopConnections marks of each member
    int *group_id, *group_vertex, *point_id, *point_ref, *lc_begin, *lc_j, *vertex_id, *vertex_group, *e_i, *e_j;
    unsigned char *vertex_fixed, *e_kind;
    SgxCovisLoopReport *report;
};

SGX_DEV int sgx_covis_vertex_of(const SgxCovisArgs &A, int id)             // index of a live keyframe among the live ones in ascending id, -1 if there is none
{
    int lo = 0, hi = A.nlive;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.sorted_id[mid] < id) lo = mid + 1; else hi = mid; }
    return lo < A.nlive && A.sorted_id[lo] == id ? lo : -1;
}

SGX_DEV bool sgx_covis_is_loop_edge(const SgxCovisLoopArgs &L, int a, int b)
{
    for (int k = 0; k < L.n_le; k++) if ((L.le[2 * k] == a && L.le[2 * k + 1] == b) || (L.le[2 * k] == b && L.le[2 * k + 1] == a)) return true;
    return false;
}

// dst[0] = first, dst[1 .. n) = rest
SGX_KERNEL(256) k_covis_loop_fill(int *dst, int n, int first, int rest)
{
    SGX_THREADS_BEGIN(tid)
    const int j = (int)blockIdx.x * 256 + tid;
    if (j < n) dst[j] = j ? rest : first;
    SGX_THREADS_END
}

// ------------------------------------------------------------------------------------------------------------------------------------------ CorrectLoop :432-436
// mvpCurrentConnectedKFs = GetVectorCovisibleKeyFrames() in list order without the isBad() entries (rule 11), then the current keyframe; every member's rank by id (its
// place in CorrectedSim3), its vertex, the queries of the UpdateConnections pass in ascending id, and the list of the point marks (position = rank).  One workgroup.
SGX_KERNEL(256) k_covis_loop_group(SgxCovisArgs A, SgxCovisLoopArgs L)
{
    SGX_LDS int s_part[256];
    SGX_LDS int s_ng;
    const int s = sgx_covis_lookup(A, L.cur);                               // live: the host looked
    sgx_covis_ordered_wg(A, s, A.max_kf, L.ord, nullptr, &L.s[LS_TMP]);
    const int n = L.s[LS_TMP] < A.max_kf ? L.s[LS_TMP] : A.max_kf - 1, seg = (n + 255) / 256;
    SGX_THREADS_BEGIN(tid)
    int c = 0;
    for (int r = tid * seg; r < n && r < (tid + 1) * seg; r++) c += A.kf[L.ord[r] * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE;
    s_part[tid] = c;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) { int o = 0; for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; } s_ng = o + 1; L.gslot[o] = s; L.group_id[o] = L.cur; }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int o = s_part[tid];
    for (int r = tid * seg; r < n && r < (tid + 1) * seg; r++) {
        const int t = L.ord[r];
        if (A.kf[t * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE) { L.gslot[o] = t; L.group_id[o] = A.kf[t * CV_FIELDS + CV_ID]; o++; }
    }
    SGX_THREADS_END
    SGX_SYNC();
    const int ng = s_ng;
    SGX_THREADS_BEGIN(tid)
    for (int g = tid; g < ng; g += 256) {
        const int id = L.group_id[g];
        int rank = 0;
        for (int m = 0; m < ng; m++) rank += L.group_id[m] < id;
        L.grank[g] = rank; L.rowg[rank] = g; L.qkf[rank] = id; A.ws_lkf[rank] = L.gslot[g];
        L.group_vertex[g] = sgx_covis_vertex_of(A, id);
    }
    for (int r = ng + tid; r < A.nlive; r += 256) L.qkf[r] = -1;             // no keyframe: the query does nothing
    if (tid == 0) { A.ws_q[CQ_VALID] = 1; A.ws_q[CQ_NL] = ng; L.s[LS_NGROUP] = ng; }
    SGX_THREADS_END
}

// The existing points of the group with mnCorrectedReference (:480-500): the first occurrence over the members in ascending id, then index order (k_covis_lm_stamp with
// position = rank), emitted as k_covis_ba_points does it; point_ref is the member's index in the group row.  The last position leaves the report.
SGX_KERNEL(256) k_covis_loop_points(SgxCovisArgs A, SgxCovisLoopArgs L)
{
    SGX_LDS int s_part[256];
    SGX_LDS int s_base;
    const int nl = A.ws_q[CQ_NL];
    const int *stamp = A.stamp, *pcnt = A.ws_pcnt;
    for (int pos = (int)blockIdx.x; pos < nl; pos += (int)gridDim.x) {
        const int k = A.ws_lkf[pos];
        const int np = A.kf[k * CV_FIELDS + CV_N], seg = (np + 255) / 256;
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int j = tid; j < pos; j += 256) c += pcnt[j];
        s_part[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { int b = 0; for (int i = 0; i < 256; i++) b += s_part[i]; s_base = b; }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int i = tid * seg; i < np && i < (tid + 1) * seg; i++) { const int p = A.heap[A.o_mp + (size_t)k * A.cap + i]; if (p >= 0 && stamp[p] == pos * A.cap + i) c++; }
        s_part[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            int o = s_base;
            for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; }
            if (pos == nl - 1) { SgxCovisLoopReport R = {}; R.status = o > L.pcap ? -3 : 0; R.n_group = nl; R.n_points = o; *L.report = R; }      // SGX_ERR_NOMEM
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int o = s_part[tid];
        for (int i = tid * seg; i < np && i < (tid + 1) * seg; i++) {
            const int p = A.heap[A.o_mp + (size_t)k * A.cap + i];
            if (p >= 0 && stamp[p] == pos * A.cap + i) { if (o < L.pcap) { L.point_id[o] = p; L.point_ref[o] = L.rowg[pos]; } o++; }
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------ the group row as an input
// The caller's group row: every id a live keyframe, no id twice, the current keyframe last.  Leaves gslot, grank, rowg, gof and LS_VALID; by the calling workgroup.
SGX_DEV void sgx_covis_loop_rows(const SgxCovisArgs &A, const SgxCovisLoopArgs &L)
{
    SGX_LDS int s_bad;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) s_bad = L.group_id[L.n_group - 1] != L.cur;
    for (int t = tid; t < A.nslots; t += 256) L.gof[t] = -1;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int bad = 0;
    for (int g = tid; g < L.n_group; g += 256) {
        const int id = L.group_id[g], sl = sgx_covis_lookup(A, id);
        int rank = 0, same = 0;
        for (int m = 0; m < L.n_group; m++) { rank += L.group_id[m] < id; same += L.group_id[m] == id; }
        if (sl < 0 || same != 1) { bad = 1; continue; }
        L.gslot[g] = sl; L.grank[g] = rank; L.rowg[rank] = g; L.gof[sl] = g;
    }
    if (bad) sgx_atomic_or(&s_bad, 1);
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) L.s[LS_VALID] = !s_bad;
    SGX_THREADS_END
    SGX_SYNC();
}

// ------------------------------------------------------------------------------------------------------------------------------------------ CorrectLoop :546-564
// the group row checked; the queries of the UpdateConnections pass are the members in list order (none when the row is refused)
SGX_KERNEL(256) k_covis_lc_begin(SgxCovisArgs A, SgxCovisLoopArgs L)
{
    sgx_covis_loop_rows(A, L);
    const int ok = L.s[LS_VALID];
    SGX_THREADS_BEGIN(tid)
    for (int g = tid; g < L.n_group; g += 256) L.qkf[g] = ok ? L.group_id[g] : -1;
    if (tid == 0 && !ok) { SgxCovisLoopReport R = {}; R.status = -1; *L.report = R; }
    SGX_THREADS_END
}

// The members in list order by one workgroup: vpPreviousNeighbors = the member's list as its mode defines it NOW (an earlier member's AddConnection may have rebuilt
// it), UpdateConnections, and the marks of LoopConnections[member] = the keys of its row that are not in the previous list, not in the group and not isBad() (rule 11),
// left in the member's count row, with their number per rank.  A is the argument block of the UpdateConnections queries (row g = member g).
SGX_KERNEL(256) k_covis_lc_apply(SgxCovisArgs A, SgxCovisLoopArgs L)
{
    SGX_LDS unsigned char s_prev[SGX_COVIS_MAX_KF];
    SGX_LDS int s_c;
    if (!L.s[LS_VALID]) return;
    for (int g = 0; g < L.n_group; g++) {
        const int s = L.gslot[g];
        int *row = L.flags + (size_t)g * A.max_kf;
        SGX_THREADS_BEGIN(tid)
        for (int t = tid; t < A.nslots; t += 256) s_prev[t] = sgx_covis_listed(A, s, t);
        if (tid == 0) s_c = 0;
        SGX_THREADS_END
        SGX_SYNC();
        sgx_covis_apply_one(A, g);
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int t = tid; t < A.nslots; t += 256) {
            const int f = A.W[(size_t)s * A.max_kf + t] > 0 && !s_prev[t] && L.gof[t] < 0 && A.kf[t * CV_FIELDS + CV_STATE] == SGX_COVIS_LIVE;
            row[t] = f; c += f;
        }
        if (c) sgx_atomic_add(&s_c, c);
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) L.vcnt[L.grank[g]] = s_c;
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// The CSR over the members in ascending id with the targets of each in ascending id: a rank starts where the ranks before it end, and within a row every lane takes a
// stretch of the sorted table.  lc_begin is whole; a row is written only if it fits wholly.  The last rank leaves the total and the report.
SGX_KERNEL(256) k_covis_lc_emit(SgxCovisArgs A, SgxCovisLoopArgs L)
{
    SGX_LDS int s_part[256];
    SGX_LDS int s_base;
    if (!L.s[LS_VALID]) return;
    const int seg = (A.nlive + 255) / 256;
    for (int r = (int)blockIdx.x; r < L.n_group; r += (int)gridDim.x) {
        const int *row = L.flags + (size_t)L.rowg[r] * A.max_kf;
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int j = tid; j < r; j += 256) c += L.vcnt[j];
        s_part[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { int b = 0; for (int i = 0; i < 256; i++) b += s_part[i]; s_base = b; }
        SGX_THREADS_END
        SGX_SYNC();
        const int base = s_base, fits = base + L.vcnt[r] <= L.lcap;
        SGX_THREADS_BEGIN(tid)
        int c = 0;
        for (int j = tid * seg; j < A.nlive && j < (tid + 1) * seg; j++) c += row[A.sorted_slot[j]];
        s_part[tid] = c;
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            int o = base;
            for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; }
            L.lc_begin[r] = base;
            if (r == L.n_group - 1) {
                L.lc_begin[L.n_group] = o;
                SgxCovisLoopReport R = {}; R.status = o > L.lcap ? -3 : 0; R.n_group = L.n_group; R.n_connections = o; *L.report = R;
            }
        }
        SGX_THREADS_END
        SGX_SYNC();
        if (fits) {
            SGX_THREADS_BEGIN(tid)
            int o = s_part[tid];
            for (int j = tid * seg; j < A.nlive && j < (tid + 1) * seg; j++) if (row[A.sorted_slot[j]]) L.lc_j[o++] = A.sorted_id[j];
            SGX_THREADS_END
        }
        SGX_SYNC();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------ OptimizeEssentialGraph
// is keyframe y (slot sy) a loop connection of group member x that the loop of :852-880 keeps: (x == cur && y == loop) || x->GetWeight(y) >= minFeat, read from x's row
SGX_DEV bool sgx_covis_eg_kept(const SgxCovisArgs &A, const SgxCovisLoopArgs &L, int sx, int idx, int sy, int idy)
{
    const int g = L.gof[sx];
    if (g < 0) return false;
    const int r = L.grank[g], end = L.lc_begin[r + 1];
    int lo = L.lc_begin[r], hi = end;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (L.lc_j[mid] < idy) lo = mid + 1; else hi = mid; }
    if (lo >= end || L.lc_j[lo] != idy) return false;
    return (idx == L.cur && idy == L.loop) || A.W[(size_t)sx * A.max_kf + sy] >= SGX_COVIS_EG_MINFEAT;
}

// The inputs checked (the group row; the CSR: lc_begin from 0, ascending, within lcap, every row's targets live keyframes in strictly ascending id), the vertices, and
// the loop-connection edges in CSR order: every lane takes a stretch of the rows, counts what the test of :862 keeps, lane 0 scans, every lane writes its stretch.
SGX_KERNEL(256) k_covis_eg_begin(SgxCovisArgs A, SgxCovisLoopArgs L)
{
    SGX_LDS int s_part[256];
    SGX_LDS int s_bad;
    sgx_covis_loop_rows(A, L);
    const int seg = (L.n_group + 255) / 256;
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) s_bad = !L.s[LS_VALID] || L.lc_begin[0] != 0;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int bad = 0;
    for (int r = tid; r < L.n_group; r += 256) { const int a = L.lc_begin[r], b = L.lc_begin[r + 1]; if (a < 0 || b < a || b > L.lcap) bad = 1; }
    if (bad) sgx_atomic_or(&s_bad, 1);
    SGX_THREADS_END
    SGX_SYNC();
    const int shape_bad = s_bad;
    SGX_SYNC();                                                           // every lane has read it before any lane raises it again
    if (!shape_bad) {                                                     // the rows lie within lc_j now
        SGX_THREADS_BEGIN(tid)
        int bad = 0;
        for (int r = tid; r < L.n_group; r += 256)
            for (int e = L.lc_begin[r]; e < L.lc_begin[r + 1]; e++)
                if (sgx_covis_lookup(A, L.lc_j[e]) < 0 || (e > L.lc_begin[r] && L.lc_j[e - 1] >= L.lc_j[e])) bad = 1;
        if (bad) sgx_atomic_or(&s_bad, 1);
        SGX_THREADS_END
        SGX_SYNC();
    }
    if (s_bad) {                                                          // its status, and nothing else of it is written by any kernel
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) { SgxCovisLoopReport R = {}; R.status = -1; *L.report = R; L.s[LS_VALID] = 0; }
        SGX_THREADS_END
        return;
    }
    SGX_THREADS_BEGIN(tid)
    for (int j = tid; j < A.nlive; j += 256) {
        const int sl = A.sorted_slot[j], id = A.sorted_id[j];
        L.vidx[sl] = j; L.vertex_id[j] = id; L.vertex_fixed[j] = (unsigned char)(id == L.loop); L.vertex_group[j] = L.gof[sl];
    }
    int c = 0;
    for (int r = tid * seg; r < L.n_group && r < (tid + 1) * seg; r++) {
        const int si = L.gslot[L.rowg[r]], idi = A.kf[si * CV_FIELDS + CV_ID];
        for (int e = L.lc_begin[r]; e < L.lc_begin[r + 1]; e++) c += sgx_covis_eg_kept(A, L, si, idi, sgx_covis_lookup(A, L.lc_j[e]), L.lc_j[e]);
    }
    s_part[tid] = c;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        int o = 0;
        for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; }
        L.s[LS_E0] = o; L.s[LS_K1] = 0; L.s[LS_K2] = 0; L.s[LS_K3] = 0;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int o = s_part[tid];
    for (int r = tid * seg; r < L.n_group && r < (tid + 1) * seg; r++) {
        const int si = L.gslot[L.rowg[r]], idi = A.kf[si * CV_FIELDS + CV_ID];
        for (int e = L.lc_begin[r]; e < L.lc_begin[r + 1]; e++) {
            const int sj = sgx_covis_lookup(A, L.lc_j[e]);
            if (!sgx_covis_eg_kept(A, L, si, idi, sj, L.lc_j[e])) continue;
            if (o < L.ecap) { L.e_i[o] = L.vidx[si]; L.e_j[o] = L.vidx[sj]; L.e_kind[o] = 0; }
            o++;
        }
    }
    SGX_THREADS_END
}

// The normal edges of vertex v (:883-972), one workgroup per vertex, in two forms: counting (EMIT 0: vcnt and the totals per kind) and writing at vbase (EMIT 1).
//   the spanning-tree edge (also when the pair is in sInsertedEdges); the loop edges of smaller id in ascending id (lane 0: a keyframe closes few loops);
//   GetCovisiblesByWeight(minFeat) as written: the entries before the first list entry below minFeat, and NONE when no entry is below it; of those the ones that are not
//   the parent, a child, a loop edge, isBad(), of larger-or-equal id or a pair of sInsertedEdges, in list order = their rank by (weight, id) among themselves.
template <int EMIT> SGX_KERNEL(256) k_covis_eg_vertex(SgxCovisArgs A, SgxCovisLoopArgs L)
{
    SGX_LDS unsigned long long s_key[SGX_COVIS_MAX_KF];
    SGX_LDS int s_slot[SGX_COVIS_MAX_KF];
    SGX_LDS int s_n, s_weak, s_c12, s_c1, s_c2;
    if (!L.s[LS_VALID]) return;
    for (int v = (int)blockIdx.x; v < A.nlive; v += (int)gridDim.x) {
        const int s = A.sorted_slot[v], idv = A.sorted_id[v], parent = A.kf[s * CV_FIELDS + CV_PARENT];
        const int base = EMIT ? L.vbase[v] : 0;
        SGX_THREADS_BEGIN(tid)
        if (tid == 0) {
            s_n = 0; s_weak = 0;
            int o = base, c1 = 0, c2 = 0;
            if (parent >= 0) {
                if (EMIT && o < L.ecap) { L.e_i[o] = v; L.e_j[o] = L.vidx[parent]; L.e_kind[o] = 1; }
                o++; c1 = 1;
            }
            for (int last = -1;;) {                                       // mspLoopEdges in ascending id, those below this keyframe's
                int best = INT_MAX, bt = -1;
                for (int k = 0; k < L.n_le; k++) {
                    const int other = L.le[2 * k] == s ? L.le[2 * k + 1] : L.le[2 * k + 1] == s ? L.le[2 * k] : -1;
                    if (other < 0) continue;
                    const int id = A.kf[other * CV_FIELDS + CV_ID];
                    if (id < idv && id > last && id < best) { best = id; bt = other; }
                }
                if (bt < 0) break;
                if (EMIT && o < L.ecap) { L.e_i[o] = v; L.e_j[o] = L.vidx[bt]; L.e_kind[o] = 2; }
                o++; c2++; last = best;
            }
            s_c1 = c1; s_c2 = c2; s_c12 = c1 + c2;
        }
        SGX_THREADS_END
        SGX_SYNC();
        SGX_THREADS_BEGIN(tid)
        for (int t = tid; t < A.nslots; t += 256) {
            if (!sgx_covis_listed(A, s, t)) continue;
            const int w = A.W[(size_t)s * A.max_kf + t];
            if (w < SGX_COVIS_EG_MINFEAT) { s_weak = 1; continue; }
            const int idt = A.kf[t * CV_FIELDS + CV_ID];
            if (t == parent || A.kf[t * CV_FIELDS + CV_STATE] != SGX_COVIS_LIVE || A.kf[t * CV_FIELDS + CV_PARENT] == s || idt >= idv || sgx_covis_is_loop_edge(L, s, t) ||
                sgx_covis_eg_kept(A, L, s, idv, t, idt) || sgx_covis_eg_kept(A, L, t, idt, s, idv)) continue;
            const int pos = sgx_atomic_add(&s_n, 1);
            s_key[pos] = ((unsigned long long)w << 32) | (unsigned)idt; s_slot[pos] = t;
        }
        SGX_THREADS_END
        SGX_SYNC();
        const int n = s_weak ? s_n : 0;                                   // upper_bound found no entry below minFeat: the result is empty (KeyFrame.cc:193-194)
        SGX_THREADS_BEGIN(tid)
        if (EMIT) {
            for (int i = tid; i < n; i += 256) {
                const unsigned long long key = s_key[i];
                int rank = 0;
                for (int j = 0; j < n; j++) rank += s_key[j] > key;
                const int o = base + s_c12 + rank;
                if (o < L.ecap) { L.e_i[o] = v; L.e_j[o] = L.vidx[s_slot[i]]; L.e_kind[o] = 3; }
            }
        } else if (tid == 0) {
            L.vcnt[v] = s_c12 + n;
            if (s_c1) sgx_atomic_add(&L.s[LS_K1], s_c1);
            if (s_c2) sgx_atomic_add(&L.s[LS_K2], s_c2);
            if (n) sgx_atomic_add(&L.s[LS_K3], n);
        }
        SGX_THREADS_END
        SGX_SYNC();
    }
}

// vbase: where every vertex's edges start = the loop-connection edges and the vertices before it; the report with the true counts
SGX_KERNEL(256) k_covis_eg_scan(SgxCovisArgs A, SgxCovisLoopArgs L)
{
    SGX_LDS int s_part[256];
    if (!L.s[LS_VALID]) return;
    const int seg = (A.nlive + 255) / 256;
    SGX_THREADS_BEGIN(tid)
    int c = 0;
    for (int v = tid * seg; v < A.nlive && v < (tid + 1) * seg; v++) c += L.vcnt[v];
    s_part[tid] = c;
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    if (tid == 0) {
        int o = L.s[LS_E0];
        for (int i = 0; i < 256; i++) { const int c = s_part[i]; s_part[i] = o; o += c; }
        SgxCovisLoopReport R = {};
        R.status = o > L.ecap ? -3 : 0;                                   // SGX_ERR_NOMEM
        R.n_group = L.n_group; R.n_connections = L.lc_begin[L.n_group]; R.n_vertices = A.nlive; R.n_edges = o;
        R.n_kind[0] = L.s[LS_E0]; R.n_kind[1] = L.s[LS_K1]; R.n_kind[2] = L.s[LS_K2]; R.n_kind[3] = L.s[LS_K3];
        *L.report = R;
    }
    SGX_THREADS_END
    SGX_SYNC();
    SGX_THREADS_BEGIN(tid)
    int o = s_part[tid];
    for (int v = tid * seg; v < A.nlive && v < (tid + 1) * seg; v++) { const int c = L.vcnt[v]; L.vbase[v] = o; o += c; }
    SGX_THREADS_END
}
