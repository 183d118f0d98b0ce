// sgx_ba_plan.h — host-only planning of a bundle adjustment, before anything touches the device: the switches of one call (BaSwitches), the flattened problem's index
// structures (build_index) and the choice and layout of the reduced-camera-system solver (plan_solver).  Included by sgx_ba.cpp only, after sgx_ba_kernels.h (SgxBaEdge,
// SGX_NB, SGX_ENV_MAXM, SGX_BA_MAX_DENSE).
#pragma once
#include <limits.h>

// Every switch of the bundle adjustments and of the solver they share with the essential-graph optimisation, filled once at the top of a C entry (ba_switches(), sgx_ba.cpp)
// from the test taps of include/sgx_debug.h and the environment.  The product build has neither (sgx_rt.h): every member keeps its default there.
struct BaSwitches {
    int init_mode = 0;      // sgx_ba_debug_set_init: 0 = envelope solver: only its tiles are initialised, 1 = the whole matrix, 2 = the whole matrix NaN, then the tiles, 3 = 2 + every double / float scratch array of the arena NaN before the first kernel
    int jobs_host = 0;      // sgx_ba_debug_set_jobs: 1 = build the Schur job list on the host (the emulator's only path; A/B arm of the device builder)
    int solver = 0;         // sgx_ba_debug_set_solver, else SGX_BA_SOLVER = dense | env | auto: 0 auto, 1 dense blocked Cholesky, 2 envelope solver
    int twist = 1;          // SGX_BA_TWIST: 0 = never the two-branch ordering
    int timing = 0;         // SGX_BA_TIMING: wall-clock of the host phases on stderr
    int env_dbg = 0;        // SGX_ENV_DBG, timing tap of k_chol_env_factor: 1 skip the diagonal tiles, 2 skip panel + update, 4 skip the update
    int wide_min = 1024;    // SGX_TUNE_CHOL_WIDE_MIN: unknowns above which the dense factorisation works in outer panels (tools/campaign_ba_large.py)
};

// Index structures of a flattened problem: plain host data.
struct BaIndex {
    int np = 0, nl = 0, ne = 0, nf = 0, NP = 0;                // poses, landmarks, edges, free poses, unknowns of the reduced camera system (6 nf)
    std::vector<SgxBaEdge> E;
    std::vector<int> pt_start, pt_edges, pose_start, pose_edges;      // CSR by landmark and by pose, both in edge order
    std::vector<int> pose_edges_l;                             // the edges of a pose in ascending landmark order (ties: edge order) for the Schur job list
    std::vector<int> hidx, free_pose;                          // pose -> row of the reduced system (-1 fixed) and back
    std::vector<double> Xd;
    size_t jobs_cap = 0;                                       // upper bound of the Schur job list: sum over landmarks of (edges with a free pose)^2
    int row_of_edge(int k) const { return hidx[E[k].pose]; }
};

static int build_index(const sgx_ba_problem &P, BaIndex *out)
{
    BaIndex &ix = *out;
    ix.np = P.n_poses; ix.nl = P.n_points; ix.ne = P.n_edges;
    ix.hidx.resize(ix.np);
    for (int i = 0; i < ix.np; i++) { if (P.pose_fixed[i]) ix.hidx[i] = -1; else { ix.hidx[i] = (int)ix.free_pose.size(); ix.free_pose.push_back(i); } }
    ix.nf = (int)ix.free_pose.size(); ix.NP = 6 * ix.nf;
    if (ix.NP > SGX_BA_MAX_DENSE) return SGX_ERR_UNSUPPORTED;
    std::vector<SgxBaEdge> &E = ix.E;
    E.resize(ix.ne); ix.pt_start.assign(ix.nl + 1, 0); ix.pose_start.assign(ix.np + 1, 0); ix.pt_edges.resize(ix.ne); ix.pose_edges.resize(ix.ne);
    for (int k = 0; k < ix.ne; k++) {
        const int p = P.edge_pose[k], l = P.edge_point[k];
        if (p < 0 || p >= ix.np || l < 0 || l >= ix.nl) return SGX_ERR_INVALID;
        E[k].pose = p; E[k].point = l; E[k].flags = (P.edge_obs[3 * k + 2] < 0 ? 0 : 1) | 4;
        E[k].obs[0] = P.edge_obs[3 * k]; E[k].obs[1] = P.edge_obs[3 * k + 1]; E[k].obs[2] = P.edge_obs[3 * k + 2]; E[k].info = P.edge_info[k];
        ix.pt_start[l + 1]++; ix.pose_start[p + 1]++;
    }
    for (int l = 0; l < ix.nl; l++) ix.pt_start[l + 1] += ix.pt_start[l];
    for (int p = 0; p < ix.np; p++) ix.pose_start[p + 1] += ix.pose_start[p];
    { std::vector<int> f1(ix.nl, 0), f2(ix.np, 0);
      for (int k = 0; k < ix.ne; k++) { ix.pt_edges[ix.pt_start[E[k].point] + f1[E[k].point]++] = k; ix.pose_edges[ix.pose_start[E[k].pose] + f2[E[k].pose]++] = k; } }
    for (int l = 0; l < ix.nl; l++) { size_t c = 0; for (int q = ix.pt_start[l]; q < ix.pt_start[l + 1]; q++) if (ix.row_of_edge(ix.pt_edges[q]) >= 0) c++; ix.jobs_cap += c * c; }
    if (ix.jobs_cap > (size_t)INT_MAX) return SGX_ERR_UNSUPPORTED;      // the list's offsets and totals are int, on the host and in k_ba_jobs_scan: refused before anything is allocated
    ix.pose_edges_l = ix.pose_edges;
    for (int p = 0; p < ix.np; p++) {      // (a caller that adds its edges landmark by landmark — Optimizer.cc:573-640 does — hands every pose its edges already in this order)
        const auto lt = [&](int x, int y) { return E[x].point != E[y].point ? E[x].point < E[y].point : x < y; };
        const auto b = ix.pose_edges_l.begin() + ix.pose_start[p], e = ix.pose_edges_l.begin() + ix.pose_start[p + 1];
        if (!std::is_sorted(b, e, lt)) std::sort(b, e, lt);
    }
    ix.Xd.resize(3 * (size_t)ix.nl);
    for (size_t i = 0; i < ix.Xd.size(); i++) ix.Xd[i] = (double)P.points[i];
    return SGX_OK;
}

// Solver of the reduced camera system.  Free poses i1, i2 are coupled when they share a landmark.  With the free poses in keyframe order (hidx) the tile rows of the system are
// non-zero from a first tile column on and fill stays inside that envelope; when it is narrow the solver walks it with one persistent workgroup (k_chol_env_factor)
// instead of the dense blocked factorisation.  Rows of column step k = rows[rstart[k] .. rstart[k+1]).  Two-branch elimination: column steps [0, nA) and [nA, nA + nB) are
// independent, the remaining nsep unknowns are their separator (nB = 0: one branch).  Empty = the dense solver.
struct EnvPlan {
    std::vector<int> rstart, rows; int nA = 0, nB = 0; size_t nsep = 0;
    bool empty() const { return rstart.empty(); }
    int nrows() const { return empty() ? 0 : rstart.back(); }
    // the four integers of sgx_ba_debug_last_plan: envelope solver?, column steps of the first branch (all of them when there is one branch), of the second, separator unknowns
    void describe(int NP, int plan[4]) const { plan[0] = empty() ? 0 : 1; plan[1] = nB > 0 ? nA : (empty() ? 0 : (NP + SGX_NB - 1) / SGX_NB); plan[2] = nB; plan[3] = (int)nsep; }
};

// Plan for an ordering pos[natural free-pose index] -> position: tile pattern of the reduced system from the landmarks' pose sets, symbolic tile Cholesky (the structure of
// column k is R(k); every pair of R(k) becomes a tile of the factor), narrowness test.  Returns false when a step has too many rows or, unless forced, the envelope is wide.
static bool plan_envelope(const BaIndex &ix, const std::vector<int> &pos, bool force_env, EnvPlan *plan)
{
    const int nt = (ix.NP + SGX_NB - 1) / SGX_NB;
    std::vector<int> &rstart = plan->rstart, &rws = plan->rows;
    std::vector<uint8_t> pat((size_t)nt * nt, 0);
    std::vector<int> tl;
    for (int l = 0; l < ix.nl; l++) {
        tl.clear();
        for (int q = ix.pt_start[l]; q < ix.pt_start[l + 1]; q++) {
            const int h = ix.row_of_edge(ix.pt_edges[q]); if (h < 0) continue;
            const int u0 = 6 * pos[h], t0 = u0 / SGX_NB, t1 = (u0 + 5) / SGX_NB;
            tl.push_back(t0); if (t1 != t0) tl.push_back(t1);
        }
        std::sort(tl.begin(), tl.end()); tl.erase(std::unique(tl.begin(), tl.end()), tl.end());      // a landmark's poses sit on a few tiles
        for (size_t a = 0; a < tl.size(); a++) for (size_t b = 0; b < a; b++) pat[(size_t)tl[a] * nt + tl[b]] = 1;
    }
    // a pose that straddles two tiles couples them even without a landmark
    for (int h = 0; h < ix.nf; h++) { const int u0 = 6 * h, t0 = u0 / SGX_NB, t1 = (u0 + 5) / SGX_NB; if (t1 != t0) pat[(size_t)t1 * nt + t0] = 1; }
    rstart.assign(nt + 1, 0); rws.clear();
    std::vector<int> R;
    size_t total = 0;
    for (int k = 0; k < nt; k++) {
        R.clear();
        for (int r = k + 1; r < nt; r++) if (pat[(size_t)r * nt + k]) R.push_back(r);
        if ((int)R.size() > SGX_ENV_MAXM) return false;
        for (size_t a = 0; a < R.size(); a++) for (size_t b = 0; b < a; b++) pat[(size_t)R[a] * nt + R[b]] = 1;
        rws.insert(rws.end(), R.begin(), R.end());                                 // rows ascending inside a step
        rstart[k + 1] = (int)rws.size(); total += R.size();
    }
    if (rws.empty()) rws.push_back(0);
    // narrow = a step's tile products fit a few rounds of the persistent workgroup's waves; otherwise the dense two-level path (matrix cores) wins
    return force_env || total <= (size_t)nt * 10;
}

// Chooses the solver and, for the two-branch ordering, renumbers the free poses (ix.free_pose / ix.hidx): the order of the unknowns IS the order of the free poses.
static EnvPlan plan_solver(BaIndex &ix, const BaSwitches &sw)
{
    EnvPlan plan;
    const bool want_env = sw.solver != 1, force_env = sw.solver == 2;
    const int nf = ix.nf, nt = (ix.NP + SGX_NB - 1) / SGX_NB;
    if (!want_env || ix.NP <= (force_env ? 0 : 1024)) return plan;
    // Two-branch ordering: [poses 0 .. a) ascending][poses t0-1 .. bs DEScending][separator: the rest, natural order]: the band is eliminated from both ends at once.
    // The separator must cut every coupling between the halves (no pose of [bs, t0) shares a landmark with a pose < a): it is the stretch [a, bs) behind the first
    // half plus — when the trajectory closes on itself — the tail [t0, nf) that sees the start again.  Branch sizes are multiples of 16 poses = 3 tiles.
    if (sw.twist && nt >= 24) {
        // the lowest pose each pose is coupled with (natural order = keyframe order)
        std::vector<int> fblk(nf);
        for (int i = 0; i < nf; i++) fblk[i] = i;
        for (int l = 0; l < ix.nl; l++) {
            int lo = nf;
            for (int q = ix.pt_start[l]; q < ix.pt_start[l + 1]; q++) { const int h = ix.row_of_edge(ix.pt_edges[q]); if (h >= 0 && h < lo) lo = h; }
            for (int q = ix.pt_start[l]; q < ix.pt_start[l + 1]; q++) { const int h = ix.row_of_edge(ix.pt_edges[q]); if (h >= 0 && lo < fblk[h]) fblk[h] = lo; }
        }
        const int a = (nf / 2 / 16) * 16;
        int bs = a; while (bs < nf && fblk[bs] < a) bs++;                     // behind the first half: coupled with it
        int t0 = bs; while (t0 < nf && fblk[t0] >= a) t0++;                   // the independent stretch ends where the start is seen again
        const int nb_poses = ((t0 - bs) / 16) * 16; bs = t0 - nb_poses;
        if (a >= 16 && nb_poses >= 16) {
            std::vector<int> pos(nf);
            int sp = a + nb_poses;
            for (int h = 0; h < nf; h++) pos[h] = h < a ? h : ((h >= bs && h < t0) ? a + (t0 - 1 - h) : sp++);
            const int tA = 6 * a / SGX_NB, tB = 6 * nb_poses / SGX_NB;
            bool ok = plan_envelope(ix, pos, force_env, &plan);
            // the two branches must not touch each other's tiles: no row of the second branch in a column step of the first (they run concurrently)
            for (int k = 0; ok && k < tA; k++) for (int q = plan.rstart[k]; q < plan.rstart[k + 1]; q++) if (plan.rows[q] >= tA && plan.rows[q] < tA + tB) { ok = false; break; }
            if (ok) {
                plan.nA = tA; plan.nB = tB; plan.nsep = (size_t)ix.NP - (size_t)(tA + tB) * SGX_NB;
                std::vector<int> fp2(nf);
                for (int h = 0; h < nf; h++) fp2[pos[h]] = ix.free_pose[h];
                ix.free_pose.swap(fp2);
                for (int h = 0; h < nf; h++) ix.hidx[ix.free_pose[h]] = h;
                return plan;
            }
        }
    }
    std::vector<int> pos(nf); for (int h = 0; h < nf; h++) pos[h] = h;
    if (!plan_envelope(ix, pos, force_env, &plan)) plan = EnvPlan();
    return plan;
}
