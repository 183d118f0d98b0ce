"""numpy float64 restatement of PnPsolver (src/sg-slam/src/PnPsolver.cc) and the OpenCV 3.4 algebra it calls (tests only): JacobiSVDImpl_<double>, SVBkSb (cvSolve /
cvInvert with CV_SVD) and MulTransposedR (cvMulTransposed), written from their published algorithm; the Jacobi rotation's std::hypot is the kernel's
sgx_pnp_hypot (max * sqrt(1 + (min / max)^2)), so that the device agrees too.  Every expression is evaluated in the order the C code writes it,
sums are sequential (np.cumsum with a leading +0), and the loops of the Jacobi sweep run in the kernel's order, so the results are the kernel-logic emulator's bits.
Arrays carry a leading batch axis H (hypotheses), vectorised; lanes of a batch that the C code would leave alone are masked.  Defined behaviour where the reference's is
undefined (sg_slam_amd/csrc/sgx_pnp_kernels.h): a Gauss-Newton step whose qr_solve meets a singular A makes no update; division by a zero beta is IEEE."""
import math
import numpy as np

DBL_EPSILON = np.finfo(np.float64).eps
DBL_MIN = np.finfo(np.float64).tiny


def seqsum(x, axis=-1):
    """0.0 + x[0] + x[1] + ... in order along axis"""
    x = np.moveaxis(np.asarray(x, 'f8'), axis, -1)
    z = np.zeros(x.shape[:-1] + (1,))
    return np.cumsum(np.concatenate([z, x], -1), -1)[..., -1]


def hypot(x, y):
    """sgx_pnp_hypot: max * sqrt(1 + (min / max)^2), correctly rounded operations only (the kernel's replacement for std::hypot)"""
    a = np.abs(x); b = np.abs(y)
    sw = a < b
    a, b = np.where(sw, b, a), np.where(sw, a, b)
    with np.errstate(all='ignore'):
        r = b / a
        h = a * np.sqrt(1.0 + r * r)
    return np.where((a == 0) | (b == 0), a + b, h)


def jacobi(At, m, n):
    """JacobiSVDImpl_<double>(At, W, Vt, m, n, n, DBL_MIN, DBL_EPSILON * 10) on a batch: At (H, n, m) -> (U^T rows, W descending, Vt)"""
    At = np.array(At, 'f8'); H = At.shape[0]
    eps = DBL_EPSILON * 10
    W = seqsum(At * At, -1)
    Vt = np.broadcast_to(np.eye(n), (H, n, n)).copy()
    active = np.ones(H, bool)
    with np.errstate(all='ignore'):
        for _ in range(max(m, 30)):
            changed = np.zeros(H, bool)
            for i in range(n - 1):
                for j in range(i + 1, n):
                    Ai = At[:, i, :].copy(); Aj = At[:, j, :].copy()
                    a = W[:, i].copy(); b = W[:, j].copy()
                    p = seqsum(Ai * Aj, -1)
                    rot = active & ~(np.abs(p) <= eps * np.sqrt(a * b))
                    if not rot.any(): continue
                    p = p * 2
                    beta = a - b; gamma = hypot(p, beta)
                    neg = beta < 0
                    delta = (gamma - beta) * 0.5
                    s_n = np.sqrt(delta / gamma); c_n = p / (gamma * s_n * 2)
                    c_p = np.sqrt((gamma + beta) / (gamma * 2)); s_p = p / (gamma * c_p * 2)
                    c = np.where(neg, c_n, c_p)[:, None]; s = np.where(neg, s_n, s_p)[:, None]
                    t0 = c * Ai + s * Aj; t1 = (-s) * Ai + c * Aj
                    r = rot[:, None]
                    At[:, i, :] = np.where(r, t0, Ai); At[:, j, :] = np.where(r, t1, Aj)
                    W[:, i] = np.where(rot, seqsum(t0 * t0, -1), a); W[:, j] = np.where(rot, seqsum(t1 * t1, -1), b)
                    Vi = Vt[:, i, :].copy(); Vj = Vt[:, j, :].copy()
                    Vt[:, i, :] = np.where(r, c * Vi + s * Vj, Vi); Vt[:, j, :] = np.where(r, (-s) * Vi + c * Vj, Vj)
                    changed |= rot
            active = changed
            if not changed.any(): break
        W = np.sqrt(seqsum(At * At, -1))
        ar = np.arange(H)
        for i in range(n - 1):
            j = np.full(H, i)
            for k in range(i + 1, n):
                j = np.where(W[ar, j] < W[:, k], k, j)
            sw = j != i
            if sw.any():
                h = ar[sw]; jj = j[sw]
                W[h, i], W[h, jj] = W[h, jj].copy(), W[h, i].copy()
                At[h, i, :], At[h, jj, :] = At[h, jj, :].copy(), At[h, i, :].copy()
                Vt[h, i, :], Vt[h, jj, :] = Vt[h, jj, :].copy(), Vt[h, i, :].copy()
        need = (W <= DBL_MIN).any(1)
        for h in np.nonzero(need)[0]: _complete(At[h], W[h], m, n)
        ok = ~need
        At[ok] = At[ok] * np.where(W[ok] > DBL_MIN, 1 / W[ok], 0.)[:, :, None]          # s = sd > minval ? 1 / sd : 0 (a NaN row becomes 0 * NaN)
    return At, W, Vt


def _complete(At, W, m, n):
    """the completion of zero singular values and the normalisation of one matrix (scalar, in place)"""
    eps = DBL_EPSILON * 10; rng = 0x12345678; M64 = (1 << 64) - 1
    for i in range(n):
        sd = float(W[i]); ii = 0
        while ii < 100 and sd <= DBL_MIN:
            val0 = 1. / m
            for k in range(m):
                rng = ((rng & 0xffffffff) * 4164903690 + (rng >> 32)) & M64
                At[i, k] = val0 if (rng & 0xffffffff) & 256 else -val0
            for _ in range(2):
                for j in range(i):
                    sd = 0.0
                    for k in range(m): sd += float(At[i, k]) * float(At[j, k])
                    asum = 0.0
                    for k in range(m):
                        t = float(At[i, k]) - sd * float(At[j, k]); At[i, k] = t; asum += abs(t)
                    asum = 1 / asum if asum > eps * 100 else 0.0
                    for k in range(m): At[i, k] = float(At[i, k]) * asum
            sd = 0.0
            for k in range(m): t = float(At[i, k]); sd += t * t
            sd = float(np.sqrt(sd)); ii += 1
        s = 1 / sd if sd > DBL_MIN else 0.
        for k in range(m): At[i, k] = float(At[i, k]) * s


def svd(A):
    """cv::SVD::compute(A (H, m, n), m >= n): (U (H, m, n), W, Vt) — U's columns are the rotated rows of A^T"""
    A = np.asarray(A, 'f8'); m, n = A.shape[1:]
    At, W, Vt = jacobi(np.swapaxes(A, 1, 2), m, n)
    return np.swapaxes(At, 1, 2), W, Vt


def solve_svd(A, b):
    """cvSolve(A (H, m, n), b (H, m), x, CV_SVD)"""
    A = np.asarray(A, 'f8'); m, n = A.shape[1:]
    At, W, Vt = jacobi(np.swapaxes(A, 1, 2), m, n)
    threshold = seqsum(W, -1) * (DBL_EPSILON * 2)
    x = np.zeros((A.shape[0], n))
    with np.errstate(all='ignore'):
        for i in range(n):
            wi = W[:, i]; skip = np.abs(wi) <= threshold; wi = 1 / wi
            s = seqsum(At[:, i, :] * b, -1) * wi
            x = np.where(skip[:, None], x, x + s[:, None] * Vt[:, i, :])
    return x


def invert_svd(A):
    """cvInvert(A (H, n, n), X, CV_SVD)"""
    A = np.asarray(A, 'f8'); n = A.shape[1]
    At, W, Vt = jacobi(np.swapaxes(A, 1, 2), n, n)
    threshold = seqsum(W, -1) * (DBL_EPSILON * 2)
    X = np.zeros_like(A)
    with np.errstate(all='ignore'):
        for i in range(n):
            wi = W[:, i]; skip = np.abs(wi) <= threshold; wi = 1 / wi
            buf = At[:, i, :] * wi[:, None]
            X = np.where(skip[:, None, None], X, X + Vt[:, i, :, None] * buf[:, None, :])
    return X


def mul_transposed(M):
    """cvMulTransposed(M (H, r, c), D, 1) = M^T M, every entry one sequential sum over the rows"""
    M = np.asarray(M, 'f8')
    return seqsum(M[:, :, :, None] * M[:, :, None, :], 1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _qr_solve(A, b):
    """qr_solve (:860-950) on a batch of 6 x 4 systems: (X, ok); ok = False where A is singular (X not written in the reference)"""
    A = A.copy(); b = b.copy(); H = A.shape[0]
    ok = np.ones(H, bool); A1 = np.zeros((H, 4)); A2 = np.zeros((H, 4)); X = np.zeros((H, 4))
    for k in range(4):
        eta = np.abs(A[:, k, k])
        for i in range(k + 1, 6):
            elt = np.abs(A[:, i - 1, k]); eta = np.where(eta < elt, elt, eta)       # the reference reads the row before it advances (:880-885): rows k .. nr - 2
        ok &= ~(eta == 0)
        inv_eta = 1. / eta; s = np.zeros(H)
        for i in range(k, 6):
            A[:, i, k] = A[:, i, k] * inv_eta; s = s + A[:, i, k] * A[:, i, k]
        sigma = np.sqrt(s); sigma = np.where(A[:, k, k] < 0, -sigma, sigma)
        A[:, k, k] = A[:, k, k] + sigma
        A1[:, k] = sigma * A[:, k, k]; A2[:, k] = (-eta) * sigma
        for j in range(k + 1, 4):
            s = np.zeros(H)
            for i in range(k, 6): s = s + A[:, i, k] * A[:, i, j]
            tau = s / A1[:, k]
            for i in range(k, 6): A[:, i, j] = A[:, i, j] - tau * A[:, i, k]
    for j in range(4):
        tau = np.zeros(H)
        for i in range(j, 6): tau = tau + A[:, i, j] * b[:, i]
        tau = tau / A1[:, j]
        for i in range(j, 6): b[:, i] = b[:, i] - tau * A[:, i, j]
    X[:, 3] = b[:, 3] / A2[:, 3]
    for i in range(2, -1, -1):
        s = np.zeros(H)
        for j in range(i + 1, 4): s = s + A[:, i, j] * X[:, j]
        X[:, i] = (b[:, i] - s) / A2[:, i]
    return X, ok


def gauss_newton(L, rho, betas):
    with np.errstate(all='ignore'):
        return _gauss_newton(L, rho, betas)


def _gauss_newton(L, rho, betas):
    betas = betas.copy()
    for _ in range(5):
        A = np.zeros((L.shape[0], 6, 4)); b = np.zeros((L.shape[0], 6))
        B0, B1, B2, B3 = (betas[:, i] for i in range(4))
        for i in range(6):
            r = [L[:, i, c] for c in range(10)]
            A[:, i, 0] = 2 * r[0] * B0 + r[1] * B1 + r[3] * B2 + r[6] * B3
            A[:, i, 1] = r[1] * B0 + 2 * r[2] * B1 + r[4] * B2 + r[7] * B3
            A[:, i, 2] = r[3] * B0 + r[4] * B1 + 2 * r[5] * B2 + r[8] * B3
            A[:, i, 3] = r[6] * B0 + r[7] * B1 + r[8] * B2 + 2 * r[9] * B3
            b[:, i] = rho[:, i] - (r[0] * B0 * B0 + r[1] * B0 * B1 + r[2] * B1 * B1 + r[3] * B0 * B2 + r[4] * B1 * B2 + r[5] * B2 * B2 + r[6] * B0 * B3 +
                                   r[7] * B1 * B3 + r[8] * B2 * B3 + r[9] * B3 * B3)
        x, ok = _qr_solve(A, b)
        betas = np.where(ok[:, None], betas + x, betas)
    return betas


def find_betas(L, rho, which):
    cols = {1: [0, 1, 3, 6], 2: [0, 1, 2], 3: [0, 1, 2, 3, 4]}[which]
    b = solve_svd(L[:, :, cols], rho)
    betas = np.zeros((L.shape[0], 4))
    if which == 1:
        neg = b[:, 0] < 0
        b0 = np.where(neg, np.sqrt(np.where(neg, -b[:, 0], 0)), np.sqrt(np.where(neg, 0, b[:, 0])))
        betas[:, 0] = b0
        for i in (1, 2, 3): betas[:, i] = np.where(neg, (-b[:, i]) / b0, b[:, i] / b0)
        return betas
    neg = b[:, 0] < 0
    b0 = np.where(neg, np.sqrt(np.where(neg, -b[:, 0], 0)), np.sqrt(np.where(neg, 0, b[:, 0])))
    b1 = np.where(neg, np.where(b[:, 2] < 0, np.sqrt(np.where(b[:, 2] < 0, -b[:, 2], 0)), 0.0), np.where(b[:, 2] > 0, np.sqrt(np.where(b[:, 2] > 0, b[:, 2], 0)), 0.0))
    b0 = np.where(b[:, 1] < 0, -b0, b0)
    betas[:, 0] = b0; betas[:, 1] = b1
    betas[:, 2] = 0.0 if which == 2 else b[:, 3] / b0
    return betas


def compute_R_and_t(pws, us, alphas, ut, betas, cam):
    fu, fv, uc, vc = cam; n = pws.shape[1]
    ccs = np.zeros((pws.shape[0], 4, 3))
    for i in range(4): ccs = ccs + betas[:, i, None, None] * ut[:, 11 - i, :].reshape(-1, 4, 3)
    a = alphas
    pcs = a[:, :, 0, None] * ccs[:, None, 0, :] + a[:, :, 1, None] * ccs[:, None, 1, :] + a[:, :, 2, None] * ccs[:, None, 2, :] + a[:, :, 3, None] * ccs[:, None, 3, :]
    pcs = np.where((pcs[:, 0, 2] < 0.0)[:, None, None], -pcs, pcs)
    pc0 = seqsum(pcs, 1) / n; pw0 = seqsum(pws, 1) / n
    abt = seqsum((pcs - pc0[:, None, :])[:, :, :, None] * (pws - pw0[:, None, :])[:, :, None, :], 1)       # abt[j][c]
    At, W, Vt = jacobi(np.swapaxes(abt, 1, 2), 3, 3)
    R = np.zeros((pws.shape[0], 3, 3))
    for i in range(3):
        for j in range(3): R[:, i, j] = At[:, 0, i] * Vt[:, 0, j] + At[:, 1, i] * Vt[:, 1, j] + At[:, 2, i] * Vt[:, 2, j]
    det = (R[:, 0, 0] * R[:, 1, 1] * R[:, 2, 2] + R[:, 0, 1] * R[:, 1, 2] * R[:, 2, 0] + R[:, 0, 2] * R[:, 1, 0] * R[:, 2, 1] - R[:, 0, 2] * R[:, 1, 1] * R[:, 2, 0] -
           R[:, 0, 1] * R[:, 1, 0] * R[:, 2, 2] - R[:, 0, 0] * R[:, 1, 2] * R[:, 2, 1])
    R[:, 2, :] = np.where((det < 0)[:, None], -R[:, 2, :], R[:, 2, :])
    t = pc0 - _dot(R, pw0[:, None, :])
    with np.errstate(all='ignore'):
        Xc = _dot(R[:, None, 0, :], pws) + t[:, 0, None]; Yc = _dot(R[:, None, 1, :], pws) + t[:, 1, None]
        inv_Zc = 1.0 / (_dot(R[:, None, 2, :], pws) + t[:, 2, None])
        ue = uc + fu * Xc * inv_Zc; ve = vc + fv * Yc * inv_Zc
        u = us[:, :, 0]; v = us[:, :, 1]
        err = seqsum(np.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve)), 1) / n
    return R, t, err


def epnp(pws, us, cam):
    """compute_pose (:477-525) on a batch: pws (H, n, 3), us (H, n, 2) float64, cam = (fu, fv, uc, vc) float64 -> R (H, 3, 3), t (H, 3)"""
    pws = np.asarray(pws, 'f8'); us = np.asarray(us, 'f8'); H, n = pws.shape[:2]
    fu, fv, uc, vc = cam
    with np.errstate(all='ignore'):
        c0 = seqsum(pws, 1) / n
        d = pws - c0[:, None, :]
        pp = seqsum(d[:, :, :, None] * d[:, :, None, :], 1)
        uct, dc, _ = jacobi(pp, 3, 3)
        cws = np.zeros((H, 4, 3)); cws[:, 0] = c0
        for i in range(1, 4): cws[:, i] = c0 + np.sqrt(dc[:, i - 1] / n)[:, None] * uct[:, i - 1, :]
        cc = np.swapaxes(cws[:, 1:, :] - cws[:, None, 0, :], 1, 2)           # cc[i][j - 1] = cws[j][i] - cws[0][i]
        ci = invert_svd(cc)
        dp = pws - cws[:, None, 0, :]
        alphas = np.zeros((H, n, 4))
        for j in range(3): alphas[:, :, 1 + j] = ci[:, j, None, 0] * dp[:, :, 0] + ci[:, j, None, 1] * dp[:, :, 1] + ci[:, j, None, 2] * dp[:, :, 2]
        alphas[:, :, 0] = 1.0 - alphas[:, :, 1] - alphas[:, :, 2] - alphas[:, :, 3]
        M = np.zeros((H, n, 2, 12))
        for i in range(4):
            M[:, :, 0, 3 * i] = alphas[:, :, i] * fu; M[:, :, 0, 3 * i + 2] = alphas[:, :, i] * (uc - us[:, :, 0])
            M[:, :, 1, 3 * i + 1] = alphas[:, :, i] * fv; M[:, :, 1, 3 * i + 2] = alphas[:, :, i] * (vc - us[:, :, 1])
        mtm = mul_transposed(M.reshape(H, 2 * n, 12))
        ut, _, _ = jacobi(mtm, 12, 12)
        v = [ut[:, 11 - i, :].reshape(H, 4, 3) for i in range(4)]
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        dv = [np.stack([v[i][:, a, :] - v[i][:, b, :] for a, b in pairs], 1) for i in range(4)]      # (H, 6, 3)
        L = np.zeros((H, 6, 10))
        L[:, :, 0] = _dot(dv[0], dv[0]); L[:, :, 1] = 2.0 * _dot(dv[0], dv[1]); L[:, :, 2] = _dot(dv[1], dv[1]); L[:, :, 3] = 2.0 * _dot(dv[0], dv[2])
        L[:, :, 4] = 2.0 * _dot(dv[1], dv[2]); L[:, :, 5] = _dot(dv[2], dv[2]); L[:, :, 6] = 2.0 * _dot(dv[0], dv[3]); L[:, :, 7] = 2.0 * _dot(dv[1], dv[3])
        L[:, :, 8] = 2.0 * _dot(dv[2], dv[3]); L[:, :, 9] = _dot(dv[3], dv[3])
        dist2 = lambda p, q: (p[:, 0] - q[:, 0]) * (p[:, 0] - q[:, 0]) + (p[:, 1] - q[:, 1]) * (p[:, 1] - q[:, 1]) + (p[:, 2] - q[:, 2]) * (p[:, 2] - q[:, 2])
        rho = np.stack([dist2(cws[:, a], cws[:, b]) for a, b in pairs], 1)
        best = None
        for which in (1, 2, 3):
            betas = gauss_newton(L, rho, find_betas(L, rho, which))
            R, t, err = compute_R_and_t(pws, us, alphas, ut, betas, cam)
            if best is None: best = (R, t, err)
            else:
                w = err < best[2]
                best = (np.where(w[:, None, None], R, best[0]), np.where(w[:, None], t, best[1]), np.where(w, err, best[2]))
    return best[0], best[1]


def check_inliers(R, t, p3dw, p2d, cam, max_err):
    """CheckInliers (:308-340): R (H, 3, 3), t (H, 3) float64 against all N correspondences -> (H, N) bool"""
    fu, fv, uc, vc = cam
    P = p3dw.astype('f8'); x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all='ignore'):
        Xc = (R[:, 0, 0, None] * x + R[:, 0, 1, None] * y + R[:, 0, 2, None] * z + t[:, 0, None]).astype('f4')
        Yc = (R[:, 1, 0, None] * x + R[:, 1, 1, None] * y + R[:, 1, 2, None] * z + t[:, 1, None]).astype('f4')
        invZc = (1 / (R[:, 2, 0, None] * x + R[:, 2, 1, None] * y + R[:, 2, 2, None] * z + t[:, 2, None])).astype('f4')
        ue = uc + fu * Xc.astype('f8') * invZc.astype('f8'); ve = vc + fv * Yc.astype('f8') * invZc.astype('f8')
        dx = (p2d[:, 0].astype('f8') - ue).astype('f4'); dy = (p2d[:, 1].astype('f8') - ve).astype('f4')
        e2 = dx * dx + dy * dy
    return e2 < max_err


def tcw_of(R, t):
    T = np.eye(4, dtype='f4'); T[:3, :3] = R.astype('f4'); T[:3, 3] = t.astype('f4')
    return T


def ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon):
    """SetRansacParameters (:121-157) -> (mRansacMinInliers, mRansacMaxIts)"""
    eps = np.float32(epsilon)
    nMin = int(np.float32(N) * eps)
    nMin = max(nMin, minInliers, minSet)
    with np.errstate(all='ignore'):
        q = np.float32(nMin) / np.float32(N)
        if eps < q: eps = q
        if nMin == N: nIt = 1
        else:
            clog = lambda x: math.log(x) if x > 0 else (-math.inf if x == 0 else math.nan)         # libm log / pow, as the C code calls them
            v = np.ceil(np.float64(clog(1 - probability)) / np.float64(clog(1 - math.pow(float(eps), 3.0))))
            nIt = int(v) if (v == v and -2147483648.0 <= v < 2147483648.0) else -2147483648
    return nMin, max(1, min(nIt, maxIterations))


def draw_indices(N, draws):
    """four RandomInt(0, size - 1) with the swap-and-pop of vAvailableIndices (:191-201) per hypothesis: draws (H, 4) raw rand() values -> (H, 4) indices"""
    out = np.zeros((len(draws), 4), 'i8')
    for h, d in enumerate(draws):
        avail = {}
        for k in range(4):
            size = N - k
            r = int((float(d[k]) / (2147483647.0 + 1.0)) * size)
            out[h, k] = avail.get(r, r)
            avail[r] = avail.get(size - 1, size - 1)
    return out


class PnPsolverRef:
    """the reference class on host arrays: p2d (N, 2), sigma2 (N), p3dw (N, 3) float32, cam = fx, fy, cx, cy (float32)"""

    def __init__(self, p2d, sigma2, p3dw, cam):
        self.p2d = np.asarray(p2d, 'f4').reshape(-1, 2); self.sigma2 = np.asarray(sigma2, 'f4').reshape(-1); self.p3dw = np.asarray(p3dw, 'f4').reshape(-1, 3)
        self.N = len(self.p2d); self.cam = tuple(float(np.float32(c)) for c in cam)
        self.its = 0; self.best = 0; self.best_mask = np.zeros(self.N, bool); self.best_tcw = np.zeros((4, 4), 'f4')
        self.refines = 0; self.refines_on_other_set = 0; self._memo = {}
        self.set_ransac_parameters(0.99, 8, 300, 4, 0.4, 5.991)

    def set_ransac_parameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        assert minSet == 4
        self.min_inliers, self.max_its = ransac_parameters(self.N, probability, minInliers, maxIterations, minSet, epsilon)
        self.max_err = self.sigma2 * np.float32(th2); self.th2 = np.float32(th2)

    def call_hypotheses(self, n):
        return 0 if self.N < self.min_inliers else max(0, n, self.max_its - self.its)

    def refine(self):
        """Refine (:260-306) on the best-so-far inliers: (ok, Tcw, mask, n)"""
        key = (self.best_mask.tobytes(), self.min_inliers, float(self.th2))       # Refine's outcome depends on the set, minInliers and th2
        if key not in self._memo:
            self.refines += 1
            idx = np.nonzero(self.best_mask)[0]
            R, t = epnp(self.p3dw[idx][None].astype('f8'), self.p2d[idx][None].astype('f8'), self.cam)
            m = check_inliers(R, t, self.p3dw, self.p2d, self.cam, self.max_err)[0]
            self._memo[key] = (int(m.sum()) > self.min_inliers, tcw_of(R[0], t[0]), m, int(m.sum()))
        return self._memo[key]

    def iterate(self, n_iterations, draws):
        """(Tcw or None, bNoMore, inliers, nInliers, iterations_run)"""
        none = np.zeros(self.N, bool)
        if self.N < self.min_inliers: return None, True, none, 0, 0
        total = self.call_hypotheses(n_iterations)
        run = total; res = None
        if total:
            d = np.asarray(draws, 'i8')[:4 * total].reshape(total, 4)
            idx = draw_indices(self.N, d)
            R, t = epnp(self.p3dw[idx].astype('f8'), self.p2d[idx].astype('f8'), self.cam)
            masks = check_inliers(R, t, self.p3dw, self.p2d, self.cam, self.max_err)
            counts = masks.sum(1)
            for h in range(total):
                if counts[h] >= self.min_inliers:
                    if counts[h] > self.best:
                        self.best_mask = masks[h].copy(); self.best = int(counts[h]); self.best_tcw = tcw_of(R[h], t[h])
                    if not (masks[h] == self.best_mask).all(): self.refines_on_other_set += 1      # Refine reads the best-so-far set, not this hypothesis'
                    ok, T, m, n = self.refine()
                    if ok: res = (T, False, m, n); run = h + 1; break
        self.its += run
        if res is not None: return res[0], False, res[2], res[3], run
        if self.its >= self.max_its:
            if self.best >= self.min_inliers: return self.best_tcw.copy(), True, self.best_mask.copy(), self.best, run
            return None, True, none, 0, run
        return None, False, none, 0, run
