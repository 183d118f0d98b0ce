"""numpy restatement of Initializer (src/sg-slam/src/Initializer.cc) and the OpenCV 3.4 algebra it calls (tests only): float32 arithmetic in the reference's order,
double where OpenCV uses double.  JacobiSVDImpl_<float> (one-sided Jacobi on the rows of A^T, or of A itself when m < n; the FULL_UV completion from
cv::RNG(0x12345678)), cv::gemm's small-matrix path, the closed-form 3 x 3 inverse and determinant, cv::norm / Mat::dot in double: written from their published
algorithm, with the assumptions sg_slam_amd/csrc/sgx_init_kernels.h lists.  The Jacobi rotation's std::hypot is the kernel's sgx_init_hypot.  Sums are sequential
(np.cumsum), arrays carry a leading batch axis (hypotheses or matches), lanes the C code would leave alone are masked; so the results are the emulator's bits."""
import math
import numpy as np

F = np.float32
FLT_MIN = float(np.finfo('f4').tiny)
EPS = F(2.0 ** -22)                # FLT_EPSILON * 2


def f4(x): return np.asarray(x, 'f4')
def f8(x): return np.asarray(x, 'f8')


def seqsum(x, axis=-1):
    """x[0] + x[1] + ... in order along axis, in x's own precision"""
    return np.cumsum(x, axis=axis).take(-1, axis=axis)


def hypot(x, y):
    a = np.abs(x); b = np.abs(y)
    sw = a < b
    a, b = np.where(sw, b, a), np.where(sw, a, b)
    with np.errstate(all='ignore'):
        r = b / a
        h = a * np.sqrt(1.0 + r * r)
    return np.where((a == 0) | (b == 0), a + b, h)


def _rng_next(state):
    state = ((state & 0xffffffff) * 4164903690 + (state >> 32)) & ((1 << 64) - 1)
    return state, state & 0xffffffff


def _complete_scalar(At, W, m, n, n1):
    """the completion / normalisation loop of JacobiSVDImpl_<float> on one matrix (in place)"""
    rng = 0x12345678
    for i in range(n1):
        sd = float(W[i]) if i < n else 0.0
        ii = 0
        while ii < 100 and sd <= FLT_MIN:
            val0 = F(1. / m)
            for k in range(m):
                rng, r = _rng_next(rng)
                At[i, k] = val0 if r & 256 else -val0
            for _ in range(2):
                for j in range(i):
                    sd = 0.0
                    for k in range(m): sd += float(At[i, k] * At[j, k])
                    asum = F(0)
                    for k in range(m):
                        t = F(float(At[i, k]) - sd * float(At[j, k])); At[i, k] = t; asum = asum + np.abs(t)
                    with np.errstate(all='ignore'):
                        asum = F(1) / asum if asum > EPS * F(100) else F(0)
                    for k in range(m): At[i, k] = At[i, k] * asum
            sd = 0.0
            for k in range(m): sd += float(At[i, k]) * float(At[i, k])
            sd = math.sqrt(sd); ii += 1
        s = F(1 / sd if sd > FLT_MIN else 0.)
        At[i] = At[i] * s


def jacobi(At, m, n, n1, want_vt=True):
    """JacobiSVDImpl_<float>(At, W, Vt, m, n, n1, FLT_MIN, 2 FLT_EPSILON) on a batch: At (H, max(n, n1), m) float32 -> (At, W (H, n) float64 descending, Vt (H, n, n))"""
    At = np.array(At, 'f4'); H = At.shape[0]
    eps = float(EPS)
    W = seqsum(f8(At[:, :n]) ** 2, -1)
    Vt = np.broadcast_to(np.eye(n, dtype='f4'), (H, n, n)).copy()
    active = np.ones(H, bool)
    with np.errstate(all='ignore'):
        for _ in range(max(m, 30)):
            changed = np.zeros(H, bool)
            for i in range(n - 1):
                for j in range(i + 1, n):
                    Ai = At[:, i, :].copy(); Aj = At[:, j, :].copy()
                    a = W[:, i].copy(); b = W[:, j].copy()
                    p = seqsum(f8(Ai) * f8(Aj), -1)
                    rot = active & ~(np.abs(p) <= eps * np.sqrt(a * b))
                    if not rot.any(): continue
                    p = p * 2
                    beta = a - b; gamma = hypot(p, beta)
                    neg = beta < 0
                    delta = (gamma - beta) * 0.5
                    s_n = f4(np.sqrt(delta / gamma)); c_n = f4(p / (gamma * f8(s_n) * 2))
                    c_p = f4(np.sqrt((gamma + beta) / (gamma * 2))); s_p = f4(p / (gamma * f8(c_p) * 2))
                    c = np.where(neg, c_n, c_p)[:, None]; s = np.where(neg, s_n, s_p)[:, None]
                    t0 = c * Ai + s * Aj; t1 = (-s) * Ai + c * Aj
                    r = rot[:, None]
                    At[:, i, :] = np.where(r, t0, Ai); At[:, j, :] = np.where(r, t1, Aj)
                    W[:, i] = np.where(rot, seqsum(f8(t0) ** 2, -1), a); W[:, j] = np.where(rot, seqsum(f8(t1) ** 2, -1), b)
                    if want_vt:
                        Vi = Vt[:, i, :].copy(); Vj = Vt[:, j, :].copy()
                        Vt[:, i, :] = np.where(r, c * Vi + s * Vj, Vi); Vt[:, j, :] = np.where(r, (-s) * Vi + c * Vj, Vj)
                    changed |= rot
            active = changed
            if not changed.any(): break
        W = np.sqrt(seqsum(f8(At[:, :n]) ** 2, -1))
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
        if n1 > 0:
            hard = ~(W > FLT_MIN).all(1)                           # a zero (or NaN) singular value: that matrix takes the scalar loop
            easy = ~hard; At0 = At.copy()
            At[easy, :n] = At[easy, :n] * f4(1 / W[easy])[:, :, None]
            if n1 > n and easy.any():                             # rows n .. n1 - 1 of every easy matrix: the same random row (the generator starts at its seed)
                rng = 0x12345678
                for i in range(n, n1):
                    vals = []
                    for k in range(m): rng, r = _rng_next(rng); vals.append(F(1. / m) if r & 256 else -F(1. / m))
                    v = np.broadcast_to(f4(vals), (H, m)).copy()
                    for _ in range(2):
                        for j in range(i):
                            sd = seqsum(f8(v * At[:, j, :]), -1)
                            t = f4(f8(v) - sd[:, None] * f8(At[:, j, :]))
                            asum = seqsum(np.abs(t), -1)
                            asum = np.where(asum > EPS * F(100), F(1) / asum, F(0))
                            v = t * asum[:, None]
                    sd = np.sqrt(seqsum(f8(v) ** 2, -1))
                    again = easy & ~(sd > FLT_MIN)                  # would draw again: that matrix takes the scalar loop from the rows before the normalisation
                    At[again] = At0[again]; hard |= again; easy &= ~again
                    At[:, i, :] = np.where(easy[:, None], v * f4(1 / sd)[:, None], At[:, i, :])
            for h in np.nonzero(hard)[0]:
                _complete_scalar(At[h], W[h], m, n, n1)
    return At, W, Vt


def svd3(A):
    """cv::SVD::compute(A (H, 3, 3)) -> U, w (float32), Vt"""
    At, W, Vt = jacobi(np.swapaxes(f4(A), 1, 2), 3, 3, 3)
    return np.swapaxes(At, 1, 2), f4(W), Vt


def mul3(A, B, alpha=1.0):
    """cv::gemm's small-matrix path: float dot product left to right, (float)(dot * alpha) in double"""
    A = f4(A); B = f4(B)
    t = A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :] + A[..., :, 2, None] * B[..., None, 2, :]
    return f4(f8(t) * np.asarray(alpha, 'f8')[..., None, None])


def mul3_tn(A, B):
    """A^T B on the generic path: double accumulation"""
    A = f8(A); B = f8(B)
    s = np.zeros(np.broadcast_shapes(A.shape, B.shape))
    for k in range(3): s = s + A[..., k, :, None] * B[..., k, None, :]
    return f4(s * 1.0)


def mulv3(A, b):
    A = f4(A); b = f4(b)
    t = A[..., :, 0] * b[..., None, 0] + A[..., :, 1] * b[..., None, 1] + A[..., :, 2] * b[..., None, 2]
    return f4(f8(t) * 1.0)


def det3(m):
    m4 = f4(m); m = f8(m4)
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1]) - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0]) +
            m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def inv3(S):
    S = f8(f4(S)); d = det3(S)
    with np.errstate(all='ignore'):
        di = 1. / d
        g = lambda a, b, c, e: (S[..., a // 3, a % 3] * S[..., b // 3, b % 3] - S[..., c // 3, c % 3] * S[..., e // 3, e % 3]) * di
        D = np.stack([g(4, 8, 5, 7), g(2, 7, 1, 8), g(1, 5, 2, 4), g(5, 6, 3, 8), g(0, 8, 2, 6), g(2, 3, 0, 5), g(3, 7, 4, 6), g(1, 6, 0, 7), g(0, 4, 1, 3)], -1)
    D = np.where((d == 0)[..., None], 0.0, D)
    return f4(D).reshape(S.shape)


def dot3d(a, b):
    a = f8(f4(a)); b = f8(f4(b))
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def unit3(t):
    t = f4(t)
    with np.errstate(all='ignore'):
        inv = f4(1. / np.sqrt(dot3d(t, t)))
    return t * inv[..., None]


# ---------------------------------------------------------------------------------------------------------------------------------------------------- Initializer
def normalize(xy):
    """Normalize (:749-795) over all keys of a frame: (meanX, meanY, sX, sY) float32"""
    xy = f4(xy).reshape(-1, 2); n = len(xy)
    with np.errstate(all='ignore'):
        mean = (seqsum(xy, 0) if n else np.zeros(2, 'f4')) / F(n)
        dev = (seqsum(np.abs(xy - mean), 0) if n else np.zeros(2, 'f4')) / F(n)
        s = f4(1.0 / f8(dev))
    return f4([mean[0], mean[1], s[0], s[1]])


def T_of(nm):
    return f4([[nm[2], 0, -nm[0] * nm[2]], [0, nm[3], -nm[1] * nm[3]], [0, 0, 1]])


def draw_sets(N, draws):
    """mvSets (:82-97): draws (its, 8) raw rand() values -> (its, 8) indices into mvMatches12"""
    out = np.zeros((len(draws), 8), 'i8')
    for h, d in enumerate(draws):
        avail = {}
        for k in range(8):
            size = N - k
            r = min(max(int((float(d[k]) / (2147483647.0 + 1.0)) * size), 0), size - 1)
            out[h, k] = avail.get(r, r)
            avail[r] = avail.get(size - 1, size - 1)
    return out


def compute_h21(p1, p2):
    """ComputeH21 (:226-266) on a batch: p1, p2 (H, 8, 2) normalised points -> Hn (H, 3, 3)"""
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    z = np.zeros_like(u1); o = np.ones_like(u1)
    r0 = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], -1); r1 = np.stack([u1, v1, o, z, z, z, (-u2) * u1, (-u2) * v1, -u2], -1)
    A = np.stack([r0, r1], 2).reshape(len(u1), 16, 9)
    _, _, Vt = jacobi(np.swapaxes(A, 1, 2), 16, 9, 0)
    return Vt[:, 8, :].reshape(-1, 3, 3)


def compute_f21(p1, p2):
    """ComputeF21 (:268-303): the 8 x 9 system (vt.row(8) = the completed ninth row), then the rank-2 projection"""
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1)
    At = np.concatenate([A, np.zeros((len(A), 1, 9), 'f4')], 1)
    At, _, _ = jacobi(At, 9, 8, 9, want_vt=False)
    Fpre = At[:, 8, :].reshape(-1, 3, 3)
    U, w, Vt = svd3(Fpre)
    w = w.copy(); w[:, 2] = 0
    D = np.zeros((len(A), 3, 3), 'f4')
    for i in range(3): D[:, i, i] = w[:, i]
    return mul3(mul3(U, D), Vt)


def check_homography(H21, H12, xy, sigma):
    """CheckHomography (:305-388) for hypotheses H21, H12 (H, 3, 3) over matches xy (N, 4): score (H) float32, inliers (H, N)"""
    h = f4(H21).reshape(-1, 9, 1); hi = f4(H12).reshape(-1, 9, 1)
    u1, v1, u2, v2 = (f4(xy)[None, :, k] for k in range(4))
    th = F(5.991); inv = f4(1.0 / f8(F(sigma) * F(sigma)))
    with np.errstate(all='ignore'):
        w2 = f4(1.0 / f8(hi[:, 6] * u2 + hi[:, 7] * v2 + hi[:, 8]))
        a = (hi[:, 0] * u2 + hi[:, 1] * v2 + hi[:, 2]) * w2; b = (hi[:, 3] * u2 + hi[:, 4] * v2 + hi[:, 5]) * w2
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv
        w1 = f4(1.0 / f8(h[:, 6] * u1 + h[:, 7] * v1 + h[:, 8]))
        a = (h[:, 0] * u1 + h[:, 1] * v1 + h[:, 2]) * w1; b = (h[:, 3] * u1 + h[:, 4] * v1 + h[:, 5]) * w1
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv
        return _score(chi1, chi2, th, th)


def check_fundamental(F21, xy, sigma):
    """CheckFundamental (:390-468): the gate is 3.841, the score counts from 5.991"""
    f = f4(F21).reshape(-1, 9, 1)
    u1, v1, u2, v2 = (f4(xy)[None, :, k] for k in range(4))
    inv = f4(1.0 / f8(F(sigma) * F(sigma)))
    with np.errstate(all='ignore'):
        a2 = f[:, 0] * u1 + f[:, 1] * v1 + f[:, 2]; b2 = f[:, 3] * u1 + f[:, 4] * v1 + f[:, 5]; c2 = f[:, 6] * u1 + f[:, 7] * v1 + f[:, 8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv
        a1 = f[:, 0] * u2 + f[:, 3] * v2 + f[:, 6]; b1 = f[:, 1] * u2 + f[:, 4] * v2 + f[:, 7]; c1 = f[:, 2] * u2 + f[:, 5] * v2 + f[:, 8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv
        return _score(chi1, chi2, F(3.841), F(5.991))


def _score(chi1, chi2, th, th_score):
    out1 = chi1 > th; out2 = chi2 > th
    c = np.stack([np.where(out1, F(0), th_score - chi1), np.where(out2, F(0), th_score - chi2)], -1).reshape(len(chi1), -1)     # adding +0 leaves a score >= 0 unchanged
    return seqsum(f4(c), -1), ~out1 & ~out2


def first_strict_max(scores):
    """`if(currentScore>score)` from score = 0 in iteration order: index of the winner or -1 (a NaN never wins)"""
    best = F(0); win = -1
    for h, s in enumerate(scores):
        if s > best: best = s; win = h
    return win, best


def check_rt(R, t, xy, inl, cam, th2):
    """CheckRT (:798-907) for hypotheses R (Q, 3, 3), t (Q, 3) over the matches xy (N, 4) with vbMatchesInliers inl (N):
    state (Q, N) 0 / 1 counted in nGood / 2 also vbGood, cosParallax (Q, N), points (Q, N, 3)"""
    R = f4(R); t = f4(t); xy = f4(xy); Q = len(R); N = len(xy)
    fx, fy, cx, cy = (F(c) for c in cam)
    K = f4([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    P1 = f4([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]])
    Rt = np.concatenate([R, t[:, :, None]], 2)                     # (Q, 3, 4)
    P2 = f4(f8(K[None, :, 0, None] * Rt[:, None, 0, :] + K[None, :, 1, None] * Rt[:, None, 1, :] + K[None, :, 2, None] * Rt[:, None, 2, :]) * 1.0)
    O2 = f4((f8(R[:, 0, :]) * f8(t[:, 0, None]) + f8(R[:, 1, :]) * f8(t[:, 1, None]) + f8(R[:, 2, :]) * f8(t[:, 2, None])) * -1.0)
    x1, y1, x2, y2 = (xy[None, :, k, None] for k in range(4))
    bc = lambda a: np.broadcast_to(a, (Q, N, 4))
    M = np.stack([bc(x1 * P1[None, None, 2] - P1[None, None, 0]), bc(y1 * P1[None, None, 2] - P1[None, None, 1]),
                  x2 * P2[:, None, 2] - P2[:, None, 0], y2 * P2[:, None, 2] - P2[:, None, 1]], 2)            # (Q, N, 4, 4)
    _, _, Vt = jacobi(np.swapaxes(M.reshape(-1, 4, 4), 1, 2), 4, 4, 0)
    v = Vt[:, 3, :].reshape(Q, N, 4)
    with np.errstate(all='ignore'):
        inv = f4(1.0 / f8(v[..., 3]))
        X = v[..., :3] * inv[..., None]
        fin = np.isfinite(X).all(-1)
        n2 = X - O2[:, None, :]
        d1 = f4(np.sqrt(dot3d(X, X))); d2 = f4(np.sqrt(dot3d(n2, n2)))
        cosp = f4(dot3d(X, n2) / f8(d1 * d2))
        low = f8(cosp) < 0.99998
        X2 = f4(f8(R[:, None, :, 0] * X[..., None, 0] + R[:, None, :, 1] * X[..., None, 1] + R[:, None, :, 2] * X[..., None, 2]) * 1.0 + f8(t[:, None, :]) * 1.0)
        ok = inl[None, :] & fin & ~((X[..., 2] <= 0) & low) & ~((X2[..., 2] <= 0) & low)
        iz1 = f4(1.0 / f8(X[..., 2]))
        ex = fx * X[..., 0] * iz1 + cx - xy[None, :, 0]; ey = fy * X[..., 1] * iz1 + cy - xy[None, :, 1]
        ok &= ~((ex * ex + ey * ey) > th2)
        iz2 = f4(1.0 / f8(X2[..., 2]))
        ex = fx * X2[..., 0] * iz2 + cx - xy[None, :, 2]; ey = fy * X2[..., 1] * iz2 + cy - xy[None, :, 3]
        ok &= ~((ex * ex + ey * ey) > th2)
    state = np.where(ok, np.where(low, 2, 1), 0).astype('u1')
    return state, cosp, X


def parallax_of(c):
    c = float(F(c))
    return F(math.acos(c) * 180 / math.pi) if -1.0 <= c <= 1.0 else F(np.nan)


def faugeras(H21, cam):
    """ReconstructH's eight motion hypotheses (:584-686): (R (8, 3, 3), t (8, 3)) or None at the `d1/d2 < 1.00001 || d2/d3 < 1.00001` exit"""
    fx, fy, cx, cy = (F(c) for c in cam)
    K = f4([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    A = mul3(mul3(inv3(K), H21), K)
    U, w, Vt = svd3(A[None]); U, w, Vt = U[0], w[0], Vt[0]
    s = F(det3(U) * det3(Vt))
    d1, d2, d3 = w
    with np.errstate(all='ignore'):
        if float(d1 / d2) < 1.00001 or float(d2 / d3) < 1.00001: return None
        den = d1 * d1 - d3 * d3
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / den); aux3 = np.sqrt((d2 * d2 - d3 * d3) / den)
        x1 = [aux1, aux1, -aux1, -aux1]; x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2); ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2); cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        Rs = []; ts = []
        for i in range(8):
            q = i & 3
            if i < 4:
                Rp = f4([[ct, 0, -st[q]], [0, 1, 0], [st[q], 0, ct]]); tp = f4([x1[q] * (d1 - d3), F(0) * (d1 - d3), -x3[q] * (d1 - d3)])
            else:
                Rp = f4([[cp, 0, sp[q]], [0, -1, 0], [sp[q], 0, -cp]]); tp = f4([x1[q] * (d1 + d3), F(0) * (d1 + d3), x3[q] * (d1 + d3)])
            Rs.append(mul3(mul3(U, Rp, float(s)), Vt)); ts.append(unit3(mulv3(U, tp)))
    return f4(Rs), f4(ts)


def decompose_e(F21, cam):
    """ReconstructF's four motion hypotheses (:479-497, DecomposeE :909-929)"""
    fx, fy, cx, cy = (F(c) for c in cam)
    K = f4([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    E = mul3(mul3_tn(K, F21), K)
    U, w, Vt = svd3(E[None]); U, Vt = U[0], Vt[0]
    t = unit3(U[:, 2].copy())
    W = f4([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
    R1 = mul3(mul3(U, W), Vt); R2 = mul3(mul3(U, W.T.copy()), Vt)
    if det3(R1) < 0: R1 = -R1
    if det3(R2) < 0: R2 = -R2
    return f4([R1, R2, R1, R2]), f4([t, t, -t, -t])


class InitializerRef:
    """the reference class on host arrays: keys (n, 2) float32 undistorted points, cam = fx, fy, cx, cy"""

    def __init__(self, keys1, cam, sigma=1.0, iterations=200):
        self.k1 = f4(keys1).reshape(-1, 2); self.cam = tuple(float(F(c)) for c in cam); self.sigma = F(sigma); self.iterations = int(iterations)

    def models(self, keys2, matches12, draws):
        """FindHomography / FindFundamental: everything up to RH.  Returns a dict, or None when N < 8"""
        k2 = f4(keys2).reshape(-1, 2); m = np.asarray(matches12, 'i8').reshape(-1)
        i1 = np.nonzero((m >= 0) & (m < len(k2)))[0]; i2 = m[i1]; N = len(i1)
        out = dict(i1=i1, i2=i2, N=N, xy=np.concatenate([self.k1[i1], k2[i2]], 1) if N else np.zeros((0, 4), 'f4'))
        if N < 8: return out
        sets = draw_sets(N, np.asarray(draws, 'i8').reshape(-1)[:8 * self.iterations].reshape(self.iterations, 8))
        nm1 = normalize(self.k1); nm2 = normalize(k2)
        T1 = T_of(nm1); T2 = T_of(nm2)
        with np.errstate(all='ignore'):
            pn1 = (self.k1 - nm1[:2]) * nm1[2:]; pn2 = (k2 - nm2[:2]) * nm2[2:]
            p1 = pn1[i1][sets]; p2 = pn2[i2][sets]
            H21 = mul3(mul3(inv3(T2), compute_h21(p1, p2)), T1); H12 = inv3(H21)
            F21 = mul3(mul3(T2.T.copy(), compute_f21(p1, p2)), T1)
            sh, inh = check_homography(H21, H12, out['xy'], self.sigma); sf, inf_ = check_fundamental(F21, out['xy'], self.sigma)
        wh, SH = first_strict_max(sh); wf, SF = first_strict_max(sf)
        out.update(sets=sets, H21s=H21, F21s=F21, scores_h=sh, scores_f=sf, win_h=wh, win_f=wf, SH=SH, SF=SF,
                   H21=H21[wh] if wh >= 0 else np.zeros((3, 3), 'f4'), F21=F21[wf] if wf >= 0 else np.zeros((3, 3), 'f4'),
                   inl_h=inh[wh] if wh >= 0 else np.zeros(N, bool), inl_f=inf_[wf] if wf >= 0 else np.zeros(N, bool))
        return out

    def initialize(self, keys2, matches12, draws):
        """(ok, R21, t21, vP3D, vbTriangulated, inliers, report) as sg_slam_amd.initializer.Initializer.Initialize returns them; report['outcome'] names the path taken"""
        n1 = len(self.k1)
        R21 = np.zeros((3, 3), 'f4'); t21 = np.zeros(3, 'f4'); P = np.zeros((n1, 3), 'f4'); tri = np.zeros(n1, bool); inl = np.zeros(n1, bool)
        M = self.models(keys2, matches12, draws); N = M['N']
        rep = dict(SH=0.0, SF=0.0, RH=float('nan'), model=1, n_matches=N, n_inliers_h=0, n_inliers_f=0, n_hyp=0, best_hyp=-1, n_good=np.zeros(8, 'i4'),
                   cos_parallax=np.zeros(8, 'f4'), parallax=np.zeros(8, 'f4'), H21=np.zeros(9, 'f4'), F21=np.zeros(9, 'f4'), outcome='few_matches')
        if N < 8: return False, R21, t21, P, tri, inl, rep
        SH, SF = M['SH'], M['SF']
        with np.errstate(all='ignore'): RH = SH / (SH + SF)
        model = 0 if float(RH) > 0.40 else 1
        rep.update(SH=float(SH), SF=float(SF), RH=float(RH), model=model, n_inliers_h=int(M['inl_h'].sum()), n_inliers_f=int(M['inl_f'].sum()),
                   H21=M['H21'].reshape(9), F21=M['F21'].reshape(9))
        if (SH if model == 0 else SF) <= 0: rep['outcome'] = 'no_model'; return False, R21, t21, P, tri, inl, rep
        mi = M['inl_h'] if model == 0 else M['inl_f']; Nin = int(mi.sum())
        inl[M['i1']] = mi
        hyp = faugeras(M['H21'], self.cam) if model == 0 else decompose_e(M['F21'], self.cam)
        if hyp is None: rep['outcome'] = 'd_ratio_exit'; return False, R21, t21, P, tri, inl, rep
        Rs, ts = hyp; Q = len(Rs)
        th2 = F(4.0 * float(self.sigma * self.sigma))
        state, cosp, X = check_rt(Rs, ts, M['xy'], mi, self.cam, th2)
        ngood = (state > 0).sum(1); sel = np.zeros(Q, 'f4'); par = np.zeros(Q, 'f4')
        for q in range(Q):
            if ngood[q] > 0:
                c = np.sort(cosp[q][state[q] > 0]); sel[q] = c[min(50, len(c) - 1)]; par[q] = parallax_of(sel[q])
        rep['n_hyp'] = Q; rep['n_good'][:Q] = ngood; rep['cos_parallax'][:Q] = sel; rep['parallax'][:Q] = par
        win = -1
        if model == 0:
            bestGood = secondBest = 0; best = -1
            for q in range(8):
                if ngood[q] > bestGood: secondBest = bestGood; bestGood = int(ngood[q]); best = q
                elif ngood[q] > secondBest: secondBest = int(ngood[q])
            rep['best_hyp'] = best
            enough = best >= 0 and secondBest < 0.75 * bestGood and bestGood > 50 and bestGood > 0.9 * Nin
            if enough and par[best] >= F(1.0): win = best
            rep['outcome'] = 'ok_h' if win >= 0 else ('parallax' if enough else 'ambiguous')
        else:
            maxGood = int(ngood.max()); nMinGood = max(int(0.9 * Nin), 50)
            nsimilar = int(sum(1 for q in range(4) if ngood[q] > 0.7 * maxGood))
            best = int(np.nonzero(ngood == maxGood)[0][0]); rep['best_hyp'] = best
            enough = not (maxGood < nMinGood or nsimilar > 1)
            if enough and par[best] > F(1.0): win = best            # the else-if chain tests the first hypothesis equal to maxGood only
            rep['outcome'] = 'ok_f' if win >= 0 else ('parallax' if enough else 'ambiguous')
        if win >= 0:
            R21 = Rs[win].copy(); t21 = ts[win].copy()
            g = state[win] > 0
            P[M['i1'][g]] = X[win][g]; tri[M['i1'][g]] = state[win][g] == 2
        return win >= 0, R21, t21, P, tri, inl, rep
