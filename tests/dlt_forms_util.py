"""Restatements, bars and inputs of tests/test_dlt_forms.py (csrc/dlt.hip: dlt_kernel, dlt_conf_kernel).  TEST INFRASTRUCTURE.

Notation: u = 2^-24 (half an fp32 ulp, relative), e = 2^-53 (the same for fp64).

What the kernel computes, per (sample, joint), and what is restated here
------------------------------------------------------------------------
  M[r][c] = fma(K[r][2], T[2][c], fma(K[r][1], T[1][c], fl32(K[r][0] T[0][c])))                  fp32, restated exactly (``restate_M``)
  a0[c]   = u M[2][c] - M[0][c],  a1[c] = v M[2][c] - M[1][c]                                    fp32, in ONE of two roundings:
            two-step fl(fl(u M2) - M0), or fused fl(u M2 - M0) -- the compiler's contraction setting decides, so both are
            restated (``restate_rows(..., fused=)``) and a test accepts either, but the same one for a whole launch.
  Exact rational arithmetic (fractions.Fraction) with one round-to-nearest-even to 24 bits per operation (``rne24``): an fma
  emulated through fp64 would round twice.
  The solve is NOT restated step by step: the reference is the fp64 SVD of the rows (scaled by the confidence in fp64 in the
  weighted mode, one rounding, as the kernel does), the right singular vector x of the smallest singular value WITH THE SIGN
  x[3] >= 0, and X* = x[:3] / (x[3] + 1e-7) (``solve_svd``).  The sign is part of the reference: LAPACK returns either, and the
  two answers differ by X (x3 + d) / (x3 - d) - X ~ 2e-7 |X| / x3 (``sign_gap``), 1.7e-7 m at 0.6 m, 5e-6 m at 5 m.

The bar of the solve (``solve_bar``)
------------------------------------
  |X - X*|_inf <= u |X*|_inf  +  c e kappa (1 + |X*|_inf) / x3,         kappa = sigma1^2 / (sigma3^2 - sigma4^2)
  First term: the one fp32 rounding of each output.  Second term: the kernel finds x as the eigenvector of G = A^T A for its
  smallest eigenvalue sigma4^2.  A symmetric perturbation dG moves that eigenvector by |dx| <= |dG|_2 / gap with
  gap = sigma3^2 - sigma4^2 (Davis-Kahan, first order), and X = x[:3] / x3 turns dx into |dX| <= |dx| (1 + |X|) / x3.  With
  |dG|_2 <= c e sigma1^2 the term follows.  c counts the roundings of the kernel as it is written:
   * accumulation.  The products a_r a_c of fp32 numbers are exact in fp64 (48 bits).  A view adds (p0 + p1) and then G += : two
     roundings, none if contracted; an entry of G is a chain of at most 2N roundings over 2N non-negative-bounded terms:
     |dG_rc| <= 2N e sum |a_r||a_c|, so |dG|_F <= 2N e |A|_F^2 <= 2N e 4 sigma1^2.  The weighted mode rounds d = a conf and each
     product once more: 2N + 3 in place of 2N.                                                    c_acc = 4 (2N + 3 [weighted])
   * Jacobi.  Each rotation (c^, s^) is computed through at most 4 roundings after tt, so c^2 + s^2 = (1 + eps)^2, |eps| <= 5e:
     it is an exact rotation scaled by (1 + eps).  (An inexact ANGLE is no error: any rotation is a similarity.)  Applying it,
     every new element c g_p -+ s g_q has 2 more roundings on |c g_p| + |s g_q| <= |(g_p, g_q)|: 7e |(g_p, g_q)| per element, two
     elements per pair, sqrt(2) 7e |G|_F <= 10 e |G|_F per pass, a column pass and a row pass per rotation, |G|_F <= 2 sigma1^2:
     40 e sigma1^2 per rotation, 6 rotations per sweep.                                          c_rot = 240 per sweep
   * V accumulates the same rotations in a column pass of its own: 10 e |V|_F ... per rotation directly on x (|x| = 1), 60 e per
     sweep, not amplified by the gap; kappa >= 1, so it is folded in.                             c_vec = 60 per sweep
   * the stopping rule off <= 1e-40 diag leaves an off-diagonal norm of 1e-20 sigma1^2: below e, ignored.
  c = c_acc + 300 (sweeps + 1): the sweeps the fp64 numpy restatement of the algorithm takes on that joint (``solve_jacobi``),
  plus one because contraction may move the stopping test by a sweep.  Nothing in c was fitted to the kernel's output.  The
  restatement alone is asserted (CPU) to stay under HALF this bar on every joint of the ladder, and to converge in under 12
  sweeps, which is the kernel's cap.  On the rungs up to sigma1/sigma3 = 1e2 the second term is below u |X*| (asserted), so there
  the bar says "one fp32 rounding of the fp64 answer, twice over".

The ladder (``ladder``)
-----------------------
  Rungs sigma1/sigma3 = 1e1 .. 1e5; a rung holds the joints whose ratio lies in the decade CENTRED on it, [r / sqrt(10),
  r sqrt(10)), and the baseline of each sample is found by bisection so that its first joint sits in [0.7 r, 1.3 r].  Per rung 8
  samples (N in {2, 3, 8, 16} views x a point at 0.6 m and at 5 m), 3 joints each within 2 cm: 24 joints a rung, 40 samples and
  290 views in one ragged launch.  uv is the noise-free projection rounded to fp32 (pixel noise at a 0.03 mm baseline would
  leave no triangulation to speak of); x3 > 0.05 throughout.  ``invert=False``: T = [R | -R C] given in fp32.  ``invert=True``: the
  fp32 camera->master matrix [R^T | C] in a master frame shifted off the rig, inverted by the kernel."""
import contextlib
from fractions import Fraction

import numpy as np
import torch

U, E = 2.0 ** -24, 2.0 ** -53
RUNGS = (1e1, 1e2, 1e3, 1e4, 1e5)
LADDER_VIEWS = (2, 3, 8, 16)
LADDER_DISTS = (0.6, 5.0)
LADDER_J = 3


# ---- exact fp32 arithmetic ---------------------------------------------------------------------------------------------------------
def rne24(q):
    """Fraction -> the nearest fp32 (24-bit significand, ties to even) as a Fraction.  Normal range only (asserted)."""
    if q == 0:
        return q
    a = abs(q)
    ex = a.numerator.bit_length() - a.denominator.bit_length()          # 2^(ex-1) < a < 2^(ex+1)
    if a < Fraction(2) ** ex:
        ex -= 1
    assert Fraction(2) ** ex <= a < Fraction(2) ** (ex + 1) and -126 <= ex <= 127, (q, ex)
    ulp = Fraction(2) ** (ex - 23)
    n, rem = divmod(a, ulp)
    if rem * 2 > ulp or (rem * 2 == ulp and n % 2 == 1):
        n += 1
    r = n * ulp
    return r if q > 0 else -r


def _F(x):
    return Fraction(float(x))


def restate_M(K, T):
    """K (3,3), T (>=3,4) fp32 -> M (3,4) as Fractions holding fp32 values: the kernel's fma chain, one rounding per step."""
    M = [[None] * 4 for _ in range(3)]
    for r in range(3):
        for c in range(4):
            p = rne24(_F(K[r, 0]) * _F(T[0, c]))
            p = rne24(_F(K[r, 1]) * _F(T[1, c]) + p)
            M[r][c] = rne24(_F(K[r, 2]) * _F(T[2, c]) + p)
    return M


def restate_rows(M, uv, fused):
    """M from restate_M, uv (2,) fp32 -> the view's two rows (2,4) float64 (exactly the fp32 values of the chosen rounding)."""
    out = np.empty((2, 4))
    for i in range(2):
        s = _F(uv[i])
        for c in range(4):
            out[i, c] = float(rne24(s * M[2][c] - M[i][c]) if fused else rne24(rne24(s * M[2][c]) - M[i][c]))
    return out


def rows_of(uv, K, T, fused):
    """uv (N,J,2), K (N,3,3), T (N,4,4) fp32 -> rows (J,N,2,4) float64 in the given rounding."""
    N, J = uv.shape[:2]
    out = np.empty((J, N, 2, 4))
    for n in range(N):
        M = restate_M(K[n], T[n])
        for j in range(J):
            out[j, n] = restate_rows(M, uv[n, j], fused)
    return out


def rows_fp64(uv, K, T):
    """The same rows with no fp32 rounding at all: fp64 M = K T[:3] and fp64 rows (the end-to-end reference)."""
    M = K.astype(np.float64) @ T.astype(np.float64)[:, :3, :]
    uv = uv.astype(np.float64)
    r0 = uv[:, :, 0, None] * M[:, None, 2] - M[:, None, 0]
    r1 = uv[:, :, 1, None] * M[:, None, 2] - M[:, None, 1]
    return np.stack([r0, r1], 2).transpose(1, 0, 2, 3)                 # (J,N,2,4)


# ---- the solve ---------------------------------------------------------------------------------------------------------------------
def _scaled(rows, conf):
    A = np.asarray(rows, dtype=np.float64)
    if conf is not None:
        A = A * np.asarray(conf, dtype=np.float64)[:, None, None]       # one fp64 rounding per element, as the kernel's d = a * sc
    return A


def solve_svd(rows, conf=None, sign=+1):
    """rows (N,2,4) -> X* (3,), singular values (4,), x (4,): fp64 SVD, x3 >= 0 (sign=-1: the other sign, for the sign tests)."""
    A = _scaled(rows, conf).reshape(-1, 4)
    s, vt = np.linalg.svd(A)[1:]
    x = vt[-1] if vt[-1, 3] >= 0 else -vt[-1]
    x = x * sign
    s = np.concatenate([s, np.zeros(4 - len(s))])
    return x[:3] / (x[3] + 1e-7), s, x


def sign_gap(X, x3):
    """|X(x3 < 0) - X(x3 >= 0)|_inf predicted: 2e-7 |X|_inf / x3."""
    return 2e-7 * np.abs(X).max() / abs(x3)


def solve_jacobi(rows, conf=None, raw=False):
    """The kernel's algorithm in fp64 python floats: normal matrix in view order, cyclic Jacobi with the kernel's stopping rule,
    smallest diagonal, sign, + 1e-7 -> (X fp64 (3,), sweeps taken[, x3 as the rotations left it, before the sign rule])."""
    A = _scaled(rows, conf)
    G = [[0.0] * 4 for _ in range(4)]
    for v in range(A.shape[0]):
        d0, d1 = [float(t) for t in A[v, 0]], [float(t) for t in A[v, 1]]
        for r in range(4):
            for c in range(r, 4):
                G[r][c] += d0[r] * d0[c] + d1[r] * d1[c]
    for r in range(1, 4):
        for c in range(r):
            G[r][c] = G[c][r]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    sweeps = 0
    for _ in range(12):
        off = diag = 0.0
        for r in range(4):
            diag += G[r][r] * G[r][r]
            for c in range(r + 1, 4):
                off += G[r][c] * G[r][c]
        if off <= 1e-40 * diag and diag < float("inf"):
            break
        sweeps += 1
        for p in range(3):
            for q in range(p + 1, 4):
                if G[p][q] == 0.0:
                    continue
                theta = (G[q][q] - G[p][p]) / (2.0 * G[p][q])
                tt = (1.0 if theta >= 0 else -1.0) / (abs(theta) + (theta * theta + 1.0) ** 0.5)
                c = 1.0 / (tt * tt + 1.0) ** 0.5
                s = tt * c
                for k in range(4):
                    a, b = G[k][p], G[k][q]
                    G[k][p], G[k][q] = c * a - s * b, s * a + c * b
                for k in range(4):
                    a, b = G[p][k], G[q][k]
                    G[p][k], G[q][k] = c * a - s * b, s * a + c * b
                for k in range(4):
                    a, b = V[k][p], V[k][q]
                    V[k][p], V[k][q] = c * a - s * b, s * a + c * b
    m = 0
    for k in range(1, 4):
        if G[k][k] < G[m][m]:
            m = k
    x = [V[k][m] for k in range(4)]
    x3_raw = x[3]
    if x[3] < 0:
        x = [-t for t in x]
    den = x[3] + 1e-7
    X = np.array([x[0] / den, x[1] / den, x[2] / den])
    return (X, sweeps, x3_raw) if raw else (X, sweeps)


def kappa(s):
    return s[0] ** 2 / (s[2] ** 2 - s[3] ** 2)


def c_of(N, sweeps, weighted=False):
    """The constant of the bar's second term (module docstring): accumulation + rotations over the sweeps taken (+1)."""
    return 4 * (2 * N + (3 if weighted else 0)) + 300 * (sweeps + 1)


def solve_bar(Xs, s, x3, N, sweeps, weighted=False):
    """-> (bar, first term, second term) of one joint."""
    a = float(np.abs(Xs).max())
    t1 = U * a
    t2 = c_of(N, sweeps, weighted) * E * kappa(s) * (1.0 + a) / x3
    return t1 + t2, t1, t2


def unit(Xs, s, x3):
    """The bare perturbation unit e kappa (1 + |X|) / x3 (what measured errors are printed in)."""
    return E * kappa(s) * (1.0 + float(np.abs(Xs).max())) / x3


def svd32(rows, conf=None):
    """The fp32 SVD of the same rows (numpy LAPACK in single precision), re-signed: the header's comparison."""
    A = _scaled(rows, conf).reshape(-1, 4).astype(np.float32)
    vt = np.linalg.svd(A)[2]
    x = vt[-1] if vt[-1, 3] >= 0 else -vt[-1]
    return (x[:3] / (x[3] + np.float32(1e-7))).astype(np.float64)


# ---- the oracle, re-signed -----------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def resigned_svd():
    """Inside: torch.linalg.svd returns VT whose LAST row has a non-negative last entry -- dlt_oracle with the sign rule stated."""
    real = torch.linalg.svd

    def svd(A, *a, **k):
        Um, S, VT = real(A, *a, **k)
        sgn = torch.where(VT[..., -1:, 3:] < 0, -torch.ones_like(VT[..., -1:, 3:]), torch.ones_like(VT[..., -1:, 3:]))
        return Um, S, torch.cat([VT[..., :-1, :], VT[..., -1:, :] * sgn], -2)
    torch.linalg.svd = svd
    try:
        yield
    finally:
        torch.linalg.svd = real


# ---- the threshold pass (restated in tests/test_dlt_confidence.py::restate; here only the selection, for packing) -------------------
def selections(conf, views, threshold):
    """conf (BN,J) -> per sample a list over joints of the selected LOCAL view indices, and the thresholds they were taken at:
    conf > thr; while at most one and thr > 0, thr -= 0.05 in fp64; the lowered thr carries to the sample's following joints."""
    offs = np.concatenate([[0], np.cumsum(views)]).astype(int)
    sel, thrs = [], []
    for s, e in zip(offs[:-1], offs[1:]):
        thr, row, trow = float(threshold), [], []
        for j in range(conf.shape[1]):
            cf = conf[s:e, j].astype(np.float64)
            while thr > 0 and int((cf > thr).sum()) <= 1:
                thr -= 0.05
            row.append(np.where(cf > thr)[0])
            trow.append(thr)
        sel.append(row)
        thrs.append(trow)
    return sel, thrs


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def intrinsics(rng, N):
    K = np.zeros((N, 3, 3))
    K[:, 0, 0] = rng.uniform(550, 650, N)
    K[:, 1, 1] = rng.uniform(550, 650, N)
    K[:, 0, 2] = rng.uniform(120, 136, N)
    K[:, 1, 2] = rng.uniform(120, 136, N)
    K[:, 2, 2] = 1.0
    return K.astype(np.float32)


class _Rig:
    """N cameras on a baseline that can be scaled: centres base * pos_n (pos spans [-0.5, 0.5] along x, small y / z jitter), each
    looking down +z up to a rotation of 0.04 rad; points near `point` (camera-cluster frame).  shift: the master frame's origin
    seen from the cluster (invert form only)."""

    def __init__(self, rng, N, point, J, shift=None):
        pos = np.zeros((N, 3))
        pos[:, 0] = np.linspace(-0.5, 0.5, N)
        pos[1:-1, 0] += rng.uniform(-0.3, 0.3, max(N - 2, 0)) / N
        pos[:, 1:] = rng.uniform(-0.15, 0.15, (N, 2))
        self.pos, self.N, self.J = pos, N, J
        self.R = np.stack([_rodrigues(rng.normal(size=3) * 0.04 / np.sqrt(3)) for _ in range(N)])
        self.K = intrinsics(rng, N)
        self.X = np.asarray(point)[None] + rng.uniform(-0.02, 0.02, (J, 3))
        self.shift = np.zeros(3) if shift is None else np.asarray(shift, dtype=np.float64)

    def build(self, base, invert):
        """-> uv (N,J,2), K, mat (N,4,4) fp32 (T master->camera, or E camera->master when invert), T64 the matrix the fp64
        reference uses (mat itself, or inv(E) in fp64)."""
        C = self.shift[None] + base * self.pos
        mat = np.tile(np.eye(4), (self.N, 1, 1))
        if invert:
            mat[:, :3, :3] = self.R.transpose(0, 2, 1)
            mat[:, :3, 3] = C
            mat = mat.astype(np.float32)
            T64 = np.linalg.inv(mat.astype(np.float64))
        else:
            mat[:, :3, :3] = self.R
            mat[:, :3, 3] = -np.einsum("nij,nj->ni", self.R, C)
            mat = mat.astype(np.float32)
            T64 = mat.astype(np.float64)
        Xm = self.X + self.shift[None]
        pc = np.einsum("nij,kj->nki", T64[:, :3, :3], Xm) + T64[:, None, :3, 3]
        q = np.einsum("nij,nkj->nki", self.K.astype(np.float64), pc)
        uv = (q[..., :2] / q[..., 2:]).astype(np.float32)
        return uv, self.K, mat, T64.astype(np.float64)

    def ratio(self, base, invert):
        uv, K, mat, T64 = self.build(base, invert)
        s = np.linalg.svd(rows_fp64(uv, K, T64)[0].reshape(-1, 4))[1]
        return s[0] / s[2]


_LADDERS = {}


def ladder(invert):
    """-> dict(views [40], uv (290,3,2), K, mat, T64, rung (40,) index into RUNGS, dist (40,), base (40,)); built once per form."""
    if invert in _LADDERS:
        return _LADDERS[invert]
    rng = np.random.default_rng(2024 + int(invert))
    out = dict(views=[], uv=[], K=[], mat=[], T64=[], rung=[], dist=[], base=[])
    for ri, r in enumerate(RUNGS):
        for d in LADDER_DISTS:
            for N in LADDER_VIEWS:
                point = np.array([0.1, -0.06, 0.98]) * d
                rig = _Rig(rng, N, point, LADDER_J, shift=(0.21, -0.13, 0.34) if invert else None)
                target = r * rng.uniform(0.7, 1.3)
                lo, hi = 1e-7, 2.0                                       # the ratio falls as the baseline grows
                for _ in range(60):
                    mid = np.sqrt(lo * hi)
                    if rig.ratio(mid, invert) > target:
                        lo = mid
                    else:
                        hi = mid
                base = np.sqrt(lo * hi)
                uv, K, mat, T64 = rig.build(base, invert)
                for k, v in (("uv", uv), ("K", K), ("mat", mat), ("T64", T64)):
                    out[k].append(v)
                out["views"].append(N)
                out["rung"].append(ri)
                out["dist"].append(d)
                out["base"].append(base)
    for k in ("uv", "K", "mat", "T64"):
        out[k] = np.concatenate(out[k], 0)
    for k in ("rung", "dist", "base"):
        out[k] = np.asarray(out[k])
    _LADDERS[invert] = out
    return out


_LADDER_REFS = {}


def ladder_refs(fused):
    """The solve-local ladder's references in one row rounding -> list over samples of list over joints of
    dict(rows, Xs, s, x3, N, sweeps, Xj (the numpy Jacobi restatement), X32 (the fp32 SVD), bar, t1, t2, unit)."""
    if fused in _LADDER_REFS:
        return _LADDER_REFS[fused]
    L = ladder(False)
    offs = np.concatenate([[0], np.cumsum(L["views"])])
    refs = []
    for b, (s0, e0) in enumerate(zip(offs[:-1], offs[1:])):
        rows = rows_of(L["uv"][s0:e0], L["K"][s0:e0], L["mat"][s0:e0], fused)
        refs.append([joint_ref(rows[j]) for j in range(rows.shape[0])])
    _LADDER_REFS[fused] = refs
    return refs


def joint_ref(rows, conf=None):
    Xs, s, x = solve_svd(rows, conf)
    Xj, sweeps = solve_jacobi(rows, conf)
    N = rows.shape[0]
    bar, t1, t2 = solve_bar(Xs, s, x[3], N, sweeps, weighted=conf is not None)
    return dict(rows=rows, Xs=Xs, s=s, x3=x[3], N=N, sweeps=sweeps, Xj=Xj, X32=svd32(rows, conf), bar=bar, t1=t1, t2=t2,
                unit=unit(Xs, s, x[3]))


SIGN_SHIFTS = ((-3.0, 2.0, -4.0), (0.0, 0.0, -3.0), (-1.0, -1.0, -1.0), (3.0, -2.0, 4.0), (5.0, 5.0, 5.0))


def sign_batch():
    """Five samples of 4 views and 5 joints whose master frame lies metres away from the rig, on either side: the fourth column of
    A is then the largest, the smallest eigenvalue ends in another diagonal place than the last, and for the frames on the
    negative side the rotations leave x3 < 0 -- the joints on which the sign rule acts (asserted on the CPU).  T given (invert 0)."""
    rng = np.random.default_rng(77)
    uvs, Ks, Ts = [], [], []
    for sh in SIGN_SHIFTS:
        uv, K, T, _ = _Rig(rng, 4, np.array([0.06, -0.04, 0.6]), 5, shift=sh).build(0.3, False)
        uvs.append(uv), Ks.append(K), Ts.append(T)
    return dict(views=[4] * len(SIGN_SHIFTS), uv=np.concatenate(uvs), K=np.concatenate(Ks), T=np.concatenate(Ts))


def mixed_batch(B, J, seed, lo=2, hi=16):
    """A well-conditioned ragged batch for the bit-for-bit tests: view counts mixed from lo to hi, baseline 0.3 m, points at
    0.6 m, 1.5 px of noise, confidences in (0.05, 1) -> dict(views, uv (BN,J,2), conf (BN,J), K, T, E) fp32."""
    rng = np.random.default_rng(seed)
    views = [int(v) for v in rng.integers(lo, hi + 1, B)]
    if B >= 2:
        views[0], views[-1] = lo, hi
    uvs, Ks, Ts, Es = [], [], [], []
    for N in views:
        rig = _Rig(rng, N, np.array([0.06, -0.04, 0.6]), J, shift=(0.21, -0.13, 0.34))
        uv, K, E, T64 = rig.build(0.3, True)
        uvs.append(uv + rng.normal(size=uv.shape).astype(np.float32) * np.float32(1.5))
        Ks.append(K)
        Es.append(E)
        Ts.append(T64.astype(np.float32))
    BN = sum(views)
    return dict(views=views, uv=np.concatenate(uvs).astype(np.float32), conf=rng.uniform(0.05, 1.0, (BN, J)).astype(np.float32),
                K=np.concatenate(Ks), T=np.concatenate(Ts), E=np.concatenate(Es))


def exact_extrinsics(rng, N):
    """camera->master matrices whose inverse is exact in fp32 and in the kernel's fp64 Gauss-Jordan: signed-permutation rotations,
    dyadic translations (multiples of 2^-6 below 4)."""
    E = np.tile(np.eye(4), (N, 1, 1))
    for n in range(N):
        while True:
            P = np.zeros((3, 3))
            P[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
            if np.linalg.det(P) > 0:
                break
        E[n, :3, :3] = P
        E[n, :3, 3] = rng.integers(-255, 256, 3) / 64.0
    return E.astype(np.float32)
