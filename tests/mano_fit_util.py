"""TEST INFRASTRUCTURE ONLY -- fp64 restatement of the MANO fit's definition (include/poem_hip.h ``poem_mano_fit``), written from
that text on top of ``oracle/mano_oracle.py::mano_lbs``.  Nothing is shared with csrc/mano_fit.hip: the Jacobian here is a batched
central difference of the oracle (one ``mano_lbs`` call of 122 samples per step size, Richardson-extrapolated from two step
sizes), the normal equations are torch matmuls, the Cholesky is LAPACK's, the default start is an SVD Kabsch, and the LM loop
is a plain Python loop.  The seeded cases of tests/test_mano_fit.py and tests/test_mano_fit_host.py live here too."""
import functools
import math

import numpy as np
import torch

import mano_oracle as mo

NV, NX = 778, 61
F64 = torch.float64
H_STEP = 1e-4            # central-difference step; the error of the extrapolated Jacobian is O(h^4) + eps / h  (~1e-11 relative)


def composed_regression(a):
    """The joint regression as the prepared table holds it (csrc/mano.hip's header: composed with the template and the shape
    basis, fp64 products added vertex by vertex, rounded ONCE to fp32) -> JT (16,3), JSD (16,3,10), fp32 values in fp64 arrays."""
    jr, vt, sd = (np.asarray(a[k], dtype=np.float64) for k in ("J_regressor", "v_template", "shapedirs"))
    jt, jsd = np.zeros((16, 3)), np.zeros((16, 3, 10))
    for v in range(NV):                          # the kernel's order: one vertex after the other
        jt += jr[:, v, None] * vt[v]
        jsd += jr[:, v, None, None] * sd[v]
    return jt.astype(np.float32).astype(np.float64), jsd.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def assets(seed=3):
    """The seeded synthetic assets as fp64 arrays, for ``mano_lbs`` -- with the regressor moved by its least-norm correction onto
    the model the fit is defined on: J_regressor' . (v_template | shapedirs) = the table's composed, once-rounded regression.
    (Without it the fp32 rounding of the composed joints, ~2e-9 m, would be a difference of 1e-8 relative between the two
    statements of H -- of the models, not of the arithmetic.)  ``composed_error`` is what is left of that equation."""
    import poem_v2_amd as pk
    a = {k: np.asarray(v, dtype=np.float64) for k, v in pk.mano.synthetic_mano_assets(seed).items()}
    jt, jsd = composed_regression(a)
    M = np.concatenate([a["v_template"], a["shapedirs"].reshape(NV, 30)], 1)            # (778, 33)
    want = np.concatenate([jt, jsd.reshape(16, 30)], 1)                                  # (16, 33)
    jr = a["J_regressor"]
    for _ in range(2):                            # (a second pass removes the first one's rounding)
        jr = jr + np.linalg.lstsq(M.T, (want - jr @ M).T, rcond=None)[0].T
    a["J_regressor"] = jr
    return a


def composed_error(seed=3):
    """max |J_regressor' . (v_template | shapedirs) - the table's composed regression| of ``assets(seed)``"""
    import poem_v2_amd as pk
    a = assets(seed)
    jt, jsd = composed_regression(pk.mano.synthetic_mano_assets(seed))
    M = np.concatenate([a["v_template"], a["shapedirs"].reshape(NV, 30)], 1)
    return float(np.abs(a["J_regressor"] @ M - np.concatenate([jt, jsd.reshape(16, 30)], 1)).max())


def model(a, x):
    """x (B,61) -> verts (B,778,3), joints (B,21,3) in fp64: the uncentred MANO mesh plus tsl."""
    x = x.to(F64)
    v, j = mo.mano_lbs(a, x[:, :48], x[:, 48:58], center_idx=None)
    return v + x[:, None, 58:], j + x[:, None, 58:]


def _central(a, x, h):
    e = torch.eye(NX, dtype=F64) * h
    v, _ = model(a, torch.cat([x[None] + e, x[None] - e]))
    return ((v[:NX] - v[NX:]) / (2 * h)).reshape(NX, NV * 3).t().contiguous()


def jacobian(a, x, h=H_STEP, with_error=False):
    """dV/dx at x (61,) -> (2334,61).  Central differences at h and 2h, extrapolated: J = (4 J_h - J_2h) / 3.  ``with_error``
    adds max|J - J_h|, the error of the UNextrapolated J_h -- an over-estimate of J's own."""
    x = x.to(F64)
    j1, j2 = _central(a, x, h), _central(a, x, 2 * h)
    j = (4 * j1 - j2) / 3
    return (j, float((j - j1).abs().max())) if with_error else j


def reg_vector(shape_reg, pose_reg):
    lam = torch.zeros(NX, dtype=F64)
    lam[3:48], lam[48:58] = pose_reg, shape_reg
    return lam


def evaluate(a, x, target, shape_reg=0.0, pose_reg=0.0, order=0, jac=None):
    """c, g, H at x (61,) against target (778,3).  ``order`` 0: one matmul; 1: the rows in reverse, accumulated tile by tile
    (another summation order of the same numbers)."""
    x = x.to(F64)
    J = jacobian(a, x) if jac is None else jac
    r = (model(a, x[None])[0][0] - target.to(F64)).reshape(-1)
    lam = reg_vector(shape_reg, pose_reg)
    if order == 0:
        c, g, H = r @ r, J.t() @ r, J.t() @ J
    else:
        c, g, H = torch.zeros((), dtype=F64), torch.zeros(NX, dtype=F64), torch.zeros(NX, NX, dtype=F64)
        Jf, rf = J.flip(0), r.flip(0)
        for s in range(0, NV * 3, 96):
            c, g, H = c + rf[s:s + 96] @ rf[s:s + 96], g + Jf[s:s + 96].t() @ rf[s:s + 96], H + Jf[s:s + 96].t() @ Jf[s:s + 96]
    return c + (lam * x * x).sum(), g + lam * x, H + torch.diag(lam)


def solve_step(g, H, mu):
    """dx of (H + mu D) dx = -g, D = max(diag H, 1e-12); zeros where the Cholesky meets a pivot that is not positive / finite."""
    M = H + mu * torch.diag(H.diagonal().clamp_min(1e-12))
    if not bool(torch.isfinite(M).all()):
        return torch.zeros_like(g)
    L, info = torch.linalg.cholesky_ex(M)
    if int(info) != 0 or not bool(torch.isfinite(L).all()):
        return torch.zeros_like(g)
    return torch.cholesky_solve(-g[:, None], L)[:, 0]


def condition_number(H, mu):
    M = H + mu * torch.diag(H.diagonal().clamp_min(1e-12))
    return float(torch.linalg.cond(M))


def matrix_to_axis_angle(R):
    """(3,3) fp64 rotation -> axis-angle through the quaternion whose largest component is taken first (finite at angle pi)."""
    q2 = torch.stack([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                      1 - R[0, 0] - R[1, 1] + R[2, 2]])
    m = int(q2.argmax())
    h = 0.5 * math.sqrt(max(float(q2[m]), 0.0))
    f = 0.25 / h
    a, b, c = float(R[2, 1] - R[1, 2]), float(R[0, 2] - R[2, 0]), float(R[1, 0] - R[0, 1])
    xy, xz, yz = float(R[0, 1] + R[1, 0]), float(R[0, 2] + R[2, 0]), float(R[1, 2] + R[2, 1])
    q = {0: (h, a * f, b * f, c * f), 1: (a * f, h, xy * f, xz * f), 2: (b * f, xy * f, h, yz * f), 3: (c * f, xz * f, yz * f, h)}[m]
    q = torch.tensor(q, dtype=F64)
    q = q / q.norm() * (-1.0 if q[0] < 0 else 1.0)
    n = float(q[1:].norm())
    return q[1:] * (2.0 * math.atan2(n, float(q[0])) / n if n > 1e-12 else 2.0)


def default_start(a, target):
    """Root rotation = the rigid, scale-free alignment (Kabsch) of the zero-pose, zero-shape mesh onto the target; fingers and
    betas 0; tsl = the centroid difference after the rotation."""
    t = target.to(F64)
    vt = torch.as_tensor(a["v_template"]).to(F64)
    pc, gc = vt - vt.mean(0), t - t.mean(0)
    U, _, Vt = torch.linalg.svd(gc.t() @ pc)
    d = torch.sign(torch.linalg.det(U @ Vt))
    R = U @ torch.diag(torch.tensor([1.0, 1.0, float(d)], dtype=F64)) @ Vt
    x = torch.zeros(NX, dtype=F64)
    x[:3] = matrix_to_axis_angle(R)
    x[58:] = t.mean(0) - model(a, x[None])[0][0].mean(0)
    return x


def lm(a, target, x0=None, iters=8, shape_reg=0.0, pose_reg=0.0):
    """The iteration of the definition.  -> dict(x, cost, accepted (list of bool per iteration), dx (list), mu (list: the mu each
    solve used), g, H (at the result's x), xs / costs (iters + 1: the accepted point and its cost after each iteration))."""
    x = default_start(a, target) if x0 is None else x0.to(F64).clone()
    c, g, H = evaluate(a, x, target, shape_reg, pose_reg)
    mu, acc, dxs, mus, xs, cs = 1e-3, [], [], [], [x], [float(c)]
    for _ in range(iters):
        dx = solve_step(g, H, mu)
        mus.append(mu)
        dxs.append(dx)
        cn, gn, Hn = evaluate(a, x + dx, target, shape_reg, pose_reg)
        ok = bool(cn < c)                      # (a NaN compares false)
        acc.append(ok)
        if ok:
            x, c, g, H, mu = x + dx, cn, gn, Hn, max(mu / 10, 1e-9)
        else:
            mu = min(mu * 10, 1e8)
        xs.append(x)
        cs.append(float(c))
    return dict(x=x, cost=float(c), accepted=acc, dx=dxs, mu=mus, g=g, H=H, xs=xs, costs=cs)


# ---- seeded cases ----------------------------------------------------------------------------------------------------------------
def seeded_params(seed, n):
    """(n,61) fp32: root rotations about random axes by angles up to 2.8 rad, fingers sigma 0.4 rad, betas sigma 1, tsl sigma 0.3 m"""
    g = torch.Generator().manual_seed(seed)
    axis = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=F64), dim=-1)
    ang = 2.8 * torch.rand(n, 1, generator=g, dtype=F64)
    ang[0] = 2.8                                 # the largest angle always occurs
    x = torch.cat([axis * ang, 0.4 * torch.randn(n, 45, generator=g, dtype=F64), torch.randn(n, 10, generator=g, dtype=F64),
                   0.3 * torch.randn(n, 3, generator=g, dtype=F64)], 1)
    return x.float()


@functools.lru_cache(maxsize=None)
def recovery_case(seed=11, n=3, noise_mm=0.0):
    """-> dict(x_true (n,61) fp32, clean (n,778,3) fp64, target (n,778,3) fp32 = fp32(clean + noise)).  Cached: leave it unchanged."""
    x = seeded_params(seed, n)
    clean = model(assets(), x)[0]
    g = torch.Generator().manual_seed(seed + 1000)
    noise = 1e-3 * noise_mm * torch.randn(clean.shape, generator=g, dtype=F64)
    return dict(x_true=x, clean=clean, target=(clean + noise).float())


@functools.lru_cache(maxsize=None)
def recovery_reference(seed=11, n=3, noise_mm=0.0, iters=8):
    """The restatement's own fit of every sample of ``recovery_case`` from the default start -> list of ``lm`` results, with the
    fitted mesh added as ``verts`` (778,3) fp64."""
    case = recovery_case(seed, n, noise_mm)
    out = []
    for i in range(n):
        r = lm(assets(), case["target"][i], iters=iters)
        r["verts"] = model(assets(), r["x"][None])[0][0]
        out.append(r)
    return out


def eval_poses():
    """name -> x0 (61,) fp32 of the evaluation tests: a random pose; the exact-zero finger pose; one joint at |aa| = 1e-7; one joint
    at angle 3.1."""
    base = seeded_params(5, 1)[0]
    zero = base.clone()
    zero[3:48] = 0
    tiny = base.clone()
    tiny[3 * 4:3 * 4 + 3] = torch.tensor([6e-8, -6e-8, 5.2915e-8])            # |aa| = 1e-7
    big = base.clone()
    big[3 * 7:3 * 7 + 3] = 3.1 * torch.tensor([0.6, 0.0, 0.8])
    return {"random": base, "zero_fingers": zero, "tiny_joint": tiny, "angle_3.1": big}


def eval_target(seed=21):
    """A target tens of centimetres from every pose of ``eval_poses``: a large residual, so that g and the cost carry weight."""
    return model(assets(), seeded_params(seed, 1) * 0.8 + 0.2 * seeded_params(5, 1))[0][0].float()


def lm_cases():
    """name -> (x0 (61,) fp32, target (778,3) fp32) of the one- and two-step tests: "far" starts tens of centimetres away and is
    accepted twice; "overshoot" starts 2.5 rad (sigma) off in every joint, where the second, nearly undamped step is rejected."""
    g = torch.Generator().manual_seed(4)
    x = recovery_case()["x_true"][0].clone()
    x[:48] += 2.5 * torch.randn(48, generator=g)
    return {"far": (eval_poses()["random"], eval_target()), "overshoot": (x, recovery_case()["target"][0])}


ROW_EPS = NV * 3 * 2.0 ** -53      # the bound of a recursive fp64 sum of the 2334 rows, relative


def eval_bars(x, target, shape_reg=0.0, pose_reg=0.0):
    """-> (c, g, H) of the restatement at x and the MEASURED relative bars the device tests hold the kernels to: cost, gradient and
    normal matrix are formed in two summation orders and from two Jacobians (extrapolated central differences at step h and
    h / 2); a bar is four times the sum of the two spreads plus ROW_EPS, relative to the cost, max|g|, max|H| (keys c, g, H) and to
    the 2-norms (g2, H2).  A bar above 1e-9, loss.hip's precedent, would be no bar: refused here."""
    a = assets()
    Ja, Jb = jacobian(a, x, h=H_STEP), jacobian(a, x, h=H_STEP / 2)
    c0, g0, H0 = evaluate(a, x, target, shape_reg, pose_reg, jac=Ja)
    c1, g1, H1 = evaluate(a, x, target, shape_reg, pose_reg, order=1, jac=Ja)
    c2, g2, H2 = evaluate(a, x, target, shape_reg, pose_reg, jac=Jb)
    mx = lambda t: float(t.abs().max())                                   # noqa: E731
    n2 = lambda t: float(torch.linalg.matrix_norm(t, ord=2)) if t.dim() == 2 else float(t.norm())       # noqa: E731
    bars = dict(H=4 * (mx(H0 - H1) + mx(H0 - H2)) / mx(H0) + ROW_EPS, g=4 * (mx(g0 - g1) + mx(g0 - g2)) / mx(g0) + ROW_EPS,
                c=4 * (abs(float(c0 - c1)) + abs(float(c0 - c2))) / float(c0) + ROW_EPS,
                H2=4 * (n2(H0 - H1) + n2(H0 - H2)) / n2(H0) + ROW_EPS, g2=4 * (n2(g0 - g1) + n2(g0 - g2)) / n2(g0) + ROW_EPS)
    assert max(bars.values()) < 1e-9, bars
    return (c0, g0, H0), bars


LM_EXPECT = {"far": [True, True], "overshoot": [True, False]}       # the accept / reject sequences of ``lm_cases`` (host-checked)
REG = dict(shape_reg=0.5, pose_reg=0.25)                             # the regularised evaluation and two-step runs
