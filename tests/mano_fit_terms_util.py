"""TEST INFRASTRUCTURE ONLY -- fp64 restatement of the MANO fit with joint and keypoint terms (include/poem_hip.h
``poem_mano_fit_terms``), written from that text on top of the unchanged tests/mano_fit_util.py (``assets``, ``model``,
``solve_step``, ``reg_vector``).  Nothing is shared with csrc/mano_fit.hip: the residual ROWS are formed explicitly, term by term and
view by view (mesh rows, joint rows, two rows per weighted keypoint), the Jacobians of mesh and joints are extrapolated central
differences of the oracle, the cameras are inverted by LAPACK, the normal equations are matmuls of the stacked rows.  ``per_joint``
is the second statement (a 3x3 matrix, a 3-vector and a scalar per joint) the host tests hold against the rows.

Scenes: seeded cameras on a ring around the hand, 0.5 to 0.7 m away, looking at it, fx = fy = 250, 256 x 256 images."""
import functools
import math

import torch

import mano_fit_util as u

F64 = torch.float64
NX = u.NX
H_STEP = u.H_STEP
ZMIN = 1e-3                      # include/poem_hip.h POEM_FIT_ZMIN
IMAGE = 256.0


# ---- model and Jacobians -----------------------------------------------------------------------------------------------------------
def _central(a, x, h):
    e = torch.eye(NX, dtype=F64) * h
    v, j = u.model(a, torch.cat([x[None] + e, x[None] - e]))
    dv = ((v[:NX] - v[NX:]) / (2 * h)).reshape(NX, -1).t().contiguous()
    dj = ((j[:NX] - j[NX:]) / (2 * h)).reshape(NX, -1).t().contiguous()
    return dv, dj


def jacobians(a, x, h=H_STEP):
    """dV/dx (2334,61) and dP/dx (63,61) at x: central differences at h and 2h, extrapolated (4 J_h - J_2h) / 3"""
    x = x.to(F64)
    (v1, j1), (v2, j2) = _central(a, x, h), _central(a, x, 2 * h)
    return (4 * v1 - v2) / 3, (4 * j1 - j2) / 3


# ---- terms ---------------------------------------------------------------------------------------------------------------------------
def make_terms(target=None, mesh_weight=1.0, j3=None, w3=None, kp=None, w2=None, K=None, T=None, scale=IMAGE):
    """One sample's data terms (fp32 tensors as the device gets them, or None): target (778,3); j3 (21,3), w3 (21,); kp (n,21,2),
    w2 (n,21), K (n,3,3), T (n,4,4) camera->master."""
    if j3 is not None and w3 is None:
        w3 = torch.ones(21)
    if kp is not None and w2 is None:
        w2 = torch.ones(kp.shape[0], 21)
    return dict(target=target, mesh_weight=float(mesh_weight), j3=j3, w3=w3, kp=kp, w2=w2, K=K, T=T, scale=float(scale))


def project(K, T, P):
    """P (21,3) fp64 in the master frame -> (uv (21,2), p_cam (21,3)): inv(T) p, the full 3x3 K, division by h_z"""
    Ti = torch.linalg.inv(T.to(F64))
    pc = P @ Ti[:3, :3].t() + Ti[:3, 3]
    h = pc @ K.to(F64).t()
    return h[:, :2] / h[:, 2:3], pc


def rows(a, x, tm, jac=None):
    """The stacked residual r (R,) and its Jacobian (R,61) at x, and whether a weighted keypoint lies at depth <= ZMIN."""
    x = x.to(F64)
    Jv, Jj = jacobians(a, x) if jac is None else jac
    v, P = u.model(a, x[None])
    v, P = v[0], P[0]
    r, J, behind = [], [], False
    if tm["target"] is not None:
        s = math.sqrt(tm["mesh_weight"])
        r.append(s * (v - tm["target"].to(F64)).reshape(-1))
        J.append(s * Jv)
    if tm["j3"] is not None:
        for j in range(21):
            w = float(tm["w3"][j])
            if w > 0:
                r.append(math.sqrt(w) * (P[j] - tm["j3"][j].to(F64)))
                J.append(math.sqrt(w) * Jj[3 * j:3 * j + 3])
    if tm["kp"] is not None:
        for n in range(tm["kp"].shape[0]):
            if not bool((tm["w2"][n] > 0).any()):
                continue                                                     # (its camera is not read)
            K = tm["K"][n].to(F64)
            Ti = torch.linalg.inv(tm["T"][n].to(F64))
            for j in range(21):
                w = float(tm["w2"][n, j])
                if not w > 0:
                    continue
                pc = Ti[:3, :3] @ P[j] + Ti[:3, 3]
                h = K @ pc
                uv = h[:2] / h[2]
                behind = behind or bool(pc[2] <= ZMIN)
                s = math.sqrt(w) / tm["scale"]
                dpi = torch.stack([(K[0] - uv[0] * K[2]) / h[2], (K[1] - uv[1] * K[2]) / h[2]])      # (2,3) d uv / d p_cam
                r.append(s * (uv - tm["kp"][n, j].to(F64)))
                J.append(s * dpi @ Ti[:3, :3] @ Jj[3 * j:3 * j + 3])
    if not r:
        return torch.zeros(0, dtype=F64), torch.zeros(0, NX, dtype=F64), behind
    return torch.cat(r), torch.cat(J), behind


def evaluate(a, x, tm, shape_reg=0.0, pose_reg=0.0, order=0, jac=None):
    """c, g, H at x.  ``order`` 0: one matmul over the rows; 1: the rows in reverse, 96 at a time.  A weighted keypoint at depth
    <= ZMIN: c = +inf."""
    x = x.to(F64)
    r, J, behind = rows(a, x, tm, jac)
    lam = u.reg_vector(shape_reg, pose_reg)
    if order == 0:
        c, g, H = r @ r, J.t() @ r, J.t() @ J
    else:
        c, g, H = torch.zeros((), dtype=F64), torch.zeros(NX, dtype=F64), torch.zeros(NX, NX, dtype=F64)
        Jf, rf = J.flip(0), r.flip(0)
        for s in range(0, len(rf), 96):
            c, g, H = c + rf[s:s + 96] @ rf[s:s + 96], g + Jf[s:s + 96].t() @ rf[s:s + 96], H + Jf[s:s + 96].t() @ Jf[s:s + 96]
    c = c + (lam * x * x).sum()
    if behind:
        c = torch.tensor(float("inf"), dtype=F64)
    return c, g + lam * x, H + torch.diag(lam)


def per_joint(a, x, tm, jac=None):
    """The joint and keypoint terms in the second form: per joint W (3,3) = sum M^T M, b (3,) = sum M^T r, s = sum r^2 over term J
    and the views in order, then H = sum_j Jj^T W_j Jj, g = sum_j Jj^T b_j, c = sum_j s_j -> (c, g, H) without mesh and regularisers."""
    x = x.to(F64)
    _, Jj = jacobians(a, x) if jac is None else jac
    P = u.model(a, x[None])[1][0]
    c, g, H = torch.zeros((), dtype=F64), torch.zeros(NX, dtype=F64), torch.zeros(NX, NX, dtype=F64)
    for j in range(21):
        W, b, s = torch.zeros(3, 3, dtype=F64), torch.zeros(3, dtype=F64), torch.zeros((), dtype=F64)
        if tm["j3"] is not None and float(tm["w3"][j]) > 0:
            w, d = float(tm["w3"][j]), P[j] - tm["j3"][j].to(F64)
            W, b, s = W + w * torch.eye(3, dtype=F64), b + w * d, s + w * (d @ d)
        for n in range(0 if tm["kp"] is None else tm["kp"].shape[0]):
            w = float(tm["w2"][n, j])
            if not w > 0:
                continue
            K, Ti = tm["K"][n].to(F64), torch.linalg.inv(tm["T"][n].to(F64))
            pc = Ti[:3, :3] @ P[j] + Ti[:3, 3]
            h = K @ pc
            uv = h[:2] / h[2]
            M = math.sqrt(w) / tm["scale"] * torch.stack([(K[0] - uv[0] * K[2]) / h[2], (K[1] - uv[1] * K[2]) / h[2]]) @ Ti[:3, :3]
            rr = math.sqrt(w) / tm["scale"] * (uv - tm["kp"][n, j].to(F64))
            W, b, s = W + M.t() @ M, b + M.t() @ rr, s + rr @ rr
        Jq = Jj[3 * j:3 * j + 3]
        c, g, H = c + s, g + Jq.t() @ b, H + Jq.t() @ W @ Jq
    return c, g, H


def joints_start(a, j3):
    """The rigid rule on the 21 zero-pose, zero-shape joints against j3 (21,3): Kabsch rotation through the quaternion, tsl = the
    centroid difference after the rotation."""
    t = j3.to(F64)
    x = torch.zeros(NX, dtype=F64)
    p = u.model(a, x[None])[1][0]
    pc, gc = p - p.mean(0), t - t.mean(0)
    U, _, Vt = torch.linalg.svd(gc.t() @ pc)
    d = torch.sign(torch.linalg.det(U @ Vt))
    R = U @ torch.diag(torch.tensor([1.0, 1.0, float(d)], dtype=F64)) @ Vt
    x[:3] = u.matrix_to_axis_angle(R)
    x[58:] = t.mean(0) - u.model(a, x[None])[1][0].mean(0)
    return x


def lm(a, tm, x0, iters=8, shape_reg=0.0, pose_reg=0.0, h=H_STEP):
    """The iteration of the definition on the terms (``mano_fit_util.lm``'s, with this file's ``evaluate``; an infinite or NaN
    candidate cost is never accepted).  ``h``: the Jacobians' step."""
    x = x0.to(F64).clone()
    ev = lambda z: evaluate(a, z, tm, shape_reg, pose_reg, jac=jacobians(a, z, h))        # noqa: E731
    c, g, H = ev(x)
    mu, acc, dxs, mus, xs, cs, cand = 1e-3, [], [], [], [x], [float(c)], []
    for _ in range(iters):
        dx = u.solve_step(g, H, mu)
        mus.append(mu)
        dxs.append(dx)
        cn, gn, Hn = ev(x + dx)
        cand.append(float(cn))
        ok = bool(cn < c)
        acc.append(ok)
        if ok:
            x, c, g, H, mu = x + dx, cn, gn, Hn, max(mu / 10, 1e-9)
        else:
            mu = min(mu * 10, 1e8)
        xs.append(x)
        cs.append(float(c))
    return dict(x=x, cost=float(c), accepted=acc, dx=dxs, mu=mus, g=g, H=H, xs=xs, costs=cs, candidate_costs=cand,
                joints=u.model(a, x[None])[1][0])


# ---- measured bars -------------------------------------------------------------------------------------------------------------------
def eval_bars(x, tm, shape_reg=0.0, pose_reg=0.0):
    """-> (c, g, H) of the restatement at x and the MEASURED relative bars, as ``mano_fit_util.eval_bars`` measures them: two
    summation orders and two Jacobians (steps h and h / 2); a bar is four times the sum of the two spreads plus the bound of a
    recursive fp64 sum of the rows, relative to the cost, max|g|, max|H| (keys c, g, H) and the 2-norms (g2, H2).  Above 1e-9: refused."""
    a = u.assets()
    Ja, Jb = jacobians(a, x, H_STEP), jacobians(a, x, H_STEP / 2)
    nrows = len(rows(a, x, tm, Ja)[0])
    row_eps = nrows * 2.0 ** -53
    c0, g0, H0 = evaluate(a, x, tm, shape_reg, pose_reg, jac=Ja)
    c1, g1, H1 = evaluate(a, x, tm, shape_reg, pose_reg, order=1, jac=Ja)
    c2, g2, H2 = evaluate(a, x, tm, shape_reg, pose_reg, jac=Jb)
    mx = lambda t: float(t.abs().max())                                   # noqa: E731
    n2 = lambda t: float(torch.linalg.matrix_norm(t, ord=2)) if t.dim() == 2 else float(t.norm())       # noqa: E731
    bars = dict(H=4 * (mx(H0 - H1) + mx(H0 - H2)) / mx(H0) + row_eps, g=4 * (mx(g0 - g1) + mx(g0 - g2)) / mx(g0) + row_eps,
                c=4 * (abs(float(c0 - c1)) + abs(float(c0 - c2))) / float(c0) + row_eps,
                H2=4 * (n2(H0 - H1) + n2(H0 - H2)) / n2(H0) + row_eps, g2=4 * (n2(g0 - g1) + n2(g0 - g2)) / n2(g0) + row_eps)
    assert max(bars.values()) < 1e-9, bars
    return (c0, g0, H0), bars


# ---- seeded scenes -------------------------------------------------------------------------------------------------------------------
def ring_cameras(seed, n, centre):
    """n cameras on a ring around ``centre`` (3,), 0.5 .. 0.7 m away, looking at it -> K (n,3,3), T (n,4,4) camera->master, fp32"""
    g = torch.Generator().manual_seed(seed)
    ang = 2 * math.pi * (torch.arange(n, dtype=F64) + 0.3 * torch.rand(n, generator=g, dtype=F64)) / max(n, 1)
    elev = 0.5 * (torch.rand(n, generator=g, dtype=F64) - 0.5)
    dist = 0.5 + 0.2 * torch.rand(n, generator=g, dtype=F64)
    K, T = torch.zeros(n, 3, 3, dtype=F64), torch.zeros(n, 4, 4, dtype=F64)
    for i in range(n):
        d = torch.stack([torch.cos(ang[i]) * torch.cos(elev[i]), torch.sin(elev[i]), torch.sin(ang[i]) * torch.cos(elev[i])])
        pos = centre.to(F64) + dist[i] * d
        z = -d
        xa = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=F64), z)
        xa = xa / xa.norm()
        ya = torch.linalg.cross(z, xa)
        T[i, :3, 0], T[i, :3, 1], T[i, :3, 2], T[i, :3, 3], T[i, 3, 3] = xa, ya, z, pos, 1.0
        K[i] = torch.tensor([[250.0 + 5 * float(torch.rand((), generator=g)), 0, 128.0], [0, 250.0, 128.0], [0, 0, 1.0]], dtype=F64)
    return K.float(), T.float()


def observe(x, K, T, noise_px=0.0, seed=0):
    """keypoints (n,21,2) fp32 of the model's joints at x (61,) in every view, optionally with Gaussian pixel noise"""
    P = u.model(u.assets(), x[None].to(F64))[1][0]
    kp = torch.stack([project(K[n], T[n], P)[0] for n in range(K.shape[0])]) if K.shape[0] else torch.zeros(0, 21, 2, dtype=F64)
    if noise_px:
        kp = kp + noise_px * torch.randn(kp.shape, generator=torch.Generator().manual_seed(seed), dtype=F64)
    return kp.float()


def min_depth(x, tm):
    P = u.model(u.assets(), x[None].to(F64))[1][0]
    return min(float(project(tm["K"][n], tm["T"][n], P)[1][:, 2].min()) for n in range(tm["kp"].shape[0]))


EVAL_VIEWS = [1, 3, 5, 2]        # the ragged batch of the evaluation tests: sample i uses eval pose i


@functools.lru_cache(maxsize=None)
def eval_scene(kind):
    """The evaluation batch for ``kind`` in "K", "J", "MJK": a list of four (name, x0 (61,) fp32, terms) -- the four
    ``mano_fit_util.eval_poses`` with 1, 3, 5, 2 views.  The observations come from another pose (``eval_target``'s), tens of
    centimetres away: large residuals, so that g and the cost carry weight; every depth stays above 0.1 m.  Some weights are 0,
    the others between 0.5 and 1.5.  Cached: leave it unchanged."""
    a = u.assets()
    x_obs = (u.seeded_params(21, 1) * 0.8 + 0.2 * u.seeded_params(5, 1))[0]
    out = []
    for i, (name, x0) in enumerate(u.eval_poses().items()):
        centre = u.model(a, x0[None])[1][0].mean(0)
        K, T = ring_cameras(100 + i, EVAL_VIEWS[i], centre)
        g = torch.Generator().manual_seed(200 + i)
        w2 = 0.5 + torch.rand(EVAL_VIEWS[i], 21, generator=g)
        w2[torch.rand(EVAL_VIEWS[i], 21, generator=g) < 0.15] = 0.0
        w3 = 0.5 + torch.rand(21, generator=g)
        w3[torch.rand(21, generator=g) < 0.15] = 0.0
        j3 = u.model(a, x_obs[None])[1][0].float()
        tm = make_terms(target=u.eval_target() if "M" in kind else None, mesh_weight=0.75,
                        j3=j3 if "J" in kind else None, w3=w3 if "J" in kind else None,
                        kp=observe(x_obs, K, T) if "K" in kind else None, w2=w2 if "K" in kind else None, K=K, T=T)
        if "K" in kind:
            assert min_depth(x0, tm) > 0.1
        out.append((name, x0, tm))
    return out


@functools.lru_cache(maxsize=None)
def fit_scene(seed=11, sample=1, views=4, noise_px=0.0, noise_mm=0.0):
    """A fitting scene on ``mano_fit_util.recovery_case(seed)[sample]``: cameras around the true hand, keypoints of the true joints
    (+ pixel noise), the mesh target (+ noise_mm).  -> dict(x_true, clean_joints (21,3) fp64, target (778,3) fp32, K, T, kp)."""
    case = u.recovery_case(seed, 3, noise_mm)
    x = case["x_true"][sample]
    P = u.model(u.assets(), x[None])[1][0]
    K, T = ring_cameras(300 + seed + sample, views, P.mean(0))
    return dict(x_true=x, clean_joints=P, target=case["target"][sample], K=K, T=T, kp=observe(x, K, T, noise_px, seed=seed + 77))


def lm_cases():
    """name -> (x0 (61,) fp32, terms) of the one- and two-step tests, keypoints only, 3 views: "far" starts tens of centimetres
    away; "overshoot" starts 2.5 rad (sigma) off in every joint.  Their accept / reject sequences: ``LM_EXPECT`` (host-checked)."""
    sc = fit_scene(views=3)
    g = torch.Generator().manual_seed(4)
    x = sc["x_true"].clone()
    x[:48] += 2.5 * torch.randn(48, generator=g)
    far = sc["x_true"].clone()
    far[3:48] = 0
    far[58:] += torch.tensor([0.05, -0.04, 0.06])
    tm = make_terms(kp=sc["kp"], K=sc["K"], T=sc["T"])
    return {"far": (far, tm), "overshoot": (x, tm)}


def depth_cases():
    """"behind": a start whose hand lies behind camera 0 (status 4).  "crossing": a start just in front of camera 0 whose first
    candidate crosses POEM_FIT_ZMIN and is rejected by the restatement (host-checked) -> name -> (x0, terms)"""
    sc = fit_scene(views=2)
    tm = make_terms(kp=sc["kp"], K=sc["K"], T=sc["T"])
    T0 = sc["T"][0].double()
    centre = sc["clean_joints"].mean(0)
    out = {}
    for name, depth in (("behind", -0.10), ("crossing", CROSSING_DEPTH)):
        x = sc["x_true"].clone().double()
        x[58:] += (T0[:3, 3] + depth * T0[:3, 2]) - centre                  # the joints' centroid at `depth` along camera 0's axis
        out[name] = (x.float(), tm)
    return out


CROSSING_DEPTH = 0.0228          # found on the CPU: the start's nearest joint is 1.31 mm in front of camera 0, the first candidate's 0.84 mm
# the accept / reject sequences of ``lm_cases`` and of ``depth_cases()["crossing"]`` (host-checked; every rejection is decisive: the
# rejected cost is infinite or more than 1.001 times the accepted one, round-off being 1e-12)
LM_EXPECT = {"far": [True, True], "overshoot": [False, False], "crossing": [False, True]}
REG = u.REG

# the combined case: mesh with 2 mm noise + clean keypoints in 4 views, mesh_weight 1; weight_2d chosen on the CPU so that the
# restatement's joints are nearer to the clean joints than its mesh-only fit's (host-checked)
COMBINED = dict(seed=11, sample=1, views=4, noise_mm=2.0, weight_2d=1.0e3)


@functools.lru_cache(maxsize=None)
def kponly_reference():
    """Keypoints only: 4 clean views of ``fit_scene()``, x0 = the mesh default start, iters = 8 -> (scene, x0 fp32, terms, the
    restatement's fit with the Jacobians at H_STEP, the same at H_STEP / 2).  Cached: leave it unchanged."""
    sc = fit_scene(views=4)
    tm = make_terms(kp=sc["kp"], K=sc["K"], T=sc["T"])
    x0 = u.default_start(u.assets(), sc["target"]).float()
    return sc, x0, tm, lm(u.assets(), tm, x0, iters=8), lm(u.assets(), tm, x0, iters=8, h=H_STEP / 2)


@functools.lru_cache(maxsize=None)
def combined_reference():
    """``COMBINED`` -> (scene, terms, the restatement's combined fit at H_STEP, at H_STEP / 2, its mesh-only fit), all from the
    default start of the noisy mesh, iters = 8.  Cached: leave it unchanged."""
    C = COMBINED
    sc = fit_scene(C["seed"], C["sample"], C["views"], 0.0, C["noise_mm"])
    a = u.assets()
    x0 = u.default_start(a, sc["target"])
    tm = make_terms(target=sc["target"], kp=sc["kp"], w2=torch.full((C["views"], 21), float(C["weight_2d"])), K=sc["K"], T=sc["T"])
    return sc, tm, lm(a, tm, x0, iters=8), lm(a, tm, x0, iters=8, h=H_STEP / 2), lm(a, make_terms(target=sc["target"]), x0, iters=8)
