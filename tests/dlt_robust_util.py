"""fp64 numpy restatement of the outlier-robust triangulation (``poem_dlt_robust``, include/poem_hip.h) and the seeded inputs its
tests share.  Upstream has no counterpart (lib/utils/triangulation.py stops at ``triangulate_dlt``), so this file is the yardstick:
it is written from the definition in the header and not from the kernel.

Per (sample, joint): every pair (a < c) of the sample's N views -> two-view DLT -> view v is an inlier iff r_v^2 < px^2 and its depth
is > 0 (both strict) -> key (-count, sum of the inliers' r^2 in view order, a N + c), smallest wins -> with >= 2 inliers the DLT over
the inlier set, else (and for a sample with a camera that is not finite) the DLT over all views with an empty inlier set -> `refine`
Gauss-Newton steps on the summed r^2 of the views solved over, each kept only if the sum gets strictly smaller."""
import numpy as np
import torch

SHIFT_PX, NOISE_PX = 40.0, 0.5


def view_matrices(K, T, m32=False):
    """(N,3,4) M = K . T[:3]: in fp64 from the fp32 inputs, or (m32) in fp32 as the device forms it (matmul order aside)."""
    if m32:
        return (K.astype(np.float32) @ T.astype(np.float32)[:, :3, :]).astype(np.float64)
    return K.astype(np.float64) @ T.astype(np.float64)[:, :3, :]


def solve(M, uv):
    """DLT of one joint: M (n,3,4), uv (n,2) -> X (3,): smallest right singular vector x of the rows (u M[2] - M[0], v M[2] - M[1]),
    sign x[3] >= 0, X = x[:3] / (x[3] + 1e-7)."""
    uv = uv.astype(np.float64)
    rows = np.concatenate([uv[:, 0:1] * M[:, 2] - M[:, 0], uv[:, 1:2] * M[:, 2] - M[:, 1]], 0)
    if not np.isfinite(rows).all():
        return np.full(3, np.nan)
    x = np.linalg.svd(rows)[2][-1]
    if x[3] < 0:
        x = -x
    return x[:3] / (x[3] + 1e-7)


def reproject(M, X, uv):
    """-> (r^2 (n,), depth (n,)) of X in every view"""
    with np.errstate(all="ignore"):
        h = M[:, :, :3] @ X + M[:, :, 3]
        d = h[:, :2] / h[:, 2:3] - uv.astype(np.float64)
        return (d * d).sum(1), h[:, 2]


def pick(keys):
    """index of the smallest (-count, sum, id) in lexicographic order"""
    return min(range(len(keys)), key=lambda i: keys[i])


def hypotheses(M, uv, px):
    """-> [(key, inlier mask (n,) bool)] of every pair, in the order of a N + c"""
    n, out = len(M), []
    for a in range(n):
        for c in range(a + 1, n):
            r2, depth = reproject(M, solve(M[[a, c]], uv[[a, c]]), uv)
            inl = (r2 < px * px) & (depth > 0)
            s = 0.0
            for v in np.where(inl)[0]:                         # in view order, as the definition says
                s += r2[v]
            out.append(((-int(inl.sum()), s, a * n + c), inl))
    return out


def hypothesis_margin(c, px):
    """min | r - px | over every view of every pair hypothesis of the case: how far any inlier decision is from flipping"""
    offs, m = np.concatenate([[0], np.cumsum(c["views"])]).astype(int), np.inf
    for s, e in zip(offs[:-1], offs[1:]):
        M = view_matrices(c["K"][s:e], c["T"][s:e])
        for j in range(c["uv"].shape[1]):
            p = c["uv"][s:e, j]
            for a in range(e - s):
                for k in range(a + 1, e - s):
                    r2 = reproject(M, solve(M[[a, k]], p[[a, k]]), p)[0]
                    m = min(m, float(np.abs(np.sqrt(r2) - px).min()))
    return m


def gauss_newton(M, uv, X, iters):
    """-> (X, [cost before, cost after every accepted step])"""
    cost = reproject(M, X, uv)[0].sum()
    trace = [cost]
    for _ in range(iters):
        with np.errstate(all="ignore"):
            h = M[:, :, :3] @ X + M[:, :, 3]
            p = h[:, :2] / h[:, 2:3]
            Jm = (M[:, :2, :3] - p[:, :, None] * M[:, 2:3, :3]) / h[:, 2, None, None]          # (n,2,3)
            e = (p - uv.astype(np.float64)).reshape(-1)
            Jm = Jm.reshape(-1, 3)
            try:
                Y = X - np.linalg.solve(Jm.T @ Jm, Jm.T @ e)
            except np.linalg.LinAlgError:
                break
            trial = reproject(M, Y, uv)[0].sum()
        if not trial < cost:
            break
        X, cost = Y, trial
        trace.append(cost)
    return X, trace


def restate(uv, K, T, views, px, refine=0, m32=False, want_trace=False):
    """uv (BN,J,2), K (BN,3,3), T (BN,4,4) master->camera -> out (B,J,3) fp64, inlier (BN,J) bool, count (B,J) int32, resid (BN,J) fp64
    pixels (NaN where not finite) [, the refinement's cost traces and the winning pair ids]."""
    offs = np.concatenate([[0], np.cumsum(views)]).astype(int)
    J = uv.shape[1]
    out, count = np.zeros((len(views), J, 3)), np.zeros((len(views), J), dtype=np.int32)
    inlier, resid = np.zeros((uv.shape[0], J), dtype=bool), np.zeros((uv.shape[0], J))
    traces, winners = [], []
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        M = view_matrices(K[s:e], T[s:e], m32)
        broken = not np.isfinite(M).all()
        for j in range(J):
            p = uv[s:e, j]
            mask, win = np.zeros(e - s, dtype=bool), None
            if not broken:
                hyp = hypotheses(M, p, px)
                win = pick([k for k, _ in hyp])
                if -hyp[win][0][0] >= 2:
                    mask = hyp[win][1]
            over = mask if mask.any() else np.ones(e - s, dtype=bool)
            X = solve(M[over], p[over])
            X, tr = gauss_newton(M[over], p[over], X, refine) if refine else (X, [])
            out[b, j], count[b, j], inlier[s:e, j] = X, int(mask.sum()), mask
            with np.errstate(all="ignore"):
                r = np.sqrt(reproject(M, X, p)[0]).astype(np.float32).astype(np.float64)
            resid[s:e, j] = np.where(np.isfinite(r), r, np.nan)
            traces.append(tr)
            winners.append(None if win is None else hyp[win][0][2])
    return (out, inlier, count, resid, traces, winners) if want_trace else (out, inlier, count, resid)


def plain(uv, K, T, views):
    """the plain DLT over all views, fp64"""
    offs = np.concatenate([[0], np.cumsum(views)]).astype(int)
    return np.stack([np.stack([solve(view_matrices(K[s:e], T[s:e]), uv[s:e, j]) for j in range(uv.shape[1])])
                     for s, e in zip(offs[:-1], offs[1:])])


def n_outliers(views, many):
    """2 and 3 views: none; 4 and 5: one; from 8 on: one, or (many) floor((N - 1) / 3)"""
    return [0 if n < 4 else ((n - 1) // 3 if many and n >= 8 else 1) for n in views]


def make_case(views, outliers, seed, J=21):
    """Cameras of ``inputs.synthetic_batch(views, seed)``, joints = its reference joints (J = 21) or J points within 8 cm of their
    mean, uv = the exact projection + 0.5 px Gaussian noise rounded to fp32; ``outliers[b]`` randomly chosen views of sample b get a
    40 px displacement in a random direction per joint.  -> dict of numpy arrays: uv, K, E (camera->master), T (its fp32 inverse), X,
    planted (BN,J) bool = the views that are clean, views."""
    import poem_v2_amd as pk
    b = pk.inputs.synthetic_batch(views, seed=seed)
    K, E = b["img_metas"]["cam_intr"], b["img_metas"]["cam_extr"]
    T = torch.linalg.inv(E)
    g = torch.Generator().manual_seed(9000 + seed)
    X = b["reference_joints"]
    if J != 21:
        X = X.mean(1, keepdim=True) + 0.08 * (torch.rand(len(views), J, 3, generator=g) * 2 - 1)
    vs = torch.repeat_interleave(torch.arange(len(views)), torch.tensor(views))
    pc = (T[:, None, :3, :3].double() @ X[vs].double()[..., None]).squeeze(-1) + T[:, None, :3, 3].double()
    q = (K[:, None].double() @ pc[..., None]).squeeze(-1)
    uv = q[..., :2] / q[..., 2:] + NOISE_PX * torch.randn(sum(views), J, 2, generator=g, dtype=torch.float64)
    clean = torch.ones(sum(views), dtype=torch.bool)
    off = 0
    for n, k in zip(views, outliers):
        for v in torch.randperm(n, generator=g)[:k].tolist():
            ang = 2 * np.pi * torch.rand(J, generator=g, dtype=torch.float64)
            uv[off + v] += SHIFT_PX * torch.stack([torch.cos(ang), torch.sin(ang)], -1)
            clean[off + v] = False
        off += n
    return {"uv": uv.float().numpy(), "K": K.numpy(), "E": E.numpy(), "T": T.numpy(), "X": X.double().numpy(),
            "planted": clean[:, None].repeat(1, J).numpy(), "views": list(views)}


def keep_views(c, keep):
    """the case with only the views of the boolean (BN,) ``keep``"""
    offs = np.concatenate([[0], np.cumsum(c["views"])]).astype(int)
    out = {k: c[k][keep] for k in ("uv", "K", "E", "T", "planted")}
    out["X"], out["views"] = c["X"], [int(keep[s:e].sum()) for s, e in zip(offs[:-1], offs[1:])]
    return out


def one_sample(c, b):
    offs = np.concatenate([[0], np.cumsum(c["views"])]).astype(int)
    s, e = offs[b], offs[b + 1]
    out = {k: c[k][s:e] for k in ("uv", "K", "E", "T", "planted")}
    out["X"], out["views"] = c["X"][b:b + 1], [c["views"][b]]
    return out
