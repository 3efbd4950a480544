"""The sampling stage (csrc/merge.hip, csrc/sample.hip) restated once in torch, for tests/test_sampling_forms.py: device-agnostic,
float64 by default; with ``fp32=True`` the same steps in fp32 with the summation orders the kernels' source states (k-sequential
Linear sums in steps of four, the dot-product tree of merge_tail_kernel, the view sum in view order).

  1 projection   T = inv(extr) ; p = T_R (bps + centre) + T_t ; q = K p ; z = |q_z| < 1e-7 ? 1e-7 : q_z ; uv = q_xy / z ;
                 grid = uv / res * 2 - 1 ; ix = ((grid_x + 1) W - 1) / 2                                    project_ixiy
  2 table        floor, the two differences, one product, the validity masks, the clamps                    table_from_ixiy
    taps         g[v, c, s] = sum_k x[v, c, pix_k] w_k  (nw, ne, sw, se; zero padding = zero weight)        sample_table
  3 Q1           a sample's (N, C, S) block viewed as (S, N, C): globally the (V S, C) row view of g
  4 h2           merge_net_feature.0 on every Q1 row                                                        mlp0
  5 m            N > 1: sum_{n >= 1} <h_n, h_0> h_n ; N = 1: h_0                                             reduce_views
  6, 7 out       q1 + merge_net_feature.1(m) / N   (N = 1: q1 + ...)                                        stage_from_g

and the index functions of the rows the fused kernels write (merge.hip's header): h2_row_major, h2_tile_major, q1_row."""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24            # unit round-off of fp32
INT_MAX = 0x7FFFFFFF


def xs_of(C):
    """rows of a sample_merge / sample_group tile: 32 P with P = 2 for C <= 256, 1 for C = 512"""
    return 32 if C == 512 else 64


# ---------------------------------------------------------------------------------------------------------------------
# projection and table
def project_ixiy(bps, centre, view_sample, intr, extr, fh, fw, img_w, img_h, dtype=torch.float64, inv=None):
    """-> (ix, iy), each (V, S): un-normalised grid_sample(align_corners=False) coordinates of bps + centre[sample] in every view.
    ``inv``: the inverse extrinsics to use (the kernels': fp64 elimination rounded to fp32); default: the fp64 inverse."""
    dt = dtype
    T = (torch.linalg.inv(extr.double()) if inv is None else inv).to(dt)
    K = intr.to(dt)
    p = bps.to(dt)[None] + centre.to(dt)[view_sample.long()][:, None]          # (V, S, 3)
    px, py, pz = p[..., 0], p[..., 1], p[..., 2]
    t = lambda i, j: T[:, i, j][:, None]      # noqa: E731
    k = lambda i, j: K[:, i, j][:, None]      # noqa: E731
    cx = t(0, 0) * px + t(0, 1) * py + t(0, 2) * pz + t(0, 3)
    cy = t(1, 0) * px + t(1, 1) * py + t(1, 2) * pz + t(1, 3)
    cz = t(2, 0) * px + t(2, 1) * py + t(2, 2) * pz + t(2, 3)
    qx = k(0, 0) * cx + k(0, 1) * cy + k(0, 2) * cz
    qy = k(1, 0) * cx + k(1, 1) * cy + k(1, 2) * cz
    qz = (k(2, 0) * cx + k(2, 1) * cy + k(2, 2) * cz).clone()
    qz[qz.abs() < 1e-7] = 1e-7
    u, w = qx / qz, qy / qz
    if dt == torch.float32:      # the kernel multiplies by the fp32 reciprocal of the image size
        inv_w = torch.tensor(1.0, dtype=dt) / torch.tensor(float(img_w), dtype=dt)
        inv_h = torch.tensor(1.0, dtype=dt) / torch.tensor(float(img_h), dtype=dt)
        gx, gy = u * inv_w.to(u.device) * 2 - 1, w * inv_h.to(u.device) * 2 - 1
    else:
        gx, gy = u * (1.0 / img_w) * 2 - 1, w * (1.0 / img_h) * 2 - 1
    return ((gx + 1) * fw - 1) / 2, ((gy + 1) * fh - 1) / 2


def table_from_ixiy(ix, iy, fh, fw):
    """(ix, iy) (V, S) -> weights (V, S, 4) in the dtype of ix and tap pixels (V, S, 4) int64, order nw, ne, sw, se.  In fp32
    every step is one fp32 operation (floor, difference, product, compare, clamp): the exact function project_table_kernel
    evaluates.  (Coordinates beyond the int32 range: the kernel's float -> int conversion is not defined there; the weights
    are 0 either way, the pixels are whatever the clamp of the float gives.)"""
    fx0, fy0 = torch.floor(ix), torch.floor(iy)
    fx1, fy1 = fx0 + 1, fy0 + 1
    wx1, wy1 = ix - fx0, iy - fy0
    wx0, wy0 = fx1 - ix, fy1 - iy
    vx0, vx1 = (fx0 >= 0) & (fx0 < fw), (fx1 >= 0) & (fx1 < fw)
    vy0, vy1 = (fy0 >= 0) & (fy0 < fh), (fy1 >= 0) & (fy1 < fh)
    zero = torch.zeros_like(ix)
    w = torch.stack([torch.where(vx0 & vy0, wx0 * wy0, zero), torch.where(vx1 & vy0, wx1 * wy0, zero),
                     torch.where(vx0 & vy1, wx0 * wy1, zero), torch.where(vx1 & vy1, wx1 * wy1, zero)], dim=-1)
    cx0, cx1 = fx0.clamp(0, fw - 1).long(), fx1.clamp(0, fw - 1).long()
    cy0, cy1 = fy0.clamp(0, fh - 1).long(), fy1.clamp(0, fh - 1).long()
    pix = torch.stack([cy0 * fw + cx0, cy0 * fw + cx1, cy1 * fw + cx0, cy1 * fw + cx1], dim=-1)
    return w, pix


def unpack_tabo(tabo):
    """(V, S, 2) int32 as the kernels write it (nw | ne << 16, sw | se << 16) -> (V, S, 4) int64 pixels"""
    t = tabo.long() & 0xFFFFFFFF
    return torch.stack([t[..., 0] & 0xFFFF, t[..., 0] >> 16, t[..., 1] & 0xFFFF, t[..., 1] >> 16], dim=-1)


def pack_tabo(pix):
    """(V, S, 4) int64 pixels (< 65536) -> (V, S, 2) int32"""
    lo = pix[..., 0] | (pix[..., 1] << 16)
    hi = pix[..., 2] | (pix[..., 3] << 16)
    t = torch.stack([lo, hi], dim=-1)
    return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)


def sample_table(x, w, pix, absolute=False):
    """x (V, C, hw), w (V, S, 4), pix (V, S, 4) int64 -> g (V, C, S) = sum_k x[.., pix_k] w_k in the order nw, ne, sw, se.
    ``absolute``: sum_k |x| |w| instead (the scale of the a-priori bounds)."""
    V, C, _ = x.shape
    out = None
    for k in range(4):
        tap = torch.gather(x, 2, pix[..., k][:, None, :].expand(V, C, -1))
        wk = w[..., k][:, None, :].to(x.dtype)
        term = tap.abs() * wk.abs() if absolute else tap * wk
        out = term if out is None else out + term
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the merge MLPs
class MergeWeights:
    """merge_net_feature.{0,1}.{0,2}: seeded, on `device`"""

    def __init__(self, C, seed, device="cpu"):
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        H = C // 2
        self.C = C
        self.w00, self.b00 = (rn(C, C) / math.sqrt(C)).to(device), (rn(C) * 0.1).to(device)
        self.w02, self.b02 = (rn(H, C) / math.sqrt(C)).to(device), (rn(H) * 0.1).to(device)
        self.w10, self.b10 = (rn(H, H) / math.sqrt(H)).to(device), (rn(H) * 0.1).to(device)
        self.w12, self.b12 = (rn(C, H) / math.sqrt(H)).to(device), (rn(C) * 0.1).to(device)

    def oracle_dict(self, dtype=torch.float64):
        return {f"merge_net_feature.{i}.{j}.{k}": getattr(self, f"{k[0]}{i}{j}").to(dtype)
                for i in (0, 1) for j in (0, 2) for k in ("weight", "bias")}


def mm(x, w, fp32):
    """x w^T: fp64, or fp32 summed k-sequentially in steps of 4 as the MFMA chains sum it (a BLAS-ordered sum is more accurate at
    K = 512 and would measure the summation order instead of the kernel)"""
    if not fp32:
        return x.double() @ w.double().T
    x, wt = x.float(), w.float().T.contiguous()
    out = torch.zeros(x.shape[0], w.shape[0], device=x.device)
    for k in range(0, x.shape[1], 4):
        out += x[:, k:k + 4] @ wt[k:k + 4]
    return out


def mlp0(rows, W, fp32=False):
    dt = torch.float32 if fp32 else torch.float64
    return mm(F.relu(mm(rows, W.w00, fp32) + W.b00.to(dt)), W.w02, fp32) + W.b02.to(dt)


def mlp1(m, W, fp32=False):
    dt = torch.float32 if fp32 else torch.float64
    return mm(F.relu(mm(m, W.w10, fp32) + W.b10.to(dt)), W.w12, fp32) + W.b12.to(dt)


def _tree_dot(a, b):
    """<a, b> over the last axis (HALF channels) in fp32, in the order merge.hip states above merge_tail_kernel: a 4-term chain
    per 4-channel chunk q; within a 32-channel tile, q % 8 = 2 g + hh: ((g0 + g1) + (g2 + g3)) per hh, then hh 0 + hh 1; the
    tiles pairwise"""
    p = (a * b).reshape(*a.shape[:-1], -1, 4, 2, 4)          # (tile, g, hh, e)
    c = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]     # (tile, g, hh)
    t = (c[..., 0, :] + c[..., 1, :]) + (c[..., 2, :] + c[..., 3, :])      # (tile, hh)
    t = t[..., 0] + t[..., 1]                                  # (tile)
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def reduce_views(h, fp32=False):
    """h (S, N, HALF) -> m (S, HALF): merge_features_mv's weighted sum (no softmax), or the master row itself for N = 1"""
    N = h.shape[1]
    if N == 1:
        return h[:, 0]
    if not fp32:
        wts = (h[:, 1:] * h[:, :1]).sum(-1, keepdim=True)
        return (wts * h[:, 1:]).sum(1)
    acc = torch.zeros_like(h[:, 0])
    for n in range(1, N):
        acc = acc + _tree_dot(h[:, n], h[:, 0])[:, None] * h[:, n]
    return acc


def stage_from_g(g, views, W, fp32=False):
    """g (V, C, S) sampled planes, views = [N_0, N_1, ...] -> dict(q1 (B, S, C), h2 (V S, C/2) row-major Q1 rows, m (B, S, C/2),
    out (B, S, C))"""
    dt = torch.float32 if fp32 else torch.float64
    V, C, S = g.shape
    rows = g.to(dt).reshape(V * S, C)
    h2 = mlp0(rows, W, fp32)
    q1, ms, outs, off = [], [], [], 0
    for N in views:
        q = rows[off * S:(off + N) * S].view(S, N, C)[:, 0]
        m = reduce_views(h2[off * S:(off + N) * S].view(S, N, C // 2), fp32)
        y = mlp1(m, W, fp32)
        q1.append(q)
        ms.append(m)
        outs.append(q + (y if N == 1 else y / N))
        off += N
    assert off == V
    return dict(q1=torch.stack(q1), h2=h2, m=torch.stack(ms), out=torch.stack(outs))


def stage_from_table(x, w, pix, views, W, fp32=False):
    """The stage from a given table (weights (V, S, 4) + pixels (V, S, 4)): x (V, C, hw) fp32 planes"""
    dt = torch.float32 if fp32 else torch.float64
    return stage_from_g(sample_table(x.to(dt), w.to(dt), pix), views, W, fp32)


def stage_from_coordinates(x, bps, centre, view_sample, intr, extr, fh, fw, img_w, img_h, views, W, fp32=False):
    """The stage from the cameras: x (V, C, fh fw) fp32 planes"""
    dt = torch.float32 if fp32 else torch.float64
    inv = torch.linalg.inv(extr.double()).float() if fp32 else None
    ix, iy = project_ixiy(bps, centre, view_sample, intr, extr, fh, fw, img_w, img_h, dtype=dt, inv=inv)
    w, pix = table_from_ixiy(ix, iy, fh, fw)
    return stage_from_table(x, w, pix, views, W, fp32)


# ---------------------------------------------------------------------------------------------------------------------
# rows of the fused kernels' buffers
def h2_row_major(v, c, seg, C, S):
    """Q1 row of (view v, channel c, segment seg): the C consecutive floats of plane (v, c) that start at point seg C"""
    return v * S + c * (S // C) + seg


def h2_tile_major(v, c, seg, C, S):
    """the same row in the tile-major layout: [(view * tiles_per_view + tile) * XS + row-in-tile], tile = (c / XS) NSEG + seg"""
    XS, NSEG = xs_of(C), S // C
    tpv = (C // XS) * NSEG
    return (v * tpv + (c // XS) * NSEG + seg) * XS + c % XS


def h2_permutation(V, C, S, device="cpu"):
    """perm (V S) int64 with h2_tiled[perm[R]] = h2_row_major[R]"""
    NSEG = S // C
    v = torch.arange(V, device=device)[:, None, None]
    c = torch.arange(C, device=device)[None, :, None]
    seg = torch.arange(NSEG, device=device)[None, None, :]
    R = h2_row_major(v, c, seg, C, S).reshape(-1)
    T = h2_tile_major(v, c, seg, C, S).expand(V, C, NSEG).reshape(-1)
    perm = torch.empty(V * S, dtype=torch.long, device=device)
    perm[R] = T
    return perm


def q1_row(b, off, N, v, c, seg, C, S):
    """row of q1 / out ((B S, C)) that Q1 row (v, c, seg) of sample b (first view off, N views) is the master row of, or -1"""
    r = (v - off) * S + c * (S // C) + seg
    return b * S + r // N if r % N == 0 else -1


def edge_points(N, C, S, device="cpu"):
    """(S,) bool: basis points of an N-view sample with a Q1 row in the first or the last tile of a view"""
    XS, NSEG = xs_of(C), S // C
    r = torch.arange(N * S, device=device)
    rem = r % S
    c, seg = rem // NSEG, rem % NSEG
    edge = ((c < XS) & (seg == 0)) | ((c >= C - XS) & (seg == NSEG - 1))
    return edge.view(S, N).any(1)


# ---------------------------------------------------------------------------------------------------------------------
# the launch arithmetic of merge.hip's launch_sample_merge_t / launch_sample_group_t / launch_merge_tail_t, mirrored
def launch_shape(kernel, C, S, views_cap, B, ncu):
    """-> (work items, items per view or sample, grid)"""
    XS, NSEG = xs_of(C), S // C
    if kernel == "sample_merge":
        step = (C // XS) * NSEG
        items = views_cap * step
    elif kernel == "sample_group":
        step = (C // XS) * (NSEG // 8)
        items = views_cap * step
    elif kernel == "merge_tail":
        step = S // 64
        items = B * step
    else:
        raise KeyError(kernel)
    return items, step, min(items, 2 * ncu)


def grid_cell(kernel, C, S, views_cap, B, ncu):
    """where the launch's work items stand against the persistent grid's limit of 2 ncu blocks: "below", "equal", "one_above"
    (one view / sample more than fills it: some blocks take a second trip) or "twice_plus" (a little above twice it: some a
    third), else None"""
    items, step, _ = launch_shape(kernel, C, S, views_cap, B, ncu)
    G = 2 * ncu
    if items < G:
        return "below"
    if items == G:
        return "equal"
    if items <= G + step:
        return "one_above"
    if 2 * G < items <= 2 * G + 4 * step:
        return "twice_plus"
    return None


CELLS = ("below", "equal", "one_above", "twice_plus")


def cell_counts(kernel, C, S, ncu):
    """{cell: number of views (sample_merge, sample_group) or samples (merge_tail) that reaches it}; "equal" only where the
    grid's limit is a whole number of views / samples"""
    _, step, _ = launch_shape(kernel, C, S, 1, 1, ncu)
    G = 2 * ncu
    out = {"below": max(1, G // step - 1) if G // step > 1 else None, "one_above": G // step + 1, "twice_plus": 2 * G // step + 1}
    out["equal"] = G // step if G % step == 0 else None
    if out["below"] is None:
        del out["below"]
    if out["equal"] is None:
        del out["equal"]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# synthetic scenes
VIEW_KINDS = ("inside", "straddle", "behind", "clamp")


def make_points(S, seed, radius=0.1):
    """S points in a ball of `radius` (the basis point set's role)"""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(S, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    return (d * radius * torch.rand(S, 1, generator=g) ** (1.0 / 3.0)).float()


def make_cameras(kinds, img_w, img_h, seed, depth=0.6):
    """One camera per entry of `kinds`, looking at the origin from `depth` with a small random rotation -> intr (V, 3, 3), extr
    (V, 4, 4) camera -> master, fp32.  "inside": the ball of points projects inside the image; "straddle": a focal length of
    four image widths, so that the projections cross every border; "behind": the camera looks away (negative depths);
    "clamp": the third row of K is zero, so that q_z = 0 exactly and the |z| < 1e-7 clamp decides."""
    g = torch.Generator().manual_seed(seed)
    V = len(kinds)
    intr = torch.zeros(V, 3, 3, dtype=torch.float64)
    extr = torch.zeros(V, 4, 4, dtype=torch.float64)
    for v, kind in enumerate(kinds):
        assert kind in VIEW_KINDS, kind
        a = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.3
        th = float(a.norm())
        k = a / th
        Kx = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
        R = torch.eye(3, dtype=torch.float64) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)
        d = -depth if kind == "behind" else depth
        f = 4.0 if kind == "straddle" else 1.5
        off = (torch.rand(2, generator=g, dtype=torch.float64) - 0.5) * 0.1
        intr[v] = torch.tensor([[f * img_w, 0, img_w * (0.5 + float(off[0]))], [0, f * img_h, img_h * (0.5 + float(off[1]))],
                                [0, 0, 0 if kind == "clamp" else 1]], dtype=torch.float64)
        extr[v, :3, :3] = R                                   # p_master = R p_cam + t, t = -R (0, 0, d): p_cam = R^T p_master + (0, 0, d)
        extr[v, :3, 3] = -(R @ torch.tensor([0, 0, d], dtype=torch.float64))
        extr[v, 3, 3] = 1
    return intr.float(), extr.float()
