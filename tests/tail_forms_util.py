"""The parametric tail and the glue kernels (csrc/misc.hip, csrc/mano.hip) restated once on the CPU, for tests/test_tail_forms.py:
float64 where the kernel rounds, fp32 torch / numpy where it claims the reference's own roundings, integers and bit patterns where
it only moves data.

  q3_flatten        rows = feats.reshape(-1, Q); rows @ w + b and the term sum of its bound                     q3_ref
  rot6d_to_aa       the ladder (axis x angle x row scale x shear), the fp64 Gram-Schmidt matrix of the fp32 six numbers, the
                    error of an axis-angle as a rotation, the candidate pattern of the fp32 chain              rot6d_ladder ...
  finalize          nan_to_num(x) * r + c in fp32 torch (two roundings); the MANO rows nan_to_num(joints | verts) + c
  compose           A B and A b1 + b2 in fp64 with the term sums of their bound                                compose_ref
  gather / pad / broadcast / canon_xyz   numpy indexing on bit patterns; numpy's fp32 division
  view_layout       repeat / arange / n (n - 1) / 2 + k                                                        view_layout_ref
  mano table        the layout of mano.hip's header from the five asset arrays, and LBS evaluated from that table in fp64
                    (mano_table, lbs_from_table)"""
import math

import numpy as np
import torch

import mano_oracle as mo
import poem_oracle as po

U32 = 2.0 ** -24            # unit round-off of fp32
U64 = 2.0 ** -53
FLT_MAX = 3.4028234663852886e38


# ---------------------------------------------------------------------------------------------------------------------
# q3_flatten
def q3_ref(feats, w, b):
    """feats (B, Q, C), w (Q,), b (1,) fp32 -> (t (B, C) fp64, T (B, C) = sum_m |x_m w_m| + |b|)"""
    B, Q, C = feats.shape
    rows = feats.double().reshape(-1, Q)
    t = rows @ w.double() + b.double()
    T = rows.abs() @ w.double().abs() + b.double().abs()
    return t.reshape(B, C), T.reshape(B, C)


def q3_bound(Q, T):
    """a lane chain of ceil(Q / 64) fused steps, six butterfly adds, one bias add; 1.01 for the second-order terms"""
    return 1.01 * (math.ceil(Q / 64) + 7) * U32 * T


# ---------------------------------------------------------------------------------------------------------------------
# rot6d -> axis-angle
ANGLES = (0.0, 1e-7, 1e-6, 1e-4, 9e-4, 0.3, 1.0, math.pi / 2, 2 * math.pi / 3, 2.0, 3.0, math.pi - 9e-4, math.pi - 1e-4,
          math.pi - 1e-6, math.pi)
SCALES = (2.0 ** -20, 1.0, 2.0 ** 20)
SHEARS = (0.0, 0.7, 30.0)


def ladder_axes():
    g = torch.Generator().manual_seed(0)
    rnd = torch.nn.functional.normalize(torch.randn(40, 3, generator=g, dtype=torch.float64), dim=-1)
    eye = torch.eye(3, dtype=torch.float64)
    s3, s2 = 1 / math.sqrt(3.0), 1 / math.sqrt(2.0)
    special = torch.tensor([[s3, s3, s3], [-s3, s3, s3], [s2, s2, 0], [0, s2, s2], [s2, 0, -s2]], dtype=torch.float64)
    return torch.cat([rnd, eye, -eye, special])


def rot6d_ladder():
    """-> d6 (n, 6) fp32, rung (n,) int64, rungs [(angle, scale, shear)]: rung r holds every axis at that angle; the six numbers
    are the first two rows of the fp64 rotation, both scaled, the second plus shear x the first, rounded to fp32."""
    axes = ladder_axes()
    d6, rung, rungs = [], [], []
    for ang in ANGLES:
        R = mo.rodrigues(axes * ang)
        for sc in SCALES:
            for mix in SHEARS:
                d6.append(torch.cat([R[:, 0] * sc, (R[:, 1] + mix * R[:, 0]) * sc], -1))
                rung.append(torch.full((len(axes),), len(rungs), dtype=torch.int64))
                rungs.append((ang, sc, mix))
    return torch.cat(d6).float(), torch.cat(rung), rungs


def gram_schmidt64(d6):
    """the rotation the fp32 six numbers define, in fp64 (rows b1, b2, b3)"""
    d = d6.double()
    a1, a2 = d[..., :3], d[..., 3:]
    b1 = a1 / a1.norm(dim=-1, keepdim=True)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = b2 / b2.norm(dim=-1, keepdim=True)
    return torch.stack((b1, b2, torch.linalg.cross(b1, b2)), -2)


def rotation_error(aa, Rgs):
    """max entry difference between Rodrigues(aa) in fp64 and Rgs, per rotation"""
    return (mo.rodrigues(aa.double()) - Rgs).abs().amax(dim=(-1, -2))


def per_rung(err, rung, nrungs):
    out = torch.zeros(nrungs, dtype=torch.float64)
    return out.scatter_reduce(0, rung, err, "amax", include_self=True)


def rot6d_yardstick(d6, rung, nrungs):
    """the oracle's own fp32 chain on the CPU: its worst rotation error on every rung"""
    aa = po.matrix_to_axis_angle(po.rotation_6d_to_matrix(d6))
    assert aa.dtype == torch.float32
    return per_rung(rotation_error(aa, gram_schmidt64(d6)), rung, nrungs)


def rot6d_bars(yard, rungs):
    """4 x the yardstick + one ulp of a unit entry; for shear <= 0.7 never past the 2e-6 tests/test_mano.py has always asked"""
    bar = 4 * yard + 2.0 ** -23
    tame = torch.tensor([mix <= 0.7 for _, _, mix in rungs])
    return torch.where(tame, bar.clamp(max=2e-6), bar)


def q_abs32(d6):
    """the four candidates' sqrt(max(., 0)) of the fp32 chain (oracle's Gram-Schmidt), (n, 4) fp32"""
    m = po.rotation_6d_to_matrix(d6)
    tr = torch.stack([1 + m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2], 1 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2],
                      1 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2], 1 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]], -1)
    return torch.sqrt(tr.clamp(min=0))


# ---------------------------------------------------------------------------------------------------------------------
# finalize, finalize_param, param_rows
def finalize_ref(xyz, centre, radius):
    """xyz (L, B, Q, 3), centre (B, 3) fp32 -> nan_to_num(xyz) * radius + centre: fp32 torch, a product and a sum, each rounded"""
    r = torch.tensor(radius, dtype=torch.float32)
    return torch.nan_to_num(xyz) * r + centre[None, :, None, :]


def param_rows_ref(verts, joints):
    """(B, Q - 21, 3), (B, 21, 3) -> (B, Q, 3): joints then vertices, as they are"""
    return torch.cat([joints, verts], 1)


def finalize_mano_ref(verts, joints, centre):
    return torch.nan_to_num(param_rows_ref(verts, joints)) + centre[:, None, :]


def seed_specials(t, seed, frac=0.02):
    """t with NaN, +-Inf, -0 and denormals written over a seeded selection of its elements (in place) -> t"""
    g = torch.Generator().manual_seed(seed)
    flat = t.view(-1)
    n = flat.numel()
    k = max(6, int(n * frac))
    pos = torch.randperm(n, generator=g)[:min(k, n)]
    vals = torch.tensor([0x7FC00000, 0x7F800000, 0xFF800000 - (1 << 32), 0x80000000 - (1 << 32), 0x00000001, 0x807FFFFF - (1 << 32),
                         0x7FC12345, 0x00400000], dtype=torch.int64).to(torch.int32).view(torch.float32)
    flat[pos] = vals[torch.arange(len(pos)) % len(vals)]
    return t


# ---------------------------------------------------------------------------------------------------------------------
# composite Linears
def compose_ref(A, Bm, b1, b2):
    """A (N, Cm), Bm (Cm, K), b1 (Cm,), b2 (N,) or None -> W, TW, b, Tb: fp64 products and the sums of the terms' magnitudes"""
    A64, B64 = A.double().numpy(), Bm.double().numpy()
    W, TW = A64 @ B64, np.abs(A64) @ np.abs(B64)
    b, Tb = A64 @ b1.double().numpy(), np.abs(A64) @ np.abs(b1.double().numpy())
    if b2 is not None:
        b, Tb = b + b2.double().numpy(), Tb + np.abs(b2.double().numpy())
    return W, TW, b, Tb


def compose_bound(ref, T, Cm):
    """one fp32 rounding of an fp64 sum in any order, fused or not: the products of fp32 factors are exact in fp64, and a sum of
    Cm of them -- or of Cm and b2 -- takes at most Cm roundings"""
    return U32 * np.abs(ref) + Cm * U64 * T


# ---------------------------------------------------------------------------------------------------------------------
# view_layout
def view_layout_ref(views):
    v = np.asarray(views, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(v)])
    view_sample = np.repeat(np.arange(len(v)), v)
    k = np.arange(offs[-1]) - offs[view_sample]
    n = v[view_sample]
    return offs.astype(np.int32), view_sample.astype(np.int32), (n * (n - 1) // 2 + k).astype(np.int32)


LAYOUT_MAX_BATCH = 1663      # csrc/merge.h POEM_LAYOUT_MAX_BATCH
LAYOUT_BATCHES = {
    "one": [1],
    "sample_limit": [1] * LAYOUT_MAX_BATCH,
    "mixed": [1, 3, 2, 5, 4, 6, 8, 7, 9, 10],
    "both_limits": [40] * 678 + [39] * 985,          # 1663 samples, 65535 views
    "one_of_64": [64],
}


# ---------------------------------------------------------------------------------------------------------------------
# the MANO table (mano.hip's header)
NV, NJ, NPOSE, NBETA, VP, K4 = 778, 16, 135, 10, 832, 37
OFF_VT = 0
OFF_D = OFF_VT + 3 * VP
OFF_W = OFF_D + K4 * 3 * VP * 4
OFF_JT = OFF_W + NJ * VP
OFF_JSD = OFF_JT + 48
TABLE_FLOATS = OFF_JSD + 48 * NBETA


def mano_table(assets):
    """-> dict: vt (3, VP), D (K4, 3, VP, 4), W (NJ, VP) fp32, exactly the asset values and zeros; JT (48,), JSD (48, 10) fp64 with
    TJT, TJSD the sums of the magnitudes of their 778 terms."""
    vt = np.zeros((3, VP), np.float32)
    vt[:, :NV] = assets["v_template"].T
    full = np.zeros((NV, 3, 4 * K4), np.float32)
    full[:, :, :NBETA] = assets["shapedirs"]
    full[:, :, NBETA:NBETA + NPOSE] = assets["posedirs"]
    D = np.zeros((K4, 3, VP, 4), np.float32)
    D[:, :, :NV, :] = full.reshape(NV, 3, K4, 4).transpose(2, 1, 0, 3)
    W = np.zeros((NJ, VP), np.float32)
    W[:, :NV] = assets["weights"].T
    jr, v64, sd = assets["J_regressor"].astype(np.float64), assets["v_template"].astype(np.float64), assets["shapedirs"].astype(np.float64)
    JT, TJT = (jr @ v64).reshape(48), (np.abs(jr) @ np.abs(v64)).reshape(48)
    JSD = np.einsum("jv,vck->jck", jr, sd).reshape(48, NBETA)
    TJSD = np.einsum("jv,vck->jck", np.abs(jr), np.abs(sd)).reshape(48, NBETA)
    return dict(vt=vt, D=D, W=W, JT=JT, TJT=TJT, JSD=JSD, TJSD=TJSD)


def table_flat32(tab):
    """the table as the kernel lays it out, the two composed regressions rounded once"""
    return np.concatenate([tab["vt"].ravel(), tab["D"].ravel(), tab["W"].ravel(), tab["JT"].astype(np.float32),
                           tab["JSD"].astype(np.float32).ravel()])


def lbs_from_table(tab, pose_aa, betas, center_idx):
    """LBS in fp64 read from the restated table the way mano_lbs_kernel reads it: coef = (betas | R_1..15 - I | 0 0 0),
    v_posed = vt + sum_k coef[k] D[k / 4][c][v][k % 4], J = JT + JSD betas, the chain, A, the joint-major weights."""
    dt = torch.float64
    B = pose_aa.shape[0]
    R = mo.rodrigues(pose_aa.to(dt).reshape(B, 16, 3))
    bet = betas.to(dt)
    coef = torch.cat([bet, (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(B, NPOSE), torch.zeros(B, 3, dtype=dt)], 1)
    Dk = torch.from_numpy(tab["D"]).to(dt).permute(0, 3, 1, 2).reshape(4 * K4, 3, VP)
    vp = torch.from_numpy(tab["vt"]).to(dt)[None] + torch.einsum("nk,kcv->ncv", coef, Dk)          # (B, 3, VP)
    J = (torch.from_numpy(tab["JT"])[None] + bet @ torch.from_numpy(tab["JSD"]).T).reshape(B, NJ, 3)
    GR, Gt = [None] * NJ, [None] * NJ
    for j in range(NJ):
        p = mo.PARENTS[j]
        if p < 0:
            GR[j], Gt[j] = R[:, 0], J[:, 0]
        else:
            GR[j] = GR[p] @ R[:, j]
            Gt[j] = torch.einsum("nrc,nc->nr", GR[p], J[:, j] - J[:, p]) + Gt[p]
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
    At = Gt - torch.einsum("njrc,njc->njr", GR, J)
    Wt = torch.from_numpy(tab["W"]).to(dt)
    TR, Tt = torch.einsum("jv,njrc->nvrc", Wt, GR), torch.einsum("jv,njr->nvr", Wt, At)
    verts = (torch.einsum("nvrc,ncv->nvr", TR, vp) + Tt)[:, :NV]
    j21 = torch.cat([Gt, verts[:, list(mo.TIPS)]], 1)[:, list(mo.ORDER)]
    if center_idx is not None and center_idx >= 0:
        c = j21[:, center_idx:center_idx + 1]
        verts, j21 = verts - c, j21 - c
    return verts, j21


def lbs_cases(seed=11):
    """33 (pose, betas): zero; joints 1..15 one at a time at 0.9 rad about a seeded axis (every one of the 135 pose-corrective
    coefficients the only large ones once); 0.6 randn; every joint at 3 rad and at 2 pi about seeded axes; betas randn, +5, -5 in
    turn (zero for the zero pose) -> pose (33, 48), betas (33, 10), names"""
    g = torch.Generator().manual_seed(seed)
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, 3, generator=g, dtype=torch.float64), dim=-1)      # noqa: E731
    poses, names = [torch.zeros(48, dtype=torch.float64)], ["zero"]
    for j in range(1, 16):
        p = torch.zeros(16, 3, dtype=torch.float64)
        p[j] = 0.9 * unit()
        poses.append(p.reshape(48))
        names.append(f"joint{j}@0.9")
    for i in range(9):
        poses.append(0.6 * torch.randn(48, generator=g, dtype=torch.float64))
        names.append(f"randn{i}")
    for ang, nm in ((3.0, "3rad"), (2 * math.pi, "2pi")):
        for i in range(4):
            poses.append((ang * unit(16)).reshape(48))
            names.append(f"{nm}_{i}")
    pose = torch.stack(poses).float()
    betas = torch.randn(len(poses), 10, generator=g)
    betas[0] = 0
    betas[1::3] = 5.0
    betas[2::3] = -5.0
    assert len(names) == 33
    return pose, betas, names


def lbs_bar(ref64, ref32):
    """per sample: 4 |fp32 oracle - fp64| + 2^-23 max|fp64| -> (B,)"""
    e32 = (ref32.double() - ref64).abs().flatten(1).amax(1)
    return 4 * e32 + 2.0 ** -23 * ref64.abs().flatten(1).amax(1), e32
