"""Plain-Python side of tests/test_gemm_forms.py: the fragment-image index maps, the launcher's dispatch arithmetic mirrored
from csrc/gemm.hip, and the fp64 / fp32 restatements of the operations.  Nothing here touches the GPU; tests/test_host_logic.py
checks these pieces on the CPU (maps are bijections, the mirror on the release shapes, the restatements against torch)."""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------------
# index maps: float offset inside the image of element (row, col), restated from the layout comments of gemm.hip / attn.hip
def pa_index(rows, cols):
    """Packed-activation order = K image: float4 ((mt * cols/8 + kc) * 64 + lane) holds row 32 mt + (lane & 31), columns
    8 kc + 4 (lane >> 5) .. +3.  -> (rows, cols) int64 offsets (in floats)."""
    assert cols % 8 == 0
    r, c = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    lane = (r % 32) + 32 * ((c % 8) // 4)
    return (((r // 32) * (cols // 8) + c // 8) * 64 + lane) * 4 + c % 4


k_image_index = pa_index


def v_image_index(rows, cols):
    """V image: float4 (((mt * cols/32 + vt) * 4 + g) * 64 + lane) holds column 32 vt + (lane & 31), rows
    32 mt + 8 g + 4 (lane >> 5) .. +3."""
    assert cols % 32 == 0
    r, c = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    rr = r % 32
    lane = (c % 32) + 32 * ((rr % 8) // 4)
    return ((((r // 32) * (cols // 32) + c // 32) * 4 + rr // 8) * 64 + lane) * 4 + rr % 4


def image_floats(rows, cols):
    return (rows + 31) // 32 * 32 * cols


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's choice (gemm.hip: launch_gemm_split_impl, launch_panel_t, launch_gemm_kslab, poem_launch_gemm2)
def gemm2_branch(M, N):
    """(MT, NT) of poem_launch_gemm2"""
    ntiles, mtiles = (N + 31) // 32, (M + 31) // 32
    if ntiles % 4 == 0:
        return (2, 4) if (mtiles + 1) // 2 * (ntiles // 4) >= 768 else (1, 2)
    return (1, 2) if ntiles % 2 == 0 else (1, 1)


def dispatch(M, N, K, ncu, act=0, act_split=None, act2=None, seg_cols=0, ldx=None, narrow=True, kslab=True, xcd=True):
    """The kernel a poem_launch_gemm / _split / _segs call runs on a device of `ncu` CUs, as a tuple:
    ("panel", NT, MT, gelu, xcd_map) | ("kslab", MT) | ("gemm2", MT, NT) | ("refuse",)"""
    act_split = N if act_split is None else act_split
    act2 = act if act2 is None else act2
    ldx = K if ldx is None else ldx
    seg = seg_cols > 0
    two_acts = act_split < N and act2 != act
    row_tiles = (M + 31) // 32
    NT = 0
    for c in (4, 2, 1):
        if N % (32 * c) == 0 and c * K * 128 <= 128 * 1024 and (act_split >= N or act_split % (32 * c) == 0) and \
                (not seg or seg_cols % (32 * c) == 0):
            NT = c
            if row_tiles * (N // (32 * c)) >= 8 * ncu or not narrow or K > 256:
                break
    slab_ok = K >= 512 and K % 128 == 0 and N % 64 == 0 and (act_split >= N or act_split % 64 == 0) and ldx % 4 == 0 and \
        M * ldx * 4 < (1 << 32) and M >= 512
    if NT <= 1 and kslab and slab_ok and (not seg or (seg_cols % 64 == 0 and M % 32 == 0)):
        return ("kslab", 2 if (row_tiles + 15) // 16 * (N // 64) >= 2 * ncu else 1)
    if not seg and NT == 1 and N >= 64 and K >= 512 and not two_acts:
        NT = 0
    if NT == 0 or K % 8 or ldx % 4 or M * ldx * 4 >= (1 << 32):
        if seg or two_acts:
            return ("refuse",)
        return ("gemm2",) + gemm2_branch(M, N)
    panels = N // (32 * NT)
    wpp = max(1, max(ncu, panels) // panels) * 8
    cost = lambda mt: ((row_tiles + mt - 1) // mt + wpp - 1) // wpp * mt      # noqa: E731
    MT = 2 if 5 * cost(2) <= 6 * cost(1) else 1
    gelu = act == 2 or (act_split < N and act2 == 2)
    if seg and gelu:
        return ("refuse",)
    grid = max(ncu, panels)
    xm = bool(xcd and grid % 8 == 0 and (grid // 8) % panels == 0 and row_tiles >= 8 * ((grid // 8) // panels) * 8 * MT)
    return ("panel", NT, MT, gelu, xm)


def panel_passes(M, N, branch, ncu):
    """how often the slowest wave of a panel launch runs its row-group loop (rg += blocks_in_panel * 8)"""
    _, NT, MT, _, xm = branch
    panels = N // (32 * NT)
    grid = max(ncu, panels)
    rgroups = ((M + 31) // 32 + MT - 1) // MT
    if xm:
        bip, rgroups = (grid // 8) // panels, (rgroups + 7) // 8
    else:
        bip = (grid + panels - 1) // panels
    return (rgroups + bip * 8 - 1) // (bip * 8)


# ---------------------------------------------------------------------------------------------------------------------
# restatements (CPU).  fp64: the operation in float64 from the fp32 inputs.  fp32: the same with the k-sum as the kernel takes it.
def relu_nan(t):
    """v < 0 ? 0 : v -- a NaN stays a NaN"""
    return torch.where(t < 0, torch.zeros_like(t), t)


def activation(t, act):
    return t if act == ACT_NONE else (relu_nan(t) if act == ACT_RELU else F.gelu(t))      # (F.gelu: the erf form)


def linear_seq(x, w, kc=2):
    """x w^T in fp32 as one running fp32 sum over k in steps of 2 (the k-depth of the fp32 MFMA); see test_attention_forms"""
    wt = w.T.contiguous()
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k0 in range(0, w.shape[1], kc):
        acc.addmm_(x[:, k0:k0 + kc], wt[k0:k0 + kc])
    return acc


def gemm_ref(x, w, b=None, r=None, act=0, act_split=None, act2=None, fp32=False):
    """act(x w^T + b) + r, columns >= act_split with act2"""
    N = w.shape[0]
    if fp32:
        y = linear_seq(x.float(), w.float())
        cv = lambda t: t.float()      # noqa: E731
    else:
        y = x.double() @ w.double().T
        cv = lambda t: t.double()      # noqa: E731
    if b is not None:
        y = y + cv(b)
    if act_split is None or act_split >= N:
        y = activation(y, act)
    else:
        y = torch.cat([activation(y[:, :act_split], act), activation(y[:, act_split:], act2)], dim=1)
    return y if r is None else y + cv(r)


def _lane_reduce(t):
    """sum over the last dim in the kernels' order: lane l of a wave adds elements l, l + 64, .. one after the other, then a
    butterfly over the 64 lanes (xor 32, 16, .. 1).  (The order only: where a kernel fuses multiply and add, this adds rounded terms.)"""
    rows, n = t.shape
    pad = (-n) % 64
    if pad:
        t = torch.cat([t, torch.zeros(rows, pad, dtype=t.dtype)], dim=1)
    t = t.view(rows, -1, 64)
    s = torch.zeros(rows, 64, dtype=t.dtype)
    for j in range(t.shape[1]):
        s = s + t[:, j]
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, :1]


def layernorm_ref(x, g, b, eps, fp32=False):
    """two-pass LayerNorm (mean, biased variance of the differences, eps inside the root)"""
    if not fp32:
        x, g, b = x.double(), g.double(), b.double()
        mean = x.mean(-1, keepdim=True)
        d = x - mean
        return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * g + b
    cols = x.shape[1]
    mean = _lane_reduce(x) / cols
    d = x - mean
    rstd = 1.0 / torch.sqrt(_lane_reduce(d * d) / cols + torch.tensor(eps, dtype=torch.float32))
    return d * rstd * g + b


def narrow_ref(x, w, b=None, base=None, fp32=False):
    """base + (x w^T + b), one output column after the other.  fp32: the kernel's lane-strided order and butterfly, but each
    product is rounded before it is added, where the kernel's fmaf rounds once -- the same order, not the same bits."""
    if not fp32:
        y = x.double() @ w.double().T
        if b is not None:
            y = y + b.double()
        return y if base is None else base.double() + y
    cols = []
    for n in range(w.shape[0]):
        s = _lane_reduce(x * w[n])
        cols.append(s + b[n] if b is not None else s)
    y = torch.cat(cols, dim=1)
    return y if base is None else base + y
