"""The row-tile chain kernels (chain.hip: 32- / 64-row tiles; chain16.hip: tiles of 1..4 units of 16 rows) in every form the
decoder launches them, called through poem_launch_chain and held against a float64 restatement of each chain kind as the
comment at the top of chain.hip states it:

  A   t = x Wo^T + bo + res ; h = LN(t) -> y1 ; [y2 = h W2^T + b2]        (x given, or combined from the cross attention's
                                                                            split-key partials: part_o / part_ml)
  C   f = x W^T + b + res -> y1 ; y2 = f W2^T + b2
  D1  f -> y1 ; u = relu(f Wreg0^T + b) ; xyz' = xyz + u Wreg2^T + b
  D2  o = sum_s gelu(f W_s^T + b_s) Wout_s^T ; g = LN(o + bout + f) -> y3 ; y2 = g W2^T + b2        (GELU: erf form)

with the decoder's LayerNorm eps of 1e-12.  Weights are packed with hip.pack_linear into one arena; at C = 128 / 256 the arena's
native 16x16x4 image sits behind it and native_delta is the distance, as in the engine's handle.

Bars.  End to end, per output and separately for rows 0..31 (the edge rows) and the others:
|HIP - fp64| <= 4 |fp32 - fp64| + 1e-6 max|fp64|, where fp32 is the same chain restated in fp32 on the GPU from the same fp32
inputs, its products summed k-sequentially in steps of 4 as the MFMAs sum them (a BLAS-ordered fp32 sum is much more accurate
at K = 4C = 2048, D2's second GEMM, and would measure the summation order instead of the kernel).  Stage-locally, every
trailing Linear y2 is held against fp64 of the KERNEL's own y1 / y3 rows within the a-priori bound of a K-term fp32 dot product,
2 (K + 2) 2^-24 (|y| |W2|^T + |b2|): about 3e-5 of the row's absolute products, where a wrong pass offset, bias or weight row
is off by O(1).  Bit for bit: every (M, tile_p) launch against the prefix of one canonical launch (chain.hip at 32-row tiles
over all rows) -- the kernels' claim that a row's result does not depend on the tile height or the batch; sentinels in the
unused columns and the guard rows of every output; kind A from the partials against kind A from the context that
attn_combine_kernel combines; a NaN input row against the clean launch.

Forms.  The launcher picks the kernel, tile height, units per tile (RU) and tiles per CU from M and the device's CU count
(poem_launch_chain / launch_chain16_k); _cells() mirrors that choice, and the M of every sweep -- 1, 15, 16, 17, 33, 65, 799,
1598 and 16 ncu r +- 1 for r = 1..8 -- is checked to reach every (C, kind, RU, tiles per CU, weight source) cell that the
launcher can pick: RU 1..4 at C = 128 / 256 (weight ring on native images for RU 1..2, tall gemm16 on native images for RU
3..4), RU 1..2 at C = 512 (plain gemm16), one and two tiles per CU, and chain.hip at P = 1 / 2.  The mirror's kernel choice
is probed against the launcher itself: with native_delta = 0, chain16 refuses a C = 128 / 256 launch and chain.hip does not.

Variants: kind A with n2 = 0 / 1 at ldy2 C, 1 / 3 at 3C, ldres C / 2C, res_mod = Q (block 0's shared query rows) at M = B Q;
kind A from partials of 1, 2, 3 and 4 key chunks (4 heads); kind C with n2 = 1; D1; D2 with n2 = 0 and 2 at 2C.  Inputs x and
res are column blocks of wider rows whose other columns hold NaN; outputs sit in wider rows.  Edge rows: a common offset of
1e3 with a spread of 1 before a LayerNorm (a one-pass variance fails there), a constant LayerNorm row (variance 0), rows of
magnitude ~1e-4 into D1's relu (with a quarter of its biases exactly 0), rows of magnitude ~30 and ~1e3 into D2's GELU."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from poem_v2_amd import hip
from util import ChainArgs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIP_INVALID_VALUE = 1          # hipErrorInvalidValue
EPS = 1e-12                    # the decoder's LayerNorm eps
Q = 799                        # queries per sample
HEADS = 4
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t

# launchers.h: launchers of libpoem_hip.so that the decoder calls (not part of the public ABI, so bound here)
_PROTOS = {
    "poem_launch_chain": (_i, [ctypes.POINTER(ChainArgs), _i, _vp]),
    "poem_launch_native16": (_i, [_vp, _vp, _sz, _vp]),
    "poem_device_cu_count": (_i, []),
    "poem_launch_cross_attention_imgq": (_i, [_vp, _i, _i] + [_vp] * 3 + [_i] * 5 + [_vp] * 2),
    "poem_cross_attention_scratch_floats": (_sz, [_i] * 6),
    "poem_cross_attention_partials": (None, [_i] * 5 + [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_i),
                                             ctypes.POINTER(ctypes.c_float)]),
    "poem_launch_gemm_segs": (_i, [_vp, _i, _vp, _vp] + [_i] * 5 + [_vp] * 3),
}
_FNS = {}


def _fn(name):
    if name not in _FNS:
        res, args = _PROTOS[name]
        _FNS[name] = ctypes.CFUNCTYPE(res, *args)((name, hip.lib()))
    return _FNS[name]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    assert not torch.backends.cuda.matmul.allow_tf32, "the fp32 restatement needs full-precision fp32 GEMMs"
    hip.lib()


@pytest.fixture(scope="module")
def ncu():
    n = _fn("poem_device_cu_count")()
    assert n > 0
    return n


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's choice, mirrored (chain.hip poem_launch_chain + chain_tile_p, chain16.hip launch_chain16_k + chain16_kernel)
KINDS = {"A": 0, "Ap": 0, "C": 1, "D1": 2, "D2": 3}


def _c16_shape(C, kind):
    maxru, nw = (2 if C == 512 else 4), (4 if C == 128 else 8)
    lds = ((2 if kind == 3 else 1) * C * (16 * maxru + 4) + 2 * nw * 16 * maxru) * 4
    return maxru, nw, lds


def _chain16_cells(M, C, label, ncu_dev):
    """(C, kind label, RU, tiles per CU (1, or 2 for two or more), weight source) of every tile of a chain16 launch."""
    kind = KINDS[label]
    maxru, nw, lds = _c16_shape(C, kind)
    U = (M + 15) // 16
    ncu = min(ncu_dev, U)
    per_cu = (U + ncu - 1) // ncu
    pair = 2 * lds <= 160 * 1024 and per_cu >= 3
    layers = max(2 if pair else 1, (per_cu + maxru - 1) // maxru)
    t16 = C // 16 // nw
    cells = set()
    for cu_n in {U // ncu, U // ncu + (1 if U % ncu else 0)}:      # the two shares: CUs below the remainder take one more unit
        tb, te = divmod(cu_n, layers)
        for layer in range(layers):
            ru = tb + (1 if layer < te else 0)
            if ru > 0:
                assert ru <= maxru
                src = "ring" if (ru * t16 <= 4 and t16 == 2) else ("native" if C in (128, 256) else "plain")
                cells.add((C, label, ru, min(layers, 2), src))
    return cells


def _uses_chain16(M, kind, tile_p, ncu):
    if tile_p == 3:
        return True
    if tile_p != 0:
        return False
    U = (M + 15) // 16
    per_cu = (U + min(ncu, U) - 1) // min(ncu, U)
    return per_cu <= 3 if kind == 3 else (per_cu >= 3 or per_cu == 1)


def _cells(M, C, label, tile_p, ncu):
    if _uses_chain16(M, KINDS[label], tile_p, ncu):
        return _chain16_cells(M, C, label, ncu)
    p = tile_p
    if p == 0:
        r2 = ((M + 63) // 64 + ncu - 1) // ncu * 64
        r1 = ((M + 31) // 32 + ncu - 1) // ncu * 32
        p = 1 if r1 < r2 else 2
    return {(C, label, "P%d" % (1 if C == 512 else p))}


def _every_cell(C, label, ncu):
    cells = {(C, label, "P1")} | (set() if C == 512 else {(C, label, "P2")})
    for U in range(1, 12 * ncu):
        cells |= _chain16_cells(16 * U, C, label, ncu)
    return cells


def _sweep_ms(ncu):
    return sorted(set([1, 15, 16, 17, 33, 65, 799, 1598] + [16 * ncu * r + d for r in range(1, 9) for d in (-1, 1)]))


def _tile_ps(C):
    return (0, 1, 3) if C == 512 else (0, 1, 2, 3)


def _rows_for(M):
    """rows of the inputs: whole samples of Q queries (the partials are per sample)"""
    return (M + Q - 1) // Q * Q


# ---------------------------------------------------------------------------------------------------------------------
# weights, inputs, references
def _q64(t):
    """values on a 1/64 grid: a bias b and 0.75 - b are then exact in fp32, so a constant row stays constant"""
    return torch.round(t * 64) / 64


class _Weights:
    def __init__(self, C, seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g, device=DEV)     # noqa: E731
        self.C = C
        self.w1, self.b1 = rn(C, C) / math.sqrt(C), _q64(rn(C) * 0.1)
        self.w2, self.b2 = rn(3 * C, C) / math.sqrt(C), _q64(rn(3 * C) * 0.1)
        self.wf4, self.bf4 = rn(5 * C, C) / math.sqrt(C), _q64(rn(5 * C) * 0.1)
        self.bf4[:C // 4] = 0.0                                          # relu inputs of ~0 on the near-zero rows
        self.wout, self.bout = rn(C, 4 * C) / math.sqrt(4 * C), _q64(rn(C) * 0.1)
        self.wreg2, self.breg2 = rn(3, C) / math.sqrt(C), rn(3) * 0.1
        self.ln_g, self.ln_b = 1 + 0.1 * rn(C), 0.1 * rn(C)
        self.ln2_g, self.ln2_b = 1 + 0.1 * rn(C), 0.1 * rn(C)
        packed = [hip.pack_linear(w) for w in (self.w1, self.w2, self.wf4, self.wout)]
        total = sum(p.numel() for p in packed)
        self.native = C in (128, 256)
        self.arena = torch.empty(2 * total if self.native else total, dtype=torch.uint8, device=DEV)
        self.ptr, off = [], 0
        for p in packed:
            self.arena[off:off + p.numel()].copy_(p)
            self.ptr.append(self.arena.data_ptr() + off)
            off += p.numel()
        self.native_delta = 0
        if self.native:
            rc = _fn("poem_launch_native16")(self.arena.data_ptr(), self.arena.data_ptr() + total, total, hip.stream())
            assert rc == 0, rc
            self.native_delta = total
        torch.cuda.synchronize()


def _inputs(C, W, rows, seed):
    """x (rows, C) and res (rows, C) with edge rows in 1..31; xyz (rows, 3)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(rows, C, generator=g, device=DEV)
    res = torch.randn(rows, C, generator=g, device=DEV)
    xyz = torch.randn(rows, 3, generator=g, device=DEV)
    res[1:5] += 1e3                                           # t = common offset 1e3 + spread ~1 (A, C, D1)
    x[5:8] += 1e3                                             # D2: f of offset 1e3 (GELU inputs ~1e3, LayerNorm offset)
    x[8], res[8] = 0.0, 0.75 - W.b1                           # t = 0.75 exactly in every channel: LN variance 0
    x[9:13] *= 1e-4                                           # f ~ 1e-4: D1's relu inputs around 0 (bf4[:C/4] = 0)
    res[9:13] = -W.b1 + 1e-4 * res[9:13]
    x[13:17] *= 30.0                                          # large GELU inputs (D2)
    x[17], res[17] = 0.0, -W.b1                               # f = 0 exactly
    return x, res, xyz


def _mm(x, w, fp32, acc=None):
    """x w^T: fp64, or fp32 summed k-sequentially in steps of 4 (continuing `acc`)"""
    if not fp32:
        r = x.double() @ w.double().T
        return r if acc is None else acc + r
    x, wt = x.float(), w.float().T.contiguous()
    out = torch.zeros(x.shape[0], w.shape[0], device=DEV) if acc is None else acc.clone()
    for k in range(0, x.shape[1], 4):
        out += x[:, k:k + 4] @ wt[k:k + 4]
    return out


def _ln(t, g, b):
    mean = t.mean(-1, keepdim=True)
    d = t - mean
    return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + EPS) * g.to(t.dtype) + b.to(t.dtype)


def _chain_ref(W, kind, x, res, xyz, n2, fp32):
    """The chain restated (fp64, or fp32 with k-sequential sums); res: the residual row of every output row"""
    C, dt = W.C, (torch.float32 if fp32 else torch.float64)
    cv = lambda t: t.to(dt)     # noqa: E731
    out = {}
    if kind != 3:
        t = _mm(x, W.w1, fp32) + cv(W.b1) + cv(res)
        if kind == 0:
            t = _ln(t, W.ln_g, W.ln_b)
        out["y1"] = t
        if kind == 2:
            u = F.relu(_mm(t, W.wf4[:C], fp32) + cv(W.bf4[:C]))
            out["xyz"] = cv(xyz) + (u @ cv(W.wreg2).T + cv(W.breg2))
            return out
        last = t
    else:
        o = None
        for s in range(4):
            h = F.gelu(_mm(x, W.wf4[C + s * C:C + (s + 1) * C], fp32) + cv(W.bf4[C + s * C:C + (s + 1) * C]))
            o = _mm(h, W.wout[:, s * C:(s + 1) * C], fp32, o)
        last = out["y3"] = _ln(o + cv(W.bout) + cv(x), W.ln2_g, W.ln2_b)
    if n2:
        out["y2"] = _mm(last, W.w2[:n2 * C], fp32) + cv(W.b2[:n2 * C])
    return out


def _assert_close(got, r64, r32, what):
    """|HIP - fp64| <= 4 |fp32 - fp64| + 1e-6 max|fp64| on the edge rows and on the other rows, each on its own"""
    for name, sel in (("rows 0..31", slice(0, 32)), ("rows 32..", slice(32, None))):
        g, a, b = got[sel].double(), r64[sel].double(), r32[sel].double()
        if g.shape[0] == 0:
            continue
        assert bool(torch.isfinite(g).all()), f"{what} {name}: non-finite output"
        e = float((g - a).abs().max())
        e32 = float((b - a).abs().max())
        bar = 4 * e32 + 1e-6 * float(a.abs().max())
        assert e <= bar, f"{what} {name}: |hip - fp64| = {e:.3e} > 4 |fp32 - fp64| + floor = {bar:.3e} (fp32: {e32:.3e})"


def _assert_linear(y, xin, w, b, what):
    """y = xin w^T + b of a K-term fp32 dot product per element, against fp64 of the same xin: within 2 (K + 2) 2^-24 of the
    absolute products"""
    xin, w, b = xin.double(), w.double(), b.double()
    ref = xin @ w.T + b
    bound = 2 * (w.shape[1] + 2) * 2.0 ** -24 * (xin.abs() @ w.abs().T + b.abs()) + 1e-30
    err = (y.double() - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, worst {float((err / bound).max()):.1f} x the bound"


# ---------------------------------------------------------------------------------------------------------------------
# launching
_CANARY = 0x7FC0DEAD      # a NaN bit pattern no kernel writes
_GUARD_ROWS = 64          # a whole tile: a store that skips its row guard lands here, inside the allocation


class _Out:
    """an output of `width` columns at column `col0` of rows of `ld` floats, plus guard rows, all holding the canary"""

    def __init__(self, M, ld, col0, width):
        self.M, self.ld, self.col0, self.width = M, ld, col0, width
        self.buf = torch.full((M + _GUARD_ROWS, ld), _CANARY, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.col0

    def take(self, what):
        """the output (M, width) as float32; asserts every other element still holds the canary"""
        rest = self.buf.clone()
        rest[:self.M, self.col0:self.col0 + self.width] = _CANARY
        assert bool((rest == _CANARY).all()), f"{what}: a write outside the output ({int((rest != _CANARY).sum())} elements)"
        return self.buf[:self.M, self.col0:self.col0 + self.width].view(torch.float32)


def _block(t, ld, col):
    """t (rows, C) as columns [col, col + C) of rows of `ld` floats; every other column is NaN -> (buffer, pointer)"""
    buf = torch.full((t.shape[0], ld), float("nan"), device=DEV)
    buf[:, col:col + t.shape[1]] = t
    return buf, buf.data_ptr() + 4 * col


class _Case:
    """one chain variant: kind, trailing Linear (n2 at row stride ldy2), residual (ldres, res_mod), input (x or partials)"""

    def __init__(self, W, label, x, res, xyz, n2, ldy2=None, ldres_c=2, res_mod=0, partials=None):
        C = W.C
        self.W, self.label, self.kind, self.n2 = W, label, KINDS[label], n2
        self.ldy2 = ldy2 or max(n2, 1) * C
        self.res_mod = res_mod
        self.x_rows = x                                    # fp32 (rows, C): the chain's input (the context for "Ap")
        self.xbuf, self.xp = _block(x, 2 * C, C)
        self.res_rows = res[:res_mod] if res_mod else res
        # res_mod > 0: rows past the shared copy are NaN, so a launch that ignores res_mod reads NaN (inside the allocation)
        rrows = torch.cat([self.res_rows, torch.full_like(res[res_mod:], float("nan"))]) if res_mod else res
        self.rbuf, self.rp = _block(rrows, ldres_c * C, 0)
        self.ldres = ldres_c * C
        self.xyz = xyz.contiguous()
        self.partials = partials

    def outputs(self, M):
        C, o = self.W.C, {}
        if self.kind == 3:
            o["y3"] = _Out(M, C + 64, 32, C)
        else:
            o["y1"] = _Out(M, C + 64, 32, C)
        if self.kind == 2:
            o["xyz"] = _Out(M, 3, 0, 3)
        elif self.n2:
            o["y2"] = _Out(M, self.ldy2, 0, self.n2 * C)
        return o

    def launch(self, M, tile_p, from_partials=None, native_delta=None, xp=None):
        W, a = self.W, ChainArgs()
        outs = self.outputs(M)
        a.kind, a.M, a.tile_p, a.eps = self.kind, M, tile_p, EPS
        a.x, a.ldx = (xp or self.xp), 2 * W.C
        use_p = self.partials is not None if from_partials is None else from_partials
        if use_p:
            p = self.partials
            a.x, a.part_o, a.part_ml = None, p["part_o"], p["part_ml"]
            a.pc_heads, a.pc_chunks, a.pc_nq, a.pc_kc2 = HEADS, p["chunks"], Q, p["kc2"]
        a.w1, a.b1 = W.ptr[0], W.b1.data_ptr()
        a.res, a.ldres, a.res_mod = self.rp, self.ldres, self.res_mod
        a.ln_g, a.ln_b = W.ln_g.data_ptr(), W.ln_b.data_ptr()
        a.w2, a.b2, a.n2 = W.ptr[1], W.b2.data_ptr(), self.n2
        a.wf4, a.bf4, a.wreg2, a.breg2 = W.ptr[2], W.bf4.data_ptr(), W.wreg2.data_ptr(), W.breg2.data_ptr()
        a.xyz_in = self.xyz.data_ptr()
        a.wout, a.bout, a.ln2_g, a.ln2_b = W.ptr[3], W.bout.data_ptr(), W.ln2_g.data_ptr(), W.ln2_b.data_ptr()
        for k, fld in (("y1", "y1"), ("y3", "y3")):
            if k in outs:
                setattr(a, fld, outs[k].ptr)
                setattr(a, "ld" + fld, outs[k].ld)
        if "y2" in outs:
            a.y2, a.ldy2 = outs["y2"].ptr, outs["y2"].ld
        if "xyz" in outs:
            a.xyz_out = outs["xyz"].ptr
        a.native_delta = W.native_delta if native_delta is None else native_delta
        rc = _fn("poem_launch_chain")(ctypes.byref(a), W.C, hip.stream())
        torch.cuda.synchronize()
        return rc, outs

    def run(self, M, tile_p, **kw):
        rc, outs = self.launch(M, tile_p, **kw)
        what = f"C={self.W.C} {self.label} M={M} tile_p={tile_p}"
        assert rc == 0, f"{what}: launch returned {rc}"
        return {k: o.take(f"{what} {k}") for k, o in outs.items()}

    def reference(self, M, fp32):
        res = self.res_rows[torch.arange(M, device=DEV) % self.res_mod] if self.res_mod else self.res_rows[:M]
        return _chain_ref(self.W, self.kind, self.x_rows[:M], res, self.xyz[:M], self.n2, fp32)

    def check_accuracy(self, got, M):
        what = f"C={self.W.C} {self.label} n2={self.n2} ldy2={self.ldy2} ldres={self.ldres} res_mod={self.res_mod}"
        r64, r32 = self.reference(M, False), self.reference(M, True)
        for k in got:
            _assert_close(got[k], r64[k], r32[k], f"{what} {k}")
        if "y2" in got:      # stage-local: the trailing Linear over the kernel's own rows
            src = got["y3" if self.kind == 3 else "y1"]
            _assert_linear(got["y2"], src, self.W.w2[:self.n2 * self.W.C], self.W.b2[:self.n2 * self.W.C], f"{what} y2 stage")


def _same_bits(got, canon, M, what):
    for k in got:
        a, b = got[k].contiguous().view(torch.int32), canon[k][:M].contiguous().view(torch.int32)
        if not torch.equal(a, b):
            rows = (a != b).any(-1).nonzero().flatten()
            pytest.fail(f"{what} {k}: {rows.numel()} rows differ from the canonical launch, first {rows[:8].tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
# the cross attention's split-key partials (attn.hip) for kind A
def _kv_images(k, v):
    """K / V fragment images written by the F1 GEMM's image modes (gemm.hip output modes 1 / 2) from an identity weight"""
    M, C = k.shape
    wp = hip.pack_linear(torch.eye(C, device=DEV))
    bias = torch.zeros(C, device=DEV)
    imgs = []
    for rows, mode in ((k, 1), (v, 2)):
        img = torch.empty(M * C, device=DEV)
        rc = _fn("poem_launch_gemm_segs")(rows.data_ptr(), C, wp.data_ptr(), bias.data_ptr(), M, C, 0, C, 1, (_vp * 1)(img.data_ptr()),
                                          (_i * 1)(mode), hip.stream())
        assert rc == 0, rc
        imgs.append(img)
    return imgs


def _partials(C, B, chunks, seed):
    """the cross attention (4 heads, 1024 keys per chunk) of B samples of Q queries: its partials and the context that its own
    combine kernel writes from them"""
    NK = 1024 * chunks
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(B * Q, C, generator=g, device=DEV) * 0.5
    k, v = torch.randn(B * NK, C, generator=g, device=DEV), torch.randn(B * NK, C, generator=g, device=DEV)
    kimg, vimg = _kv_images(k, v)
    del k, v
    # (a NaN tail past the partials: a fill that reads past its chunks reads NaN, inside the allocation)
    scratch = torch.full((_fn("poem_cross_attention_scratch_floats")(B, Q, NK, C, HEADS, 0) + (1 << 20),), float("nan"), device=DEV)
    ctx = torch.empty(B * Q, C, device=DEV)
    rc = _fn("poem_launch_cross_attention_imgq")(q.data_ptr(), C, Q, kimg.data_ptr(), vimg.data_ptr(), ctx.data_ptr(), B, Q, NK, C,
                                                 HEADS, scratch.data_ptr(), hip.stream())
    assert rc == 0, rc
    po, pml, nch, kc2 = _vp(), _vp(), _i(), ctypes.c_float()
    _fn("poem_cross_attention_partials")(B, Q, NK, C, HEADS, scratch.data_ptr(), ctypes.byref(po), ctypes.byref(pml), ctypes.byref(nch),
                                         ctypes.byref(kc2))
    torch.cuda.synchronize()
    assert nch.value == chunks, (nch.value, chunks)
    return ctx, dict(scratch=scratch, part_o=po.value, part_ml=pml.value, chunks=chunks, kc2=kc2.value)


# ---------------------------------------------------------------------------------------------------------------------
# per width: weights, inputs and the canonical launch of every main variant (shared by the tests of that width)
_STATE = {}


def _state(C, ncu):
    if C not in _STATE:
        W = _Weights(C, seed=C)
        ms = _sweep_ms(ncu)
        rows = _rows_for(ms[-1])
        x, res, xyz = _inputs(C, W, rows, seed=C + 1)
        ctx, part = _partials(C, rows // Q, 4, seed=C + 2)
        cases = {
            "A": _Case(W, "A", x, res, xyz, n2=1, ldres_c=2),
            "Ap": _Case(W, "Ap", ctx, res, xyz, n2=1, ldres_c=1, partials=part),
            "C": _Case(W, "C", x, res, xyz, n2=1, ldy2=2 * C, ldres_c=2),
            "D1": _Case(W, "D1", x, res, xyz, n2=0, ldres_c=1),
            "D2": _Case(W, "D2", x, res, xyz, n2=2, ldy2=2 * C),
        }
        _STATE[C] = dict(W=W, x=x, res=res, xyz=xyz, ms=ms, cases=cases, canon={})
    return _STATE[C]


@pytest.fixture(scope="module", autouse=True)
def _release_state():
    yield
    _STATE.clear()
    torch.cuda.empty_cache()


def _canonical(st, label):
    """chain.hip at 32-row tiles over every row of the sweep, checked against fp64 (Ap: fed the context, x = ctx)"""
    if label not in st["canon"]:
        case, M = st["cases"][label], st["ms"][-1]
        got = case.run(M, 1, from_partials=False)
        case.check_accuracy(got, M)
        st["canon"][label] = got
    return st["canon"][label]


WIDTHS = [128, 256, 512]


def test_sweep_reaches_every_form(ncu):
    """The sweep's (M, tile_p) launches reach every (C, kind, RU, tiles per CU, weight source) cell that the launcher can pick."""
    for C in WIDTHS:
        for label in KINDS:
            want = _every_cell(C, label, ncu)
            got = set()
            for M in _sweep_ms(ncu):
                for tp in _tile_ps(C):
                    got |= _cells(M, C, label, tp, ncu)
            assert want - got == set(), f"C={C} {label}: cells no sweep launch reaches: {sorted(want - got, key=str)}"
            rus = {c[2] for c in want if len(c) == 5}
            assert rus == ({1, 2} if C == 512 else {1, 2, 3, 4}), (C, label, rus)
            assert {c[3] for c in want if len(c) == 5} == {1, 2}, (C, label)
            srcs = {c[4] for c in want if len(c) == 5}
            assert srcs == ({"plain"} if C == 512 else {"ring", "native"}), (C, label, srcs)


@pytest.mark.parametrize("label", list(KINDS))
@pytest.mark.parametrize("C", WIDTHS)
def test_chain_forms_bit_identical_and_accurate(C, label, ncu):
    """Every sweep M at every tile_p: sentinels intact, bits equal to the canonical launch's first M rows (which passed the
    fp64 bar).  Ap: every launch combines the 4-chunk partials itself, the canonical one reads the combined context."""
    st = _state(C, ncu)
    canon, case = _canonical(st, label), st["cases"][label]
    for M in st["ms"]:
        for tp in _tile_ps(C):
            _same_bits(case.run(M, tp), canon, M, f"C={C} {label} M={M} tile_p={tp}")


@pytest.mark.parametrize("C", [128, 256])
def test_launcher_choice_matches_the_mirror(C, ncu):
    """native_delta = 0: chain16 refuses the launch (it reads native images at these widths) -- tile_p = 3 always, tile_p = 0
    exactly where the mirror picks chain16; chain.hip runs and matches the canonical bits.  A refused launch writes nothing."""
    st = _state(C, ncu)
    for label in ("A", "C", "D1", "D2"):
        case, canon = st["cases"][label], _canonical(st, label)
        for M in st["ms"]:
            for tp in (0, 3):
                rc, outs = case.launch(M, tp, native_delta=0)
                what = f"C={C} {label} M={M} tile_p={tp} native_delta=0"
                if _uses_chain16(M, case.kind, tp, ncu):
                    assert rc == HIP_INVALID_VALUE, f"{what}: returned {rc}"
                    for k, o in outs.items():
                        assert bool((o.buf == _CANARY).all()), f"{what}: refused launch wrote {k}"
                else:
                    assert rc == 0, f"{what}: returned {rc}"
                    _same_bits({k: o.take(what) for k, o in outs.items()}, canon, M, what)


_VARIANTS = {      # label: (kind label, n2, ldy2 in C, ldres in C, res_mod)
    "A_n0_mod": ("A", 0, 1, 1, Q),
    "A_n1_ldy2_3C": ("A", 1, 3, 1, 0),
    "A_n3_mod": ("A", 3, 3, 2, Q),
    "C_mod": ("C", 1, 1, 1, Q),
    "D1_mod": ("D1", 0, 1, 2, Q),
    "D2_n0": ("D2", 0, 1, 1, 0),
}


@pytest.mark.parametrize("variant", list(_VARIANTS))
@pytest.mark.parametrize("C", WIDTHS)
def test_chain_variants(C, variant, ncu):
    """Trailing passes n2 = 0 / 1 / 3 at row strides C / 3C, ldres C / 2C, res_mod = Q (one copy of the residual rows for every
    sample, M = B Q and ragged): fp64 bar at M = 5 Q, the other launches bit-identical to it."""
    st = _state(C, ncu)
    label, n2, ldy2, ldres, mod = _VARIANTS[variant]
    case = _Case(st["W"], label, st["x"], st["res"], st["xyz"], n2=n2, ldy2=ldy2 * C, ldres_c=ldres, res_mod=mod)
    M0 = 5 * Q
    canon = case.run(M0, 1)
    case.check_accuracy(canon, M0)
    for M in (1, 17, 2 * Q, 5 * Q - 13, 5 * Q):
        for tp in _tile_ps(C):
            _same_bits(case.run(M, tp), canon, M, f"C={C} {variant} M={M} tile_p={tp}")


@pytest.mark.parametrize("chunks", [1, 2, 3])
@pytest.mark.parametrize("C", WIDTHS)
def test_chain_from_partials_key_chunks(C, chunks, ncu):
    """Kind A fed from 1, 2 and 3 key chunks' partials (4 in the sweep): bit-identical to kind A fed the context that the
    attention's combine kernel writes, which passes the fp64 bar; ragged M included."""
    st = _state(C, ncu)
    B = 3
    ctx, part = _partials(C, B, chunks, seed=100 * C + chunks)
    case = _Case(st["W"], "Ap", ctx, st["res"], st["xyz"], n2=1, ldres_c=2, partials=part)
    M0 = B * Q
    canon = case.run(M0, 1, from_partials=False)
    case.check_accuracy(canon, M0)
    for M in (1, 33, Q, 2 * Q + 5, M0):
        for tp in _tile_ps(C):
            _same_bits(case.run(M, tp), canon, M, f"C={C} partials chunks={chunks} M={M} tile_p={tp}")


@pytest.mark.parametrize("label", ["A", "C", "D1", "D2"])
@pytest.mark.parametrize("C", WIDTHS)
def test_nan_row_stays_in_its_row(C, label, ncu):
    """A NaN in one input row (inside a tile; the last, ragged row): that row's outputs are all non-finite, every other row is
    bit-identical to the clean launch."""
    st = _state(C, ncu)
    case, canon = st["cases"][label], _canonical(st, label)
    for M in (Q, 16 * ncu * 6 + 1):
        bad = [40, M - 1]
        xbuf = case.xbuf.clone()
        xbuf[bad, C:] = float("nan")
        keep = torch.ones(M, dtype=torch.bool, device=DEV)
        keep[bad] = False
        for tp in _tile_ps(C):
            got = case.run(M, tp, xp=xbuf.data_ptr() + 4 * C)
            what = f"C={C} {label} M={M} tile_p={tp} NaN rows {bad}"
            for k, t in got.items():
                assert not bool(torch.isfinite(t[bad]).any()), f"{what} {k}: a NaN row has finite outputs"
                assert torch.equal(t[keep].view(torch.int32), canon[k][:M][keep].view(torch.int32)), f"{what} {k}: other rows changed"


@pytest.mark.parametrize("C", WIDTHS)
def test_layer_norm_edge_rows(C, ncu):
    """The edge rows' values: the LayerNorm of a constant row is beta exactly (kind A); the rows of offset 1e3 keep a spread of
    order 1 after it.  (Their accuracy is in the canonical launch's fp64 bar, edge rows on their own.)"""
    st = _state(C, ncu)
    W, canon = st["W"], _canonical(st, "A")
    assert torch.equal(canon["y1"][8], W.ln_b), "constant row: LayerNorm(t) != beta"
    assert float(canon["y1"][1:5].std()) > 0.5, "offset rows lost their spread"
    d1 = _canonical(st, "D1")
    assert torch.equal(d1["y1"][17], torch.zeros(C, device=DEV)), "f = 0 row"
