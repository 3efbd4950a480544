"""The GEMM family (csrc/gemm.hip) in every form the decoder and the C ABI launch it, each held against a float64 restatement:
the panel kernel, the K-slab kernel, the operands-from-L2 kernel (gemm2) with its packed-activation (PA) layouts, the segmented
outputs (attention K / V images), the narrow Linear and the LayerNorm.  The launchers that are not part of the public ABI are
bound here by ctypes, as in test_attention_forms.py / test_chain_forms.py.

Bar, per case: |HIP - fp64| <= 4 |fp32 - fp64| + 1e-6 max|fp64|.  fp64 is the operation in float64 from the same fp32 inputs; fp32
is the same case restated in fp32 on the CPU with the k-sum taken sequentially in steps of 2 (gemm_forms_util.linear_seq), for
the LayerNorm and the narrow Linear in the kernels' lane-strided order followed by the butterfly.  GELU is the erf form, ReLU
keeps a NaN.  Cases of more than 2^27 multiply-adds take the CPU restatements on the first 32, the last 64 and 96 spread rows,
and every row against float64 evaluated on the device, within the bar of the sampled rows; every element is also held bit for bit
-- against another form that the code promises to be bit-identical, and by the integer-valued variant (entries in -4..4, every
partial sum exact), which must equal x w^T (+ b, relu, + r) exactly.
Biases differ in every column, residuals are non-zero.  Row-major outputs sit in canary-filled wider rows with 64 guard rows
behind; X and R given as column blocks have NaN in the foreign columns; images have the canary behind them.

Coverage (form x branch x case; the branch of every case is computed from poem_device_cu_count() by the mirror of the launcher's
arithmetic in gemm_forms_util.dispatch and asserted, so a case never passes on another kernel than the one named here):

  launch_panel_t<NT, MT, GELU>     test_dispatch_branches, cases x act NONE / GELU (shapes for 256 CUs)
    <1,1>  M 799   N 256  K 256      (narrow off: <4,1>)        <1,2>  M 16389 N 128  K 32   (narrow off: <4,1>)
    <2,1>  M 100   N 192  K 512      (K > 256 keeps NT 2)       <2,2>  M 16389 N 256  K 32
    <4,1>  M 4133  N 4096 K 32       (xcd_map on, 8 uneven row ranges, ragged last tile)
    <4,2>  M 16389 N 512  K 32
    <1,1,GELU> / <2,1,GELU> / <4,1,GELU> beside pact == 1 panels: test_fused_two_activations C 32 / 64 / 256 (NT 2, 4 with
    poem_gemm_panel_narrow(0): the narrow-panel rule picks NT 1 for so few rows)
    two passes of the persistent row-group loop: test_strided_forms (M from the mirror, ragged last tile)
  OMODE 0 / 1 / 2                  test_segments: panel at C 32 (NT 1, one panel per segment) .. 256 and K 1024 at M < 512,
                                   K-slab <1> at C 1024, M 544 / 1056, <2> at M 2592; NT 2 / 4 with poem_gemm_panel_narrow(0);
                                   <4,2> at C 128, M 16416; xcd_map on with segments (4-segment launch) at C 32, M 32960
  gemm_kslab_kernel<1> / <2>       test_dispatch_branches M 517 N 64 K 1024 / M 8190 N 2048 K 640; test_strided_forms (b), C 256
  gemm2_kernel<MT,NT,IN_PA,OUT_PA> test_pa_chains: <1,1> and <1,2> in all four layout pairs (widths 128 / 64 / 96 rotated through
                                   RM -> PA -> PA -> RM); test_pa_big_branch: <2,4> in all four pairs, 191 (odd) and 192 row tiles;
                                   test_dispatch_branches: <1,1>, <1,2>, <2,4> as the launcher's fall-back, and every case through
                                   poem_launch_gemm2 against the default dispatch
  switches                         poem_gemm_panel_narrow / poem_gemm_xcd_map / poem_gemm_kslab 0 against 1, bit for bit, every case
  strides                          ldy 2C / 3C / 5C at column 0 and C; X = columns [C, 5C) of 5C-wide rows; ldr C, 3C
  refusals (hipErrorInvalidValue / POEM_E_ARG, nothing written): two activations on a gemm2-only shape, segments with GELU,
                                   seg_cols % 32, M % 32, nsegs 0 / 7; PA output with N % 32, layout flags 2 / -1, unaligned y
  narrow_linear_kernel             N 3 + base at ldx 5C, N 106 x 32 rows, N 8 with a NULL bias; K 32 .. 1024; npb = N at 8200 rows
  layernorm_kernel                 cols 32 .. 1024, rows 1 / 3 / 5 / 799, eps 1e-12 / 1e-5, rows of mean 100, a row over 6 decades

Out of scope: the split-precision (f16 hi / lo) variants are opt-in and need the thread-local arena context that poem_gemm_split
installs.  The in-place LayerNorm (y == x) is not a decoder form (decoder.cpp: p.att -> h_attn / h_cross, p.ffo -> feats) and is
left out."""
import ctypes
import math

import pytest
import torch

import gemm_forms_util as gu
from poem_v2_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIP_INVALID_VALUE = 1          # hipErrorInvalidValue
POEM_E_ARG = -1
NONE, RELU, GELU = 0, 1, 2
_vp, _i = ctypes.c_void_p, ctypes.c_int

# launchers.h: launchers of libpoem_hip.so that the decoder calls (not part of the public ABI, so bound here)
_PROTOS = {
    "poem_launch_gemm": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp] + [_i] * 5 + [_vp]),
    "poem_launch_gemm_split": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp] + [_i] * 7 + [_vp]),
    "poem_launch_gemm_segs": (_i, [_vp, _i, _vp, _vp] + [_i] * 5 + [_vp] * 3),
    "poem_launch_gemm2": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp] + [_i] * 7 + [_vp]),
    "poem_launch_narrow_linear": (_i, [_vp, _i] + [_vp] * 4 + [_i] * 3 + [_vp]),
    "poem_launch_layernorm": (_i, [_vp] * 4 + [_i, _i, ctypes.c_float, _vp]),
    "poem_gemm_kslab": (None, [_i]),
    "poem_gemm_panel_narrow": (None, [_i]),
    "poem_gemm_xcd_map": (None, [_i]),
    "poem_device_cu_count": (_i, []),
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
    hip.lib()


@pytest.fixture(scope="module")
def ncu():
    n = _fn("poem_device_cu_count")()
    assert n > 0
    return n


def _assert_close(got, ref64, ref32, what):
    got, ref64, ref32 = (t.double().cpu() for t in (got, ref64, ref32))
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    e = float((got - ref64).abs().max())
    e32 = float((ref32 - ref64).abs().max())
    bar = 4 * e32 + 1e-6 * float(ref64.abs().max())
    print(f"{what}: |hip - fp64| = {e:.3e}, |fp32 - fp64| = {e32:.3e}, bar {bar:.3e}")
    assert e <= bar, f"{what}: |hip - fp64| = {e:.3e} > 4 |fp32 - fp64| + floor = {bar:.3e} (fp32: {e32:.3e})"


# ---- buffers ----------------------------------------------------------------------------------------------------------
_CANARY = 0x7FC0DEAD      # a NaN bit pattern no kernel writes
_GUARD_ROWS = 64          # two tiles: a store that skips its row guard lands here, inside the allocation


class _Out:
    """an output of `width` columns at column `col0` of rows of `ld` floats, plus guard rows, all holding the canary"""

    def __init__(self, M, width, ld=None, col0=0):
        self.M, self.ld, self.col0, self.width = M, ld or width, col0, width
        self.buf = torch.full((M + _GUARD_ROWS, self.ld), _CANARY, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.col0

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == _CANARY).all())

    def take(self, what):
        """the output (M, width) as float32; asserts every other element still holds the canary"""
        torch.cuda.synchronize()
        rest = self.buf.clone()
        rest[:self.M, self.col0:self.col0 + self.width] = _CANARY
        assert bool((rest == _CANARY).all()), f"{what}: a write outside the output ({int((rest != _CANARY).sum())} elements)"
        return self.buf[:self.M, self.col0:self.col0 + self.width].view(torch.float32)


class _Image:
    """a fragment image (or PA buffer) of ceil(rows / 32) * 32 x cols floats with the canary in it and behind it"""

    def __init__(self, rows, cols):
        self.rows, self.cols, self.n = rows, cols, gu.image_floats(rows, cols)
        self.buf = torch.full((self.n + 4096,), _CANARY, dtype=torch.int32, device=DEV)

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def flat(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[self.n:] == _CANARY).all()), f"{what}: a write behind the image"
        return self.buf[:self.n].view(torch.float32)

    def decode(self, index, what):
        """(rows, cols) through an index map of gemm_forms_util"""
        return self.flat(what)[index(self.rows, self.cols).to(DEV)]


def _block(t, ld, col):
    """t (rows, C) as columns [col, col + C) of rows of `ld` floats; every other column is NaN -> (buffer, pointer)"""
    if ld == t.shape[1] and col == 0:
        t = t.contiguous()
        return t, t.data_ptr()
    buf = torch.full((t.shape[0], ld), float("nan"), device=DEV)
    buf[:, col:col + t.shape[1]] = t
    return buf, buf.data_ptr() + 4 * col


def _bits_equal(a, b, what):
    a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        pytest.fail(f"{what}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}")


def _exact(got, ref, what):
    """equal as numbers, element for element (the integer-valued variants; +0 and -0 are the same number)"""
    ok = got == ref.to(got.device)
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        pytest.fail(f"{what}: {bad.shape[0]} elements differ, first at {bad[0].tolist()}")


# ---- inputs -----------------------------------------------------------------------------------------------------------
class _Data:
    """x (M, K), w (N, K) = randn / sqrt(K), a bias that differs in every column, a non-zero residual; integer=True: entries in
    -4..4 (bias: distinct integers), so that every partial sum is exact in fp32.  CPU tensors and device copies."""

    def __init__(self, M, N, K, seed, integer=False):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.integer = M, N, K, integer
        if integer:
            ri = lambda *s: torch.randint(-4, 5, s, generator=g).float()      # noqa: E731
            self.x, self.w, self.r = ri(M, K), ri(N, K), ri(M, N)
            self.b = (torch.arange(N) - N // 2).float()
        else:
            self.x, self.w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
            self.r = torch.randn(M, N, generator=g)
            self.b = (torch.arange(N) % 61 - 30).float() / 16 + torch.arange(N).float() / 4096 + 0.01 * torch.randn(N, generator=g)
        self.xd, self.wd, self.bd, self.rd = (t.to(DEV) for t in (self.x, self.w, self.b, self.r))
        self.wp = hip.pack_linear(self.wd)

    def first(self, M):
        """the same data restricted to its first M rows"""
        s = _Data.__new__(_Data)
        s.__dict__.update(self.__dict__, M=M, x=self.x[:M], xd=self.xd[:M], r=self.r[:M], rd=self.rd[:M])
        return s

    def rows(self):
        """the rows of the two CPU restatements: all, or (above 2^27 multiply-adds) the first 32, the last 64 and 96 spread rows"""
        M = self.M
        if M * self.N * self.K <= 1 << 27:
            return torch.arange(M)
        return torch.unique(torch.cat([torch.arange(32), torch.arange(M - 64, M), torch.linspace(0, M - 1, 96).round().long()]))

    def check(self, got, what, bias=True, res=True, act=NONE, act_split=None, act2=None):
        """got (M, N) against the restatements; the integer variant exactly (GELU columns: against the bar)"""
        kw = dict(act=act, act_split=act_split, act2=act2)
        if self.integer:
            ref = gu.gemm_ref(self.xd, self.wd, self.bd if bias else None, self.rd if res else None, **kw).float()      # (exact)
            exact = torch.ones(self.N, dtype=torch.bool, device=DEV)
            if act == GELU:
                exact[:self.N if act_split is None else act_split] = False
            if act2 == GELU and act_split is not None:
                exact[act_split:] = False
            _exact(got[:, exact], ref[:, exact], f"{what} (integer-valued: must be exact)")
            if bool(exact.all()):
                return
        sel = self.rows()
        b, r = (self.b if bias else None), (self.r[sel] if res else None)
        r64 = gu.gemm_ref(self.x[sel], self.w, b, r, **kw)
        r32 = gu.gemm_ref(self.x[sel], self.w, b, r, fp32=True, **kw)
        _assert_close(got[sel.to(DEV)], r64, r32, what)
        if sel.numel() < self.M:
            # every row against float64 evaluated on the device; the bar is the one of the sampled rows (fp32's own error there)
            all64 = gu.gemm_ref(self.xd, self.wd, self.bd if bias else None, self.rd if res else None, **kw)
            assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
            e = float((got.double() - all64).abs().max())
            bar = 4 * float((r32.double() - r64).abs().max()) + 1e-6 * float(r64.abs().max())
            print(f"{what}, all rows: |hip - fp64| = {e:.3e}, bar {bar:.3e}")
            assert e <= bar, f"{what}: over all rows |hip - fp64| = {e:.3e} > 4 |fp32 - fp64| + floor = {bar:.3e}"


def _gemm(d, act=NONE, bias=True, res=True, ldx=None, xcol=0, ldy=None, ycol=0, ldr=None, rcol=0, act_split=None, act2=None,
          gemm2=False, M=None, what="gemm"):
    """One launch over the first M rows of the data -> (rc, _Out).  X / R as column blocks of ldx / ldr-wide rows (NaN around)."""
    M = d.M if M is None else M
    xbuf, xp = _block(d.xd[:M], ldx or d.K, xcol)
    rbuf, rp = _block(d.rd[:M], ldr or d.N, rcol) if res else (None, None)
    out = _Out(M, d.N, ldy, ycol)
    head = (xp, ldx or d.K, d.wp.data_ptr(), d.bd.data_ptr() if bias else None, rp, (ldr or d.N) if res else 0, out.ptr, out.ld, M, d.N, d.K)
    if gemm2:
        rc = _fn("poem_launch_gemm2")(*head, act, 0, 0, hip.stream())
    elif act_split is None:
        rc = _fn("poem_launch_gemm")(*head, act, hip.stream())
    else:
        rc = _fn("poem_launch_gemm_split")(*head, act, act_split, act2, hip.stream())
    torch.cuda.synchronize()
    del xbuf, rbuf
    return rc, out


def _run(d, what, **kw):
    rc, out = _gemm(d, **kw)
    assert rc == 0, f"{what}: launch returned {rc}"
    return out.take(what)


class _switch:
    """an A/B switch of gemm.hip set for a block, restored to its default (on) afterwards"""

    def __init__(self, name, on):
        self.name, self.on = name, on

    def __enter__(self):
        _fn(self.name)(self.on)

    def __exit__(self, *exc):
        _fn(self.name)(1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. strided row-major forms through poem_launch_gemm
def _two_pass_m(N, K, ncu):
    """the smallest ragged M whose panel launch runs the persistent row-group loop twice"""
    for t in range(1, 1 << 14):
        M = 32 * t + 5
        br = gu.dispatch(M, N, K, ncu)
        if br[0] == "panel" and gu.panel_passes(M, N, br, ncu) >= 2:
            return M
    pytest.fail(f"N={N} K={K}: no M below 2^19 gives two passes of the row-group loop on {ncu} CUs")


@pytest.mark.parametrize("integer", [False, True], ids=["randn", "integer"])
@pytest.mark.parametrize("C", [32, 128, 256])
def test_strided_forms(C, integer, ncu):
    """(a) N = C into 2C / 3C / 5C-wide rows at column 0 and C; (b) X = columns [C, 5C) of 5C-wide rows, K = 4C, residual at
    ldr = C; (c) the residual from a 3C-wide buffer: the contiguous call holds the fp64 bar, the strided ones equal it bit for bit.
    M 1 / 31 / 33 / 799 and one M that sends every wave through the row-group loop twice."""
    m2 = _two_pass_m(C, C, ncu)
    da = _Data(m2, C, C, seed=C + integer, integer=integer)
    for M in (1, 31, 33, 799, m2):
        for act in ((NONE, RELU) if M in (33, m2) else (NONE,)):
            what = f"(a) C={C} M={M} act={act}"
            base = _run(da, what, M=M, act=act, res=False)
            if M != m2 or act == NONE:
                da.first(M).check(base, what, res=False, act=act)
            for ldy in (2 * C, 3 * C, 5 * C):
                for ycol in (0, C):
                    _bits_equal(_run(da, what, M=M, act=act, res=False, ldy=ldy, ycol=ycol), base, f"{what} ldy={ldy} col={ycol}")
    db = _Data(799, C, 4 * C, seed=7 * C + integer, integer=integer)
    for M in (1, 31, 33, 799):
        what = f"(b) C={C} M={M}"
        base = _run(db, what, M=M)
        db.first(M).check(base, what)
        _bits_equal(_run(db, what, M=M, ldx=5 * C, xcol=C, ldr=C, ldy=C), base, f"{what} X at [C, 5C) of 5C")
        _bits_equal(_run(db, what, M=M, ldx=5 * C, xcol=C, ldr=3 * C, rcol=2 * C, ldy=2 * C, ycol=C), base, f"{what} ldr=3C")
        what = f"(c) C={C} M={M}"
        basec = _run(da, what, M=M)
        da.first(M).check(basec, what)
        for rcol in (0, C):
            _bits_equal(_run(da, what, M=M, ldr=3 * C, rcol=rcol), basec, f"{what} ldr=3C col={rcol}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. fused N with two activations (poem_launch_gemm_split)
_FUSED = {      # name: (N in C, act, act_split in C, act2)
    "F4_relu_gelu": (5, RELU, 1, GELU),
    "F2_none": (2, NONE, 2, NONE),
    "F3_none": (3, NONE, 3, NONE),
    "gelu_none": (3, GELU, 2, NONE),
}
_FUSED_NT = {32: 1, 64: 2, 256: 4}      # the widest panel that act_split = C (and N = 5C) allows


@pytest.mark.parametrize("integer", [False, True], ids=["randn", "integer"])
@pytest.mark.parametrize("form", list(_FUSED))
@pytest.mark.parametrize("C", [32, 64, 256])
def test_fused_two_activations(C, form, integer, ncu):
    """The decoder's fused calls (F4: relu | gelu over 5C; 2C and 3C without activation) and gelu | none, ldy = N, ragged M.
    The split restricts the panel to NT = 1 / 2 / 4 at C = 32 / 64 / 256; for so few rows the narrow-panel rule takes NT = 1,
    so every case also runs with the rule off (the wide panel) and must give the same bits."""
    nC, act, sC, act2 = _FUSED[form]
    N, K, M = nC * C, C, 77
    d = _Data(M, N, K, seed=C * 11 + nC + integer, integer=integer)
    kw = dict(act=act, act_split=sC * C, act2=act2, res=False)
    two = sC < nC
    br = gu.dispatch(M, N, K, ncu, act=act, act_split=sC * C, act2=act2)
    assert br[0] == "panel" and br[3] == (GELU in (act, act2) if two else act == GELU), br
    what = f"{form} C={C}"
    y = _run(d, what, **kw)
    d.check(y, what, **kw)
    with _switch("poem_gemm_panel_narrow", 0):
        wide = gu.dispatch(M, N, K, ncu, act=act, act_split=sC * C, act2=act2, narrow=False)
        if form == "F4_relu_gelu":
            assert wide[:2] == ("panel", _FUSED_NT[C]), f"{what}: the wide panel is {wide}, not NT = {_FUSED_NT[C]}"
        _bits_equal(_run(d, what, **kw), y, f"{what} narrow-panel rule off ({wide})")
    if two:      # each half alone (one activation, its own weight rows and bias) gives the same bits as its columns of the fused call
        s = sC * C
        for lo, hi, a in ((0, s, act), (s, N, act2)):
            part = _Data.__new__(_Data)
            part.__dict__.update(d.__dict__, N=hi - lo, w=d.w[lo:hi], wd=d.wd[lo:hi], b=d.b[lo:hi], bd=d.bd[lo:hi].contiguous())
            part.wp = hip.pack_linear(part.wd.contiguous())
            _bits_equal(_run(part, what, act=a, res=False), y[:, lo:hi], f"{what} columns [{lo}, {hi}) alone")


@pytest.mark.parametrize("C", [32, 64, 256])
def test_fused_nan_row_stays_in_its_row(C):
    """A NaN in one X row: that row's ReLU columns are NaN (relu_nan), every other row is finite and unchanged."""
    N, M = 5 * C, 77
    d = _Data(M, N, C, seed=C + 3)
    kw = dict(act=RELU, act_split=C, act2=GELU, res=False)
    clean = _run(d, "clean", **kw).clone()
    d.xd[40, 3] = float("nan")
    got = _run(d, "nan", **kw)
    assert bool(torch.isnan(got[40, :C]).all()), "the NaN row's ReLU columns are not all NaN"
    assert bool(torch.isnan(got[40]).all())
    keep = torch.arange(M, device=DEV) != 40
    assert bool(torch.isfinite(got[keep]).all())
    _bits_equal(got[keep], clean[keep], "other rows")


def _segs_call(xp, ldx, wp, bp, M, K, act, seg_cols, nsegs, ptrs, modes):
    n = max(len(ptrs), 1)
    return _fn("poem_launch_gemm_segs")(xp, ldx, wp, bp, M, K, act, seg_cols, nsegs, (_vp * n)(*ptrs), (_i * n)(*modes), hip.stream())


def test_refusals_write_nothing():
    """hipErrorInvalidValue and not one store: two activations on a shape only gemm2 takes; segments with GELU, seg_cols % 32,
    M % 32, nsegs 0 and 7."""
    C, M = 32, 64
    d = _Data(M, 5 * C, 2048, seed=1)      # K = 2048: no panel fits LDS
    rc, out = _gemm(d, act=RELU, act_split=C, act2=GELU, res=False)
    assert rc == HIP_INVALID_VALUE and out.untouched(), rc
    s = _Data(M, 6 * 96, 96, seed=2)
    outs = [_Out(M, 96) for _ in range(7)]
    ptrs = [o.ptr for o in outs]
    for what, args in (("GELU", (M, 96, GELU, 96, 6, ptrs[:6], [0] * 6)),
                       ("seg_cols % 32", (M, 96, NONE, 48, 6, ptrs[:6], [0] * 6)),
                       ("M % 32", (M - 31, 96, NONE, 96, 6, ptrs[:6], [0] * 6)),
                       ("nsegs 0", (M, 96, NONE, 96, 0, ptrs[:6], [0] * 6)),
                       ("nsegs 7", (M, 96, NONE, 96, 7, ptrs, [0] * 7))):
        rc = _segs_call(s.xd.data_ptr(), 96, s.wp.data_ptr(), s.bd.data_ptr(), *args)
        assert rc == HIP_INVALID_VALUE, f"{what}: returned {rc}"
        assert all(o.untouched() for o in outs), f"{what}: a refused launch wrote"


# ---------------------------------------------------------------------------------------------------------------------
# 3. segmented outputs (poem_launch_gemm_segs): the decoder's F1
_MODES = (1, 2, 1, 2, 0, 0)


def _segments(d, M, C, first, nsegs, what):
    """segments [first, first + nsegs) of the 6C-wide F1 in the decoder's modes (weight and bias pointers offset for first > 0)
    -> decoded (M, C) outputs; the K images are decoded by the index map and by poem_unpack_rows, which must agree"""
    modes = _MODES[first:first + nsegs]
    outs = [_Out(M, C) if m == 0 else _Image(M, C) for m in modes]
    rc = _segs_call(d.xd.data_ptr(), C, d.wp.data_ptr() + 4 * first * C * C, d.bd.data_ptr() + 4 * first * C, M, C, NONE, C, nsegs,
                    [o.ptr for o in outs], modes)
    assert rc == 0, f"{what}: launch returned {rc}"
    res = []
    for j, (o, m) in enumerate(zip(outs, modes)):
        w = f"{what} segment {first + j} (mode {m})"
        if m == 0:
            res.append(o.take(w))
            continue
        res.append(o.decode(gu.k_image_index if m == 1 else gu.v_image_index, w))
        if m == 1:
            rm = _Out(M, C)
            assert hip.lib().poem_unpack_rows(o.ptr, M, C, rm.ptr, hip.stream()) == 0
            _bits_equal(rm.take(w + " unpacked"), res[-1], w + ": poem_unpack_rows against the index map")
    return res


@pytest.mark.parametrize("integer", [False, True], ids=["randn", "integer"])
@pytest.mark.parametrize("C,M", [(C, M) for C in (32, 64, 128, 256) for M in (32, 96, 1056)] + [(1024, 32), (1024, 96), (1024, 544), (1024, 1056), (1024, 2592), (128, 16416), (32, 32960)])
def test_segments(C, M, integer, ncu):
    """K image | V image | K image | V image | rows | rows from one launch of 6 segments, and from the decoder's 4 + 2 pair:
    the same bits, equal to the column blocks of one plain row-major GEMM over N = 6C, which holds the fp64 bar."""
    d = _Data(M, 6 * C, C, seed=C + M + integer, integer=integer)
    br = gu.dispatch(M, 6 * C, C, ncu, seg_cols=C)
    assert br[0] == ("kslab" if C == 1024 and M >= 512 else "panel"), br
    if C == 32:
        assert br[1] == 1, br
    if M == 2592:
        assert br == ("kslab", 2), f"{br}: this case is meant for the image epilogues of the K-slab kernel's 512-row blocks"
    br4 = gu.dispatch(M, 4 * C, C, ncu, seg_cols=C)
    if M == 32960:
        assert br4[0] == "panel" and br4[4] and not br[4], f"{br4}: this case is meant for the 4-segment launch under the XCD map"
    if M == 16416:
        assert br[:3] == ("panel", 4, 2), f"{br}: this case is meant for the image epilogues of 64-row wave tiles on wide panels"
    what = f"segs C={C} M={M} {br}"
    plain = _run(d, what + " plain", res=False)
    d.check(plain, what + " plain", res=False)
    six = _segments(d, M, C, 0, 6, what + " 6")
    pair = _segments(d, M, C, 0, 4, what + " 4") + _segments(d, M, C, 4, 2, what + " 2")
    for j in range(6):
        _bits_equal(six[j], plain[:, j * C:(j + 1) * C], f"{what}: segment {j} of 6 against the plain GEMM's columns")
        _bits_equal(pair[j], six[j], f"{what}: segment {j} of the 4 + 2 pair against the single launch")
    with _switch("poem_gemm_xcd_map", 0):           # (the XCD map's row ranges meet sidx / ycol0 in the 4-segment launch at M 32960)
        plain_map = _segments(d, M, C, 0, 4, what + " 4 xcd_map off")
    for j in range(4):
        _bits_equal(plain_map[j], pair[j], f"{what}: segment {j} of 4 with poem_gemm_xcd_map(0)")
    with _switch("poem_gemm_panel_narrow", 0):      # the widest panel the segment width allows (NT 1 / 2 / 4 at C 32 / 64 / 128 ..)
        wide = _segments(d, M, C, 0, 6, what + " 6 wide")
    for j in range(6):
        _bits_equal(wide[j], six[j], f"{what}: segment {j} with the narrow-panel rule off")


# ---------------------------------------------------------------------------------------------------------------------
# 4. dispatch branches, bit for bit
_BRANCH_CASES = {      # name: (M, N, K, the branch on a 256-CU device with act NONE)
    "panel_1_1": (799, 256, 256, ("panel", 1, 1, False, False)),
    "panel_1_2": (16389, 128, 32, ("panel", 1, 2, False, False)),
    "panel_2_1": (100, 192, 512, ("panel", 2, 1, False, False)),
    "panel_2_2": (16389, 256, 32, ("panel", 2, 2, False, False)),
    "panel_4_1_xcd": (4133, 4096, 32, ("panel", 4, 1, False, True)),
    "panel_4_2": (16389, 512, 32, ("panel", 4, 2, False, False)),
    "kslab_1": (517, 64, 1024, ("kslab", 1)),
    "kslab_2": (8190, 2048, 640, ("kslab", 2)),
    "gemm2_1_1": (77, 96, 512, ("gemm2", 1, 1)),
    "gemm2_1_2": (77, 64, 1024, ("gemm2", 1, 2)),
    "gemm2_2_4": (6085, 1024, 520, ("gemm2", 2, 4)),
}


def _intended(name, act, ncu, **kw):
    M, N, K, want = _BRANCH_CASES[name]
    if want[0] == "panel":
        want = want[:3] + (act == GELU,) + want[4:]
    got = gu.dispatch(M, N, K, ncu, act=act, **kw)
    return want, got


def test_case_list_reaches_every_branch(ncu):
    """On this device the cases take the branches their names say: every launch_panel_t<NT, MT, GELU>, xcd_map on and off, both
    K-slab heights, the three gemm2 tiles; and the switches move the cases that they are meant to move."""
    seen = set()
    for name in _BRANCH_CASES:
        for act in (NONE, GELU):
            want, got = _intended(name, act, ncu)
            assert got == want, f"{name} act={act}: this device ({ncu} CUs) takes {got}, the case is meant for {want}"
            seen.add(got)
    for nt in (1, 2, 4):
        for mt in (1, 2):
            for gelu in (False, True):
                assert any(b[:4] == ("panel", nt, mt, gelu) for b in seen), f"no case for launch_panel_t<{nt}, {mt}, {gelu}>"
    assert {b[4] for b in seen if b[0] == "panel"} == {False, True}
    assert {("kslab", 1), ("kslab", 2), ("gemm2", 1, 1), ("gemm2", 1, 2), ("gemm2", 2, 4)} <= seen
    assert _intended("panel_1_1", NONE, ncu, narrow=False)[1][:3] == ("panel", 4, 1)
    assert _intended("panel_1_2", NONE, ncu, narrow=False)[1][:3] == ("panel", 4, 1)
    assert _intended("panel_4_1_xcd", NONE, ncu, xcd=False)[1] == ("panel", 4, 1, False, False)
    assert _intended("kslab_1", NONE, ncu, kslab=False)[1] == ("gemm2", 1, 2)
    assert _intended("kslab_2", NONE, ncu, kslab=False)[1] == ("gemm2", 2, 4)


@pytest.mark.parametrize("act", [NONE, GELU], ids=["none", "gelu"])
@pytest.mark.parametrize("name", list(_BRANCH_CASES))
def test_dispatch_branches(name, act, ncu):
    """The default dispatch holds the fp64 bar (and is exact on integers); each switch off, and gemm2 called directly, give the
    same bits -- bias, activation and residual included."""
    M, N, K, _ = _BRANCH_CASES[name]
    want, got = _intended(name, act, ncu)
    assert got == want, f"{name}: this device ({ncu} CUs) takes {got}, the case is meant for {want}"
    d = _Data(M, N, K, seed=M + N + K + act)
    what = f"{name} act={act} {got}"
    y = _run(d, what, act=act)
    d.check(y, what, act=act)
    for sw in ("poem_gemm_panel_narrow", "poem_gemm_xcd_map", "poem_gemm_kslab"):
        with _switch(sw, 0):
            _bits_equal(_run(d, what, act=act), y, f"{what}: {sw}(0)")
    _bits_equal(_run(d, what, act=act, gemm2=True), y, f"{what}: poem_launch_gemm2")
    if act == NONE:
        di = _Data(M, N, K, seed=M + N + K, integer=True)
        di.check(_run(di, what + " integer", act=RELU), what + " integer", act=RELU)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the public PA layout: poem_gemm_ex, poem_pack_rows, poem_unpack_rows
def _pack_rows(t, what):
    """t (rows, cols) on the device -> _Image through poem_pack_rows; the map and the zero pad rows are checked"""
    rows, cols = t.shape
    img = _Image(rows, cols)
    t = t.contiguous()
    assert hip.lib().poem_pack_rows(t.data_ptr(), rows, cols, img.ptr, hip.stream()) == 0, what
    pad = (rows + 31) // 32 * 32
    full = img.flat(what)[gu.pa_index(pad, cols).to(DEV)]
    _bits_equal(full[:rows], t, f"{what}: packed rows against the index map")
    assert bool((full[rows:].view(torch.int32) == 0).all()), f"{what}: pad rows are not zero"
    return img


@pytest.mark.parametrize("cols", [8, 24, 256])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 799])
def test_pack_unpack_round_trip(rows, cols):
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    t = torch.randn(rows, cols, generator=g).to(DEV)
    what = f"rows={rows} cols={cols}"
    img = _pack_rows(t, what)
    out = _Out(rows, cols)
    assert hip.lib().poem_unpack_rows(img.ptr, rows, cols, out.ptr, hip.stream()) == 0
    _bits_equal(out.take(what), t, what + ": unpack(pack(x))")


def _gemm_ex(xp, ldx, d, rp, ldr, yp, ldy, M, act, in_pa, out_pa, bias=True):
    rc = hip.lib().poem_gemm_ex(xp, ldx, d.wp.data_ptr(), d.bd.data_ptr() if bias else None, rp, ldr, yp, ldy, M, d.N, d.K, act,
                                in_pa, out_pa, hip.stream())
    torch.cuda.synchronize()
    return rc


def _ex_stage(d, x, act, in_pa, out_pa, what):
    """one poem_gemm_ex stage over the stage's data d (its residual d.rd in the output's layout): x is a (M, K) row-major
    device tensor or an _Image -> the same for y"""
    M = d.M
    assert gu.gemm2_branch(M, d.N) == d.branch, (what, gu.gemm2_branch(M, d.N))
    xp = x.ptr if in_pa else x.data_ptr()
    if out_pa:
        y, r = _Image(M, d.N), _pack_rows(d.rd, what + " residual")
        assert _gemm_ex(xp, d.K, d, r.ptr, d.N, y.ptr, d.N, M, act, int(in_pa), 1) == 0, what
        y.flat(what)
        return y
    out = _Out(M, d.N)
    assert _gemm_ex(xp, d.K, d, d.rd.data_ptr(), d.N, out.ptr, d.N, M, act, int(in_pa), 0) == 0, what
    return out.take(what).contiguous()


def _unpacked(img):
    return img.decode(gu.pa_index, "PA output")


@pytest.mark.parametrize("act,integer", [(NONE, False), (RELU, False), (GELU, False), (NONE, True), (RELU, True)],
                         ids=["none", "relu", "gelu", "none_integer", "relu_integer"])
@pytest.mark.parametrize("widths", [(128, 64, 96), (64, 96, 128), (96, 128, 64)])
def test_pa_chains(widths, act, integer):
    """RM -> PA -> PA -> RM and PA -> RM, every stage with bias, activation and a residual in its output's layout, M = 77:
    fp64 bar on the chain, bit-equal to the all-row-major chain of poem_gemm_ex stage by stage.  The widths (4, 2 and 3 column
    tiles) rotate, so that gemm2's <1,2> and <1,1> tiles each run in every layout pair; K = 24 (an odd number of k-chunks).  The integer-valued chains (exact) run without GELU."""
    M, K0 = 77, 24
    g = torch.Generator().manual_seed(sum(widths) + act)
    x0 = (torch.randint(-2, 3, (M, K0), generator=g).float() if integer else torch.randn(M, K0, generator=g))
    stages, K = [], K0
    for j, N in enumerate(widths):
        d = _Data(M, N, K, seed=N * 3 + j + act, integer=integer)
        if integer:      # (keeps the chain's values small integers: weights in -1..1 with few non-zeros, relu / none only)
            d.w = (torch.randint(0, 8, (N, K), generator=g) == 0).float() * (torch.randint(0, 2, (N, K), generator=g) * 2 - 1).float()
            d.wd = d.w.to(DEV)
            d.wp = hip.pack_linear(d.wd)
        d.branch = (1, 1) if (N // 32) % 2 else (1, 2)
        stages.append(d)
        K = N
    what = f"chain {widths} act={act}"
    x0d = x0.to(DEV)
    # all row-major
    rm, t = [], x0d
    for d in stages:
        t = _ex_stage(d, t, act, False, False, what + " RM")
        rm.append(t)
    # RM -> PA -> PA -> RM
    a = _ex_stage(stages[0], x0d, act, False, True, what + " RM->PA")
    _bits_equal(_unpacked(a), rm[0], what + " stage 1 (RM -> PA)")
    b = _ex_stage(stages[1], a, act, True, True, what + " PA->PA")
    _bits_equal(_unpacked(b), rm[1], what + " stage 2 (PA -> PA)")
    c = _ex_stage(stages[2], b, act, True, False, what + " PA->RM")
    _bits_equal(c, rm[2], what + " stage 3 (PA -> RM)")
    # PA -> RM on the packed input
    p = _ex_stage(stages[0], _pack_rows(x0d, what), act, True, False, what + " PA->RM first")
    _bits_equal(p, rm[0], what + " PA -> RM")
    # the chain restated
    r64, r32 = x0.double(), x0
    for j, d in enumerate(stages):
        r64 = gu.gemm_ref(r64, d.w, d.b, d.r, act=act)
        r32 = gu.gemm_ref(r32, d.w, d.b, d.r, act=act, fp32=True)
        if integer:
            assert float(r64.abs().max()) < 2 ** 23
            _exact(rm[j], r64.float(), f"{what} stage {j + 1} (integer-valued: must be exact)")
        else:
            _assert_close(rm[j], r64, r32, f"{what} stage {j + 1}")


@pytest.mark.parametrize("mtiles", [191, 192], ids=["odd_tiles", "even_tiles"])
def test_pa_big_branch(mtiles):
    """gemm2's 64 x 128 wave tiles (<2,4>: N = 1024, (mtiles + 1) / 2 * 8 >= 768) in all four layout pairs, ragged M, with an odd
    and an even number of row tiles.  At 191 tiles the second tile of the last wave lies past the PA buffer's ceil(M / 32) * 32
    rows: its operand loads are clamped to the last tile (see LABNOTES) and its accumulators are never stored."""
    M, N, K = 32 * mtiles - 27, 1024, 16
    assert gu.gemm2_branch(M, N) == (2, 4)
    for integer in (False, True):
        d = _Data(M, N, K, seed=mtiles + integer, integer=integer)
        d.branch = (2, 4)
        for act in ((NONE,) if integer else (NONE, RELU, GELU)):
            what = f"big mtiles={mtiles} act={act} integer={integer}"
            rm = _ex_stage(d, d.xd, act, False, False, what + " RM->RM")
            d.check(rm, what, act=act)
            xpa = _pack_rows(d.xd, what)
            _bits_equal(_ex_stage(d, xpa, act, True, False, what + " PA->RM"), rm, what + " PA -> RM")
            _bits_equal(_unpacked(_ex_stage(d, d.xd, act, False, True, what + " RM->PA")), rm, what + " RM -> PA")
            _bits_equal(_unpacked(_ex_stage(d, xpa, act, True, True, what + " PA->PA")), rm, what + " PA -> PA")


def test_gemm_ex_refusals_write_nothing():
    """POEM_E_ARG and no store: PA output with N % 32 != 0, layout flags other than 0 / 1, a y that is not 16-byte aligned."""
    M = 40
    d = _Data(M, 48, 16, seed=5)
    out = _Out(M + 32, 64)
    args = (d.xd.data_ptr(), 16, d, None, 0)
    assert _gemm_ex(*args, out.ptr, 48, M, NONE, 0, 1) == POEM_E_ARG
    for flags in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        assert _gemm_ex(*args, out.ptr, 48, M, NONE, *flags) == POEM_E_ARG, flags
    assert _gemm_ex(*args, out.ptr + 4, 48, M, NONE, 0, 0) == POEM_E_ARG
    assert out.untouched()
    assert _gemm_ex(*args, out.ptr, 48, M, NONE, 0, 0) == 0 and not out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# 6. narrow Linear
def _narrow(xd, K, wd, bd, based, rows, N, ldx=None, xcol=0, reg_update=False):
    xbuf, xp = _block(xd[:rows], ldx or K, xcol)
    out = _Out(rows, N)
    bp, basep = (None if bd is None else bd.data_ptr()), (None if based is None else based[:rows].contiguous().data_ptr())
    if reg_update:
        rc = hip.lib().poem_reg_update(xp, wd.data_ptr(), bp, basep, out.ptr, rows, K, hip.stream())
    else:
        rc = _fn("poem_launch_narrow_linear")(xp, ldx or K, wd.data_ptr(), bp, basep, out.ptr, rows, K, N, hip.stream())
    assert rc == 0, rc
    got = out.take(f"narrow N={N} K={K} rows={rows}")
    del xbuf
    return got


_NARROW = {      # name: (N, base, bias, X inside 5K-wide rows, row counts)
    "reg_branch_2": (3, True, True, True, (1, 5, 799)),
    "mano_linear": (106, False, True, False, (32,)),
    "eight_no_bias": (8, True, False, False, (1, 5, 799)),
}


@pytest.mark.parametrize("K", [32, 96, 256, 1024])
@pytest.mark.parametrize("form", list(_NARROW))
def test_narrow_linear(form, K):
    N, has_base, has_bias, strided, row_counts = _NARROW[form]
    g = torch.Generator().manual_seed(K + N)
    R = max(row_counts)
    x, w = torch.randn(R, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    b = (torch.arange(N).float() / 8 - 1 + 0.01 * torch.randn(N, generator=g)) if has_bias else None
    base = torch.randn(R, N, generator=g) if has_base else None
    xd, wd = x.to(DEV), w.to(DEV)
    bd, based = (None if b is None else b.to(DEV)), (None if base is None else base.to(DEV))
    kw = dict(ldx=5 * K, xcol=K) if strided else {}
    for rows in row_counts:
        what = f"narrow {form} K={K} rows={rows}"
        got = _narrow(xd, K, wd, bd, based, rows, N, **kw)
        bs = None if base is None else base[:rows]
        _assert_close(got, gu.narrow_ref(x[:rows], w, b, bs), gu.narrow_ref(x[:rows], w, b, bs, fp32=True), what)
        if form == "reg_branch_2":
            _bits_equal(_narrow(xd, K, wd, bd, based, rows, N, reg_update=True), _narrow(xd, K, wd, bd, based, rows, N),
                        what + ": poem_reg_update against the launcher")
    xi, wi = torch.randint(-4, 5, (5, K), generator=g).float(), torch.randint(-4, 5, (N, K), generator=g).float()
    got = _narrow(xi.to(DEV), K, wi.to(DEV), None, None, 5, N)
    _exact(got, xi @ wi.T, f"narrow {form} K={K} integer-valued: must be exact")


def test_narrow_linear_column_split():
    """8200 rows take the one-block-per-row-group form (npb = N), their first 100 rows alone the one-column-per-block form
    (npb = 1): the same bits per (row, column)."""
    rows, K, N = 8200, 32, 3
    assert ((rows + 3) // 4) >= 2048 and (100 + 3) // 4 * N <= 65535
    g = torch.Generator().manual_seed(9)
    x, w, b, base = torch.randn(rows, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(rows, N, generator=g)
    xd, wd, bd, based = (t.to(DEV) for t in (x, w, b, base))
    big = _narrow(xd, K, wd, bd, based, rows, N, ldx=5 * K, xcol=K)
    _assert_close(big, gu.narrow_ref(x, w, b, base), gu.narrow_ref(x, w, b, base, fp32=True), "narrow 8200 rows")
    _bits_equal(_narrow(xd, K, wd, bd, based, 100, N, ldx=5 * K, xcol=K), big[:100], "npb = 1 against npb = N")


# ---------------------------------------------------------------------------------------------------------------------
# 7. LayerNorm
@pytest.mark.parametrize("eps", [1e-12, 1e-5])
@pytest.mark.parametrize("cols", [32, 64, 96, 256, 1024])
def test_layernorm_forms(cols, eps):
    """rows 1 / 3 / 5 / 799 (one to four waves of the last block idle), a guard behind y; plain rows, rows of mean 100 with unit
    spread, and a row whose entries span six decades."""
    g = torch.Generator().manual_seed(cols)
    gm, bt = 1 + 0.1 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)
    gd, bd = gm.to(DEV), bt.to(DEV)
    for rows in (1, 3, 5, 799):
        for kind in ("plain", "mean100", "range"):
            x = torch.randn(rows, cols, generator=g)
            if kind == "mean100":
                x = x + 100.0
            if kind == "range":
                x[rows // 2] = x[rows // 2] * torch.logspace(-3, 3, cols)[torch.randperm(cols, generator=g)]
            xd = x.to(DEV)
            out = _Out(rows, cols)
            rc = _fn("poem_launch_layernorm")(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.ptr, rows, cols, eps, hip.stream())
            assert rc == 0, rc
            what = f"layernorm cols={cols} rows={rows} eps={eps} {kind}"
            _assert_close(out.take(what), gu.layernorm_ref(x, gm, bt, eps), gu.layernorm_ref(x, gm, bt, eps, fp32=True), what)
