"""Both attention kernels in every form the decoder launches them, against a float64 restatement of the operation.

The vector attention (vecattn.hip) is reached through the launchers the decoder calls -- plain and composed MODE 0, composed
MODE 3 (fewer than 32 neighbours), MODE 1 tables + MODE 2 in both of the decoder's key layouts, composed MODE 4 -- and the split
kernel (vecattn_split.hip); the cross attention (attn.hip) through the operator and through the decoder's image form.  Cases are
chosen per dispatch case (every embed width, the one-query blocks at 256), per item map (the XCD remaps taken and not taken),
with q / k / v as column blocks of wider rows whose other columns hold NaN, and with peaked softmaxes, where a neighbour / weight
mis-pairing or a skipped rescale is gross instead of a small error near the tolerance.

Tolerance per case: |HIP - fp64| <= 4 |fp32 - fp64| + 1e-6 max|fp64|, where fp32 is the same case restated in fp32 on the CPU from
the same fp32 inputs the kernel takes (the vector attention's C x C products summed k-sequentially, as the kernel sums them).
Masking invariants and the guard rows behind each output are checked bit for bit.

Coverage (form x width x item map; "remap": B * ceil(Q / P) % 8 == 0, for MODE 2 ceil(Q / P) % 8 == 0):
  MODE 0 plain, composed   C 32 .. 1024, remap (with a partial last query group where P > 1) and not, self / cross strides
  MODE 0 composed, C 256   va_p1 0 / 1 / 2 at (B, Q) = (2, 4), (3, 5), (1, 799), (1, 1)
  MODE 3 composed          kvalid 1 / 7 / 31 at C 64 (remap), 128 (not), 256 (Q = 799); the plain form is refused
  MODE 4 composed          K 33 / 64 at C 128 (remap), 512 (not), 32 (Q = 1)
  MODE 1 + MODE 2          C 32 .. 1024 x key layouts (anchor rows of the projection, identity ids into a 32-row block)
                           x remap and not; Q = 799 and Q = 1 at C 256
  split kernel             C 128 / 512 / 1024, contiguous and both strides
  cross attention          NK 1056 / 2048 / 3072 / 16384 (1 chunk of 33 tiles, 2, 3, 16 chunks), 17408 refused; head dims
                           8 .. 256 with 1 .. 16 heads at NQ 1 / 31 / 32 / 33; the decoder's image form (q at a 2C stride,
                           q_batch_rows 0, K / V images from the F1 GEMM); logits over +-100, a maximum that moves on every
                           key tile, identical keys."""
import ctypes
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import poem_oracle as po
from poem_v2_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIP_INVALID_VALUE = 1          # hipErrorInvalidValue
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t

# launchers.h: launchers of libpoem_hip.so that the decoder calls.  They are not part of the public ABI, so they are bound here
# (as separate function objects) rather than in hip.SIGNATURES.
_PROTOS = {
    "poem_launch_vector_attention": (_i, [_vp] * 4 + [_i] + [_vp] * 3 + [_i] + [_vp] * 9 + [_i] * 7 + [_vp]),
    "poem_launch_vector_attention_k": (_i, [_vp] * 3 + [_i] * 2 + [_vp] * 3 + [_i] + [_vp] * 9 + [_i] * 7 + [_vp]),
    "poem_vector_attention_table_floats": (_sz, [_i, _i]),
    "poem_launch_vector_attention_tables": (_i, [_vp] * 10 + [_i] * 2 + [_vp]),
    "poem_launch_vector_attention_anchored": (_i, [_vp] * 4 + [_i] + [_vp] * 4 + [_i] * 6 + [_vp]),
    "poem_launch_vector_attention_split": (_i, [_vp] * 4 + [_i] + [_vp] * 3 + [_i] + [_vp] * 8 + [_i] * 6 + [_vp]),
    "poem_vecattn_valid_neighbours": (None, [_i]),
    "poem_vecattn_one_query_blocks": (None, [_i]),
    "poem_launch_cross_attention_img": (_i, [_vp, _i] + [_vp] * 3 + [_i] * 5 + [_vp] * 2),
    "poem_launch_cross_attention_imgq": (_i, [_vp, _i, _i] + [_vp] * 3 + [_i] * 5 + [_vp] * 2),
    "poem_launch_gemm_segs": (_i, [_vp, _i, _vp, _vp] + [_i] * 5 + [_vp] * 3),
    "poem_cross_attention_scratch_floats": (_sz, [_i] * 6),
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


def _assert_close(got, ref64, ref32, what):
    got, ref64, ref32 = (t.double().cpu() for t in (got, ref64, ref32))
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    e = float((got - ref64).abs().max())
    e32 = float((ref32 - ref64).abs().max())
    bar = 4 * e32 + 1e-6 * float(ref64.abs().max())
    assert e <= bar, f"{what}: |hip - fp64| = {e:.3e} > 4 |fp32 - fp64| + floor = {bar:.3e} (fp32: {e32:.3e})"


# ---- output buffers with a guard region: rows past the output keep a canary pattern
_CANARY = 0x7FC0DEAD      # a NaN bit pattern no kernel writes
_GUARD_ROWS = 3


def _guarded(rows, C):
    return torch.full(((rows + _GUARD_ROWS) * C,), _CANARY, dtype=torch.int32, device=DEV)


def _unguard(buf, rows, C, what):
    torch.cuda.synchronize()
    assert bool((buf[rows * C:] == _CANARY).all()), f"{what}: a write past the last output row"
    return buf[:rows * C].view(torch.float32).view(rows, C).clone()


def _block(t, ld, col):
    """t (rows, C) as columns [col, col + C) of rows of `ld` floats; every other column is NaN -> (buffer, pointer)."""
    buf = torch.full((t.shape[0], ld), float("nan"), device=DEV)
    buf[:, col:col + t.shape[1]] = t.to(DEV)
    return buf, buf.data_ptr() + 4 * col


# (ldq, q column, ldk, k column, ldv, v column) in units of C: the engine's strides
_LAYOUTS = {
    "rows": (1, 0, 1, 0, 1, 0),        # the operator ABI's contiguous rows
    "self": (3, 0, 3, 1, 3, 2),        # q | k | v of the fused self-attention projection (3C-wide rows)
    "cross": (1, 0, 6, 4, 6, 5),       # q at C; k / v as column blocks of the 6C-wide basis-point projection
}


# ---------------------------------------------------------------------------------------------------------------------
# vector attention
_HOT = 8.0      # "hot" fc_gamma.2: logits a / sqrt(C) of standard deviation ~10 -> each softmax dominated by one or two neighbours


def _weights(C, g, hot):
    w = {}
    for n, shp in (("fc_delta.0", (C, 3)), ("fc_delta.2", (C, C)), ("fc_gamma.0", (C, C)), ("fc_gamma.2", (C, C))):
        w["p." + n + ".weight"] = torch.randn(*shp, generator=g) / math.sqrt(shp[1])
        w["p." + n + ".bias"] = torch.randn(shp[0], generator=g) * 0.1
    if hot:
        w["p.fc_gamma.2.weight"] = w["p.fc_gamma.2.weight"] * (_HOT * math.sqrt(C))
    return w


def _compose(w, q, k):
    """The composed form's inputs, formed in fp64 and rounded once: qg = W_g1 q + (W_g1 b_d2 + b_g1), kg = W_g1 k, W_g1 W_d2."""
    Wg1, Wd2 = w["p.fc_gamma.0.weight"].to(DEV).double(), w["p.fc_delta.2.weight"].to(DEV).double()
    cvec = Wg1 @ w["p.fc_delta.2.bias"].to(DEV).double() + w["p.fc_gamma.0.bias"].to(DEV).double()
    qg = (q.to(DEV).double() @ Wg1.T + cvec).float().cpu()
    kg = (k.to(DEV).double() @ Wg1.T).float().cpu()
    return qg, kg, (Wg1 @ Wd2).float().cpu()


def _linear_seq(x, w, b=None, kc=2):
    """x w^T (+ b) in fp32 summed in the kernel's order: one running fp32 sum over k in steps of 2 (the k-depth of the fp32
    MFMA).  A BLAS GEMM sums in many partial accumulators, several times more accurately than a k-sequential chain at C = 1024
    with peaked logits: against it the 4x bar would measure the summation order rather than the kernel."""
    x2, wt = x.reshape(-1, x.shape[-1]), w.T.contiguous()
    acc = torch.zeros(x2.shape[0], w.shape[0])
    for k0 in range(0, w.shape[1], kc):
        acc.addmm_(x2[:, k0:k0 + kc], wt[k0:k0 + kc])
    acc = acc.view(*x.shape[:-1], w.shape[0])
    return acc if b is None else acc + b


def _core32(w, q, k, v, delta, C, wc=None):
    """The vector attention restated in fp32.  wc given: the composed form (vecattn.hip COMP) -- q, k are qg, kg and
    g = relu(qg - kg + (W_g1 W_d2) h); otherwise the plain form g = relu(W_g1 (q - k + pos) + b_g1)."""
    h = F.relu(F.linear(delta, w["p.fc_delta.0.weight"], w["p.fc_delta.0.bias"]))
    pos = _linear_seq(h, w["p.fc_delta.2.weight"], w["p.fc_delta.2.bias"])
    if wc is None:
        gg = F.relu(_linear_seq(q[:, :, None] - k + pos, w["p.fc_gamma.0.weight"], w["p.fc_gamma.0.bias"]))
    else:
        gg = F.relu(q[:, :, None] - k + _linear_seq(h, wc))
    a = _linear_seq(gg, w["p.fc_gamma.2.weight"], w["p.fc_gamma.2.bias"])
    a = torch.softmax(a / math.sqrt(C), dim=-2)
    return torch.einsum("bmnf,bmnf->bmf", a, v + pos)


def _rows(n):
    """Output rows the references are computed on: all of them, or 160 spread rows incl. the first and the last."""
    if n <= 256:
        return torch.arange(n)
    return torch.unique(torch.linspace(0, n - 1, 160).round().long())


def _va_check(got, c, q, xyz, kn, vn, nxyz, qg=None, kgn=None, what=""):
    """got (R, C) against the vector attention of the rows: q (R, C) raw query rows, xyz (R, 3), neighbours kn / vn (R, K, C) raw,
    nxyz (R, K, 3); qg / kgn: the composed inputs of those rows (composed form: the fp32 restatement is the composed one)."""
    C = c.C
    sel = _rows(q.shape[0])
    one = lambda t: t[sel][None]        # noqa: E731  (the oracle's (B, M, ...) layout, one sample)
    w64 = {n: t.to(DEV).double() for n, t in c.w.items()}
    ref64 = po._vec_attn_core(w64, "p.", one(q).to(DEV).double(), one(kn).to(DEV).double(), one(vn).to(DEV).double(),
                              one(xyz).to(DEV).double()[:, :, None] - one(nxyz).to(DEV).double(), C)[0]
    delta32 = one(xyz)[:, :, None] - one(nxyz)
    if qg is None:
        ref32 = _core32(c.w, one(q), one(kn), one(vn), delta32, C)[0]
    else:
        ref32 = _core32(c.w, one(qg), one(kgn), one(vn), delta32, C, wc=c.wc)[0]
    _assert_close(got[sel], ref64, ref32, what)


def _va_case(C, B, Q, NS, seed, hot, composed, layout, ldidx=32):
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(C=C, B=B, Q=Q, NS=NS, composed=composed, layout=layout)
    c.w = _weights(C, g, hot)
    c.qxyz = torch.rand(B, Q, 3, generator=g) * 2 - 1
    c.sxyz = torch.rand(B, NS, 3, generator=g) * 2 - 1
    c.q, c.k, c.v = torch.randn(B, Q, C, generator=g), torch.randn(B, NS, C, generator=g), torch.randn(B, NS, C, generator=g)
    c.idx = torch.randint(0, NS, (B, Q, ldidx), generator=g, dtype=torch.int32)
    c.g = g
    if composed:
        c.qg, c.kg, c.wc = _compose(c.w, c.q, c.k)
    c.dev = {n: t.to(DEV).contiguous() for n, t in c.w.items()}
    c.wd2p = hip.pack_linear(c.dev["p.fc_delta.2.weight"])
    c.wg1p = hip.pack_linear(c.wc.to(DEV) if composed else c.dev["p.fc_gamma.0.weight"])
    c.wg2p = hip.pack_linear(c.dev["p.fc_gamma.2.weight"])
    lq, cq, lk, ck, lv, cv = _LAYOUTS[layout]
    c.ldq, c.ldk, c.ldv = lq * C, lk * C, lv * C
    c.qbuf, c.qp = _block((c.qg if composed else c.q).reshape(B * Q, C), c.ldq, cq * C)
    c.kbuf, c.kp = _block((c.kg if composed else c.k).reshape(B * NS, C), c.ldk, ck * C)
    c.vbuf, c.vp = _block(c.v.reshape(B * NS, C), c.ldv, cv * C)
    c.qxyz_d, c.sxyz_d = c.qxyz.to(DEV), c.sxyz.to(DEV)
    return c


def _va_run(c, idx, nk=None):
    """One launch of the full kernel (MODE 0 / 3; nk: MODE 4 with K = nk at the row stride of idx) -> output rows."""
    B, Q, C = c.B, c.Q, c.C
    d = c.dev
    out = _guarded(B * Q, C)
    idx_d = idx.to(DEV).contiguous()
    ws = (d["p.fc_delta.0.weight"].data_ptr(), d["p.fc_delta.0.bias"].data_ptr(), c.wd2p.data_ptr(), d["p.fc_delta.2.bias"].data_ptr(),
          c.wg1p.data_ptr(), d["p.fc_gamma.0.bias"].data_ptr(), c.wg2p.data_ptr(), d["p.fc_gamma.2.bias"].data_ptr())
    tail = (out.data_ptr(), B, Q, C, c.ldq, c.ldk, c.ldv, int(c.composed), hip.stream())
    if nk is None:
        rc = _fn("poem_launch_vector_attention")(c.qxyz_d.data_ptr(), c.sxyz_d.data_ptr(), None, idx_d.data_ptr(), 0, c.qp, c.kp,
                                                 c.vp, c.NS, *ws, *tail)
    else:
        rc = _fn("poem_launch_vector_attention_k")(c.qxyz_d.data_ptr(), c.sxyz_d.data_ptr(), idx_d.data_ptr(), nk, idx.shape[-1],
                                                   c.qp, c.kp, c.vp, c.NS, *ws, *tail)
    assert rc == 0, f"launch failed: hipError {rc}"
    return _unguard(out, B * Q, C, f"C={C} B={B} Q={Q}")


def _va_expect(c, got, idx, what):
    """Check the rows of `got` against the references over the neighbour ids idx (B, Q, K) of the case's sources."""
    B, Q, C = c.B, c.Q, c.C
    il = idx.long()
    flat = lambda t: t.reshape(B * Q, *t.shape[2:])    # noqa: E731
    kn, vn, nxyz = (flat(po.index_points(t, il)) for t in (c.k, c.v, c.sxyz))
    kgn = flat(po.index_points(c.kg, il)) if c.composed else None
    _va_check(got, c, flat(c.q), flat(c.qxyz), kn, vn, nxyz, flat(c.qg) if c.composed else None, kgn, what)


def _group(C):
    return {32: 2, 64: 2, 128: 4, 256: 2, 512: 1, 1024: 1}[C]      # queries per block (vecattn.hip dispatch_va)


# item maps: "xcd" -- B * ceil(Q / P) % 8 == 0 (the XCD remap), partial last query group where P > 1; "odd" -- not
def _item_shape(C, imap):
    P = _group(C)
    return (2, 4 * P - (P > 1)) if imap == "xcd" else (3, 2 * P + 1)


@pytest.mark.parametrize("C", [32, 64, 128, 256, 512, 1024])
@pytest.mark.parametrize("composed", [True, False])
@pytest.mark.parametrize("imap", ["xcd", "odd"])
def test_vector_attention_every_width_both_forms(C, composed, imap):
    """MODE 0, plain and composed, at every embed width, in both item maps, with strided q / k / v (NaN outside the blocks);
    the XCD-remapped cases have peaked softmaxes."""
    B, Q = _item_shape(C, imap)
    assert (B * -(-Q // _group(C)) % 8 == 0) == (imap == "xcd")
    layout = ("self" if composed else "cross") if imap == "xcd" else ("cross" if composed else "self")
    c = _va_case(C, B, Q, 70, seed=C * 10 + composed * 2 + (imap == "xcd"), hot=imap == "xcd", composed=composed, layout=layout)
    got = _va_run(c, c.idx)
    _va_expect(c, got, c.idx, f"MODE 0 {'composed' if composed else 'plain'} C={C} {imap} {layout}")


@pytest.mark.parametrize("p1", [0, 1, 2])
@pytest.mark.parametrize("B,Q", [(2, 4), (3, 5), (1, 799), (1, 1)])
def test_vector_attention_one_query_blocks_at_256(p1, B, Q):
    """The embed-256 instantiations the decoder picks with va_p1 (one-query blocks, 3 or 2 blocks per SIMD) next to the
    two-query blocks, composed, at the decoder's strides: item counts with and without the XCD remap, Q = 799 and Q = 1."""
    c = _va_case(256, B, Q, 300, seed=B * 1000 + Q + p1, hot=(B + Q) % 2 == 0, composed=True, layout="self")
    L = _fn("poem_vecattn_one_query_blocks")
    try:
        L(p1)
        got = _va_run(c, c.idx)
    finally:
        L(0)
    _va_expect(c, got, c.idx, f"va_p1={p1} B={B} Q={Q}")


def _replace_masked(c, idx, first):
    """idx with the columns from `first` on replaced by other valid ids (different rows of the sources)."""
    other = idx.clone()
    other[..., first:] = (idx[..., first:] + 1 + torch.randint(0, c.NS - 1, idx[..., first:].shape, generator=c.g,
                                                                dtype=torch.int32)) % c.NS
    assert not torch.equal(other, idx)
    return other


@pytest.mark.parametrize("kvalid", [1, 7, 31])
@pytest.mark.parametrize("C,B,Q", [(64, 2, 7), (128, 3, 5), (256, 1, 799)])
def test_vector_attention_masked_neighbours(kvalid, C, B, Q):
    """MODE 3 (N_NEIGHBOR / N_NEIGHBOR_QUERY below 32; composed): only the first kvalid columns count -- against the reference
    over those columns, with a peaked softmax; the ids in the masked columns do not change a bit of the output."""
    c = _va_case(C, B, Q, 90, seed=C + kvalid * 7 + B, hot=True, composed=True, layout="self")
    L = _fn("poem_vecattn_valid_neighbours")
    try:
        L(kvalid)
        got = _va_run(c, c.idx)
        again = _va_run(c, _replace_masked(c, c.idx, kvalid))
    finally:
        L(32)
    assert torch.equal(got, again), "masked neighbour columns change the output"
    _va_expect(c, got, c.idx[..., :kvalid], f"MODE 3 kvalid={kvalid} C={C}")


def test_vector_attention_plain_form_refuses_masked_neighbours():
    """The plain form has no masked (MODE 3) instantiation: the launcher refuses it instead of running all 32 columns."""
    c = _va_case(64, 1, 4, 40, seed=5, hot=False, composed=False, layout="rows")
    L = _fn("poem_vecattn_valid_neighbours")
    out = _guarded(4, 64)
    d = c.dev
    try:
        L(7)
        rc = _fn("poem_launch_vector_attention")(c.qxyz_d.data_ptr(), c.sxyz_d.data_ptr(), None, c.idx.to(DEV).data_ptr(), 0, c.qp,
                                                 c.kp, c.vp, c.NS, d["p.fc_delta.0.weight"].data_ptr(), d["p.fc_delta.0.bias"].data_ptr(),
                                                 c.wd2p.data_ptr(), d["p.fc_delta.2.bias"].data_ptr(), c.wg1p.data_ptr(),
                                                 d["p.fc_gamma.0.bias"].data_ptr(), c.wg2p.data_ptr(), d["p.fc_gamma.2.bias"].data_ptr(),
                                                 out.data_ptr(), 1, 4, 64, 64, 64, 64, 0, hip.stream())
    finally:
        L(32)
    assert rc == HIP_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((out == _CANARY).all())


@pytest.mark.parametrize("K", [33, 64])
@pytest.mark.parametrize("C,B,Q,layout", [(128, 2, 15, "self"), (512, 3, 5, "cross"), (32, 1, 1, "self")])
def test_vector_attention_wide_composed(K, C, B, Q, layout):
    """MODE 4 in the composed form (the decoder's N_NEIGHBOR above 32): K neighbours at row stride 64 as two 32-column chunks,
    with a peaked softmax; ids past K in the rows do not change a bit of the output."""
    c = _va_case(C, B, Q, 100, seed=C * 3 + K + B, hot=True, composed=True, layout=layout, ldidx=64)
    got = _va_run(c, c.idx, nk=K)
    if K < 64:
        assert torch.equal(got, _va_run(c, _replace_masked(c, c.idx, K), nk=K)), "ids past K change the output"
    _va_expect(c, got, c.idx[..., :K], f"MODE 4 composed K={K} C={C}")


# MODE 1 + MODE 2 query counts: "xcd" -- ceil(Q / P) % 8 == 0 (the table mode's own XCD walk), partial last group where P > 1;
# "odd" -- not
def _table_q(C, imap):
    P = _group(C)
    return 16 * P - (P > 1) if imap == "xcd" else 13


def _table_case(C, B, Q, layout, seed, hot):
    """The first decoder block: every query's neighbours are the 32 anchors.  layout "y3": keys / values are the query rows
    anchor_idx[j] of the fused self projection (nsrc = Q, 3C-wide rows); "ident": a 32-row key block (k | v, 2C-wide rows) read
    through identity ids, q at the 3C stride."""
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(C=C, B=B, Q=Q, composed=True)
    c.w = _weights(C, g, hot)
    c.cxyz = torch.rand(Q, 3, generator=g) * 2 - 1          # canonical query coordinates (the hand template)
    c.axyz = torch.rand(32, 3, generator=g) * 2 - 1         # the anchors
    NS = Q if layout == "y3" else 32
    c.q, c.k, c.v = torch.randn(B, Q, C, generator=g), torch.randn(B, NS, C, generator=g), torch.randn(B, NS, C, generator=g)
    if layout == "y3":
        c.ids = torch.randperm(Q, generator=g)[:32] if Q >= 32 else torch.randint(0, Q, (32,), generator=g)
        ldq, ldk, ldv, kcol, vcol = 3 * C, 3 * C, 3 * C, C, 2 * C
    else:
        c.ids = torch.arange(32)
        ldq, ldk, ldv, kcol, vcol = 3 * C, 2 * C, 2 * C, 0, C
    c.NS, c.ldq, c.ldk, c.ldv = NS, ldq, ldk, ldv
    c.qg, c.kg, c.wc = _compose(c.w, c.q, c.k)
    c.qbuf, c.qp = _block(c.qg.reshape(B * Q, C), ldq, 0)
    c.kbuf, c.kp = _block(c.kg.reshape(B * NS, C), ldk, kcol)
    c.vbuf, c.vp = _block(c.v.reshape(B * NS, C), ldv, vcol)
    return c


def _tables_and_anchored(c):
    C, Q, B = c.C, c.Q, c.B
    d = {n: t.to(DEV).contiguous() for n, t in c.w.items()}
    nt = _fn("poem_vector_attention_table_floats")(Q, C)
    assert nt == -(-Q // _group(C)) * _group(C) * 32 * C
    tab_g = torch.full((nt,), float("nan"), device=DEV)
    tab_p = torch.full((nt,), float("nan"), device=DEV)
    ids = c.ids.to(torch.int32).to(DEV)
    cxyz, axyz = c.cxyz.to(DEV), c.axyz.to(DEV)
    wd2p, wcp, wg2p = (hip.pack_linear(t) for t in (d["p.fc_delta.2.weight"], c.wc.to(DEV), d["p.fc_gamma.2.weight"]))
    rc = _fn("poem_launch_vector_attention_tables")(cxyz.data_ptr(), axyz.data_ptr(), ids.data_ptr(), d["p.fc_delta.0.weight"].data_ptr(),
                                                    d["p.fc_delta.0.bias"].data_ptr(), wd2p.data_ptr(), d["p.fc_delta.2.bias"].data_ptr(),
                                                    wcp.data_ptr(), tab_g.data_ptr(), tab_p.data_ptr(), Q, C, hip.stream())
    assert rc == 0, rc
    out = _guarded(B * Q, C)
    rc = _fn("poem_launch_vector_attention_anchored")(ids.data_ptr(), c.qp, c.kp, c.vp, c.NS, wg2p.data_ptr(), tab_g.data_ptr(),
                                                      tab_p.data_ptr(), out.data_ptr(), B, Q, C, c.ldq, c.ldk, c.ldv, hip.stream())
    assert rc == 0, rc
    got = _unguard(out, B * Q, C, f"MODE 2 C={C} Q={Q}")
    assert torch.isfinite(tab_g).all() and torch.isfinite(tab_p).all(), "tables left unwritten"
    return got


def _table_expect(c, got, what):
    B, Q, C = c.B, c.Q, c.C
    il = c.ids.long().view(1, 1, 32).expand(B, Q, 32)
    flat = lambda t: t.reshape(B * Q, *t.shape[2:])    # noqa: E731
    kn, vn, kgn = (flat(po.index_points(t, il)) for t in (c.k, c.v, c.kg))
    xyz = c.cxyz.view(1, Q, 3).expand(B, Q, 3).reshape(B * Q, 3)
    nxyz = c.axyz.view(1, 32, 3).expand(B * Q, 32, 3)
    _va_check(got, c, flat(c.q), xyz, kn, vn, nxyz, flat(c.qg), kgn, what)


@pytest.mark.parametrize("C", [32, 64, 128, 256, 512, 1024])
@pytest.mark.parametrize("layout", ["y3", "ident"])
@pytest.mark.parametrize("imap", ["xcd", "odd"])
def test_vector_attention_anchor_tables(C, layout, imap):
    """MODE 1 (tables from the canonical query coordinates and the anchors) + MODE 2 (per sample) at every width, in both key
    layouts of the decoder's first block and both of MODE 2's item maps; peaked softmax in the XCD-walk cases."""
    B, Q = (2 if imap == "xcd" else 3), _table_q(C, imap)
    assert (-(-Q // _group(C)) % 8 == 0) == (imap == "xcd")
    c = _table_case(C, B, Q, layout, seed=C + 17 * (layout == "y3") + (imap == "xcd"), hot=imap == "xcd")
    _table_expect(c, _tables_and_anchored(c), f"MODE 1+2 C={C} {layout} {imap}")


@pytest.mark.parametrize("B,Q,layout", [(1, 799, "y3"), (2, 799, "ident"), (3, 1, "ident"), (2, 1, "y3")])
def test_vector_attention_anchor_tables_decoder_shapes(B, Q, layout):
    """MODE 1 + 2 at embed 256: the head's 799 queries and a single query."""
    c = _table_case(256, B, Q, layout, seed=B * 7 + Q, hot=True)
    _table_expect(c, _tables_and_anchored(c), f"MODE 1+2 B={B} Q={Q} {layout}")


@pytest.mark.parametrize("C,B,Q,layout,hot", [(1024, 2, 5, "rows", False), (1024, 3, 3, "self", True), (512, 2, 9, "cross", True),
                                              (128, 3, 13, "self", True)])
def test_vector_attention_split_kernel(C, B, Q, layout, hot):
    """The opt-in split-precision kernel (vecattn_split.hip, composed form) at embed 1024 and at the engine's strides."""
    c = _va_case(C, B, Q, 80, seed=C + B + Q, hot=hot, composed=True, layout=layout)
    d = c.dev
    i1, s1 = hip.pack_split_linear(d["p.fc_delta.2.weight"])
    i2, s2 = hip.pack_split_linear(c.wc.to(DEV))
    i3, s3 = hip.pack_split_linear(d["p.fc_gamma.2.weight"])
    scales = torch.cat([s1, s2, s3])
    idx_d = c.idx.to(DEV).contiguous()
    out = _guarded(B * Q, C)
    rc = _fn("poem_launch_vector_attention_split")(c.qxyz_d.data_ptr(), c.sxyz_d.data_ptr(), None, idx_d.data_ptr(), 0, c.qp, c.kp,
                                                   c.vp, c.NS, d["p.fc_delta.0.weight"].data_ptr(), d["p.fc_delta.0.bias"].data_ptr(),
                                                   i1.data_ptr(), d["p.fc_delta.2.bias"].data_ptr(), i2.data_ptr(), i3.data_ptr(),
                                                   scales.data_ptr(), out.data_ptr(), B, Q, C, c.ldq, c.ldk, c.ldv, hip.stream())
    assert rc == 0, rc
    got = _unguard(out, B * Q, C, f"split C={C}")
    _va_expect(c, got, c.idx, f"split C={C} {layout}")


# ---------------------------------------------------------------------------------------------------------------------
# cross attention
def _xattn_refs(q, k, v, heads):
    """softmax(Q K^T / sqrt(dh)) V per head: (fp64 on the device, fp32 on the CPU); q (B, NQ, C), k / v (B, NK, C)."""
    B, NQ, C = q.shape
    dh = C // heads

    def run(qq, kk, vv):
        sp = lambda t: t.view(B, -1, heads, dh).permute(0, 2, 1, 3)   # noqa: E731
        s = sp(qq) @ sp(kk).transpose(-1, -2) / math.sqrt(dh)
        return (torch.softmax(s, -1) @ sp(vv)).permute(0, 2, 1, 3).reshape(B, NQ, C)

    return run(*(t.to(DEV).double() for t in (q, k, v))), run(q.float().cpu(), k.float().cpu(), v.float().cpu())


def _xattn_op(q, k, v, heads):
    return hip.cross_attention(q.to(DEV).contiguous(), k.to(DEV).contiguous(), v.to(DEV).contiguous(), heads)


@pytest.mark.parametrize("NK,C,heads", [(1056, 32, 1), (1056, 256, 4), (2048, 256, 4), (3072, 256, 4), (3072, 32, 1),
                                        (16384, 64, 2)])
def test_cross_attention_key_chunks(NK, C, heads):
    """Key chunking: one chunk of 33 tiles, 2, 3 and 16 chunks of 32 tiles."""
    g = torch.Generator().manual_seed(NK + C)
    B = 1 if NK > 4096 else 2
    q, k, v = torch.randn(B, 33, C, generator=g) * 2, torch.randn(B, NK, C, generator=g), torch.randn(B, NK, C, generator=g)
    r64, r32 = _xattn_refs(q, k, v, heads)
    _assert_close(_xattn_op(q, k, v, heads), r64, r32, f"NK={NK} C={C} heads={heads}")


def test_cross_attention_refuses_17_key_chunks():
    """17 chunks of 32 key tiles is past the combine's 16: the launcher refuses it and the ABI reports an error."""
    B, NQ, NK, C, heads = 1, 8, 17408, 32, 1
    assert _fn("poem_cross_attention_scratch_floats")(B, NQ, NK, C, heads, 0) > 0
    q, k = torch.randn(B, NQ, C, device=DEV), torch.randn(B, NK, C, device=DEV)
    scratch = torch.empty(_fn("poem_cross_attention_scratch_floats")(B, NQ, NK, C, heads, 0), device=DEV)
    ctx = _guarded(B * NQ, C)
    rc = _fn("poem_launch_cross_attention_imgq")(q.data_ptr(), C, NQ, k.data_ptr(), k.data_ptr(), ctx.data_ptr(), B, NQ, NK, C, heads,
                                                 scratch.data_ptr(), hip.stream())
    assert rc == HIP_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((ctx == _CANARY).all())
    with pytest.raises(RuntimeError):
        hip.cross_attention(q, k, k, heads)


@pytest.mark.parametrize("C,heads", [(32, 4), (32, 2), (256, 16), (32, 1), (256, 8), (64, 1), (1024, 16), (128, 1), (512, 4),
                                     (256, 1), (1024, 4)])
@pytest.mark.parametrize("NQ", [1, 31, 32, 33])
def test_cross_attention_head_dims_and_query_tile_edges(C, heads, NQ):
    """Head dims 8 .. 256 with 1 .. 16 heads at the query-tile edges."""
    g = torch.Generator().manual_seed(C * 100 + heads * 10 + NQ)
    B, NK = 2, 256
    q, k, v = torch.randn(B, NQ, C, generator=g) * 2, torch.randn(B, NK, C, generator=g), torch.randn(B, NK, C, generator=g)
    r64, r32 = _xattn_refs(q, k, v, heads)
    _assert_close(_xattn_op(q, k, v, heads), r64, r32, f"C={C} heads={heads} NQ={NQ}")


def _kv_images(k, v):
    """K / V fragment images written by the F1 GEMM's image modes (gemm.hip output modes 1 / 2) from an identity weight with
    zero bias, which copies the rows exactly."""
    M, C = k.shape
    wp = hip.pack_linear(torch.eye(C, device=DEV))
    bias = torch.zeros(C, device=DEV)
    imgs = []
    for rows, mode in ((k, 1), (v, 2)):
        x = rows.to(DEV).contiguous()
        img = torch.empty(M * C, device=DEV)
        rc = _fn("poem_launch_gemm_segs")(x.data_ptr(), C, wp.data_ptr(), bias.data_ptr(), M, C, 0, C, 1, (_vp * 1)(img.data_ptr()),
                                          (_i * 1)(mode), hip.stream())
        assert rc == 0, rc
        imgs.append(img)
    torch.cuda.synchronize()
    return imgs


@pytest.mark.parametrize("C,heads,B,NQ,NK", [(256, 4, 2, 33, 4096), (128, 4, 3, 70, 1024), (1024, 4, 2, 5, 256), (64, 2, 2, 32, 2048)])
@pytest.mark.parametrize("shared_q", [False, True])
def test_cross_attention_decoder_image_form(C, heads, B, NQ, NK, shared_q):
    """The decoder's call: q as a column block of 2C-wide rows (NaN elsewhere), K / V images from poem_launch_gemm_segs, and
    (block 0) q_batch_rows = 0 -- every sample reads the same query rows.  Bit-identical to the operator on the same values."""
    g = torch.Generator().manual_seed(C + B + NQ + NK + shared_q)
    q = torch.randn(1 if shared_q else B, NQ, C, generator=g) * 2
    k, v = torch.randn(B, NK, C, generator=g), torch.randn(B, NK, C, generator=g)
    kimg, vimg = _kv_images(k.reshape(B * NK, C), v.reshape(B * NK, C))
    qbuf, qp = _block(q.reshape(-1, C), 2 * C, C)
    scratch = torch.empty(_fn("poem_cross_attention_scratch_floats")(B, NQ, NK, C, heads, 0), device=DEV)
    ctx = _guarded(B * NQ, C)
    if shared_q:
        rc = _fn("poem_launch_cross_attention_imgq")(qp, 2 * C, 0, kimg.data_ptr(), vimg.data_ptr(), ctx.data_ptr(), B, NQ, NK, C, heads,
                                                     scratch.data_ptr(), hip.stream())
    else:
        rc = _fn("poem_launch_cross_attention_img")(qp, 2 * C, kimg.data_ptr(), vimg.data_ptr(), ctx.data_ptr(), B, NQ, NK, C, heads,
                                                    scratch.data_ptr(), hip.stream())
    assert rc == 0, rc
    got = _unguard(ctx, B * NQ, C, "image form").view(B, NQ, C)
    qb = q.expand(B, NQ, C)
    assert torch.equal(got, _xattn_op(qb, k, v, heads)), "image form differs from the operator"
    r64, r32 = _xattn_refs(qb, k, v, heads)
    _assert_close(got, r64, r32, f"image form C={C} shared_q={shared_q}")


def _rising_keys(g, B, NQ, NK, C, heads, step):
    """Keys whose logits rise by `step` (> the lazy threshold, 8 / log2(e) = 5.5) from each 32-key tile to the next for every
    query: the running maximum moves, and the accumulators are rescaled, on every tile."""
    dh = C // heads
    q = torch.randn(B, NQ, C, generator=g) * 0.05
    k = torch.randn(B, NK, C, generator=g)
    q.view(B, NQ, heads, dh)[..., 0] = 1.0
    level = torch.arange(NK, dtype=torch.float32) // 32 * step + torch.rand(NK, generator=g)
    k.view(B, NK, heads, dh)[..., 0] = (level * math.sqrt(dh))[None, :, None]
    return q, k


@pytest.mark.parametrize("case", ["spread100", "rising", "rising_chunks", "identical"])
def test_cross_attention_hard_softmax(case):
    """Logits spanning +-100; a maximum that passes the lazy threshold in every key tile (one chunk of 33 tiles; two chunks);
    all keys identical (exactly uniform weights)."""
    g = torch.Generator().manual_seed(len(case))
    B, NQ = 2, 33
    if case == "spread100":
        NK, C, heads = 1024, 64, 1
        q = torch.randn(B, NQ, C, generator=g)
        k = torch.randn(B, NK, C, generator=g) * 40.0     # logits ~ N(0, 40^2)
    elif case.startswith("rising"):
        NK, C, heads = (1056, 256, 4) if case == "rising" else (2048, 128, 2)
        q, k = _rising_keys(g, B, NQ, NK, C, heads, 7.0)
    else:
        NK, C, heads = 3072, 128, 2
        q = torch.randn(B, NQ, C, generator=g) * 2
        k = torch.randn(B, 1, C, generator=g).expand(B, NK, C).contiguous()
    v = torch.randn(B, NK, C, generator=g)
    r64, r32 = _xattn_refs(q, k, v, heads)
    if case == "spread100":
        s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(C)
        assert float(s.max()) > 100 and float(s.min()) < -100
    _assert_close(_xattn_op(q, k, v, heads), r64, r32, case)
