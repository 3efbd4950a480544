"""Kernels on batch-scaled tensors past 2 GiB and 4 GiB (include/poem_hip.h "Size limits", DESIGN.md "Offsets past 4 GiB").

Several kernels read through one buffer descriptor with 32-bit byte offsets; an offset that wraps stays inside the same
allocation, so the failure is a plausible wrong answer (sample b reading the rows of sample b - 256), not a fault.  Each case
here runs a HIP operator on a tensor past the limit and compares chosen rows -- both sides of the 2^31- and 2^32-byte
offsets, the first and the last rows -- with a float64 reference of those rows only.  Inputs are seeded random data generated
on the device, so no checked row holds the data of the row its wrapped offset would alias.  Where the library refuses a size
it says so (POEM_E_UNSUPPORTED), and the test asserts the refusal.  Every case stays below 24 GiB of device memory."""
import ctypes
import math

import pytest
import torch

import poem_oracle as po
from poem_v2_amd import hip
from util import build_hip_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GIB = 1 << 30
PEAK_BUDGET = 24 * GIB


@pytest.fixture(autouse=True)
def _memory_budget():
    assert torch.cuda.is_available(), "these tests must run on the GPU box"
    hip.lib()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()          # (what earlier tests of the session still hold)
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak device memory of the test {peak / GIB:.2f} GiB")
    torch.cuda.empty_cache()
    assert peak <= PEAK_BUDGET, peak


def _randn(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.randn(shape, generator=g, device=DEV)
    return t.mul_(scale) if scale != 1.0 else t


def _rows_across(n, row_bytes):
    """Row ids on both sides of the 2^31- and 2^32-byte offsets of a (n, row_bytes) tensor, plus its first and last rows."""
    rows = {0, 1, n - 2, n - 1}
    for edge in (1 << 31, 1 << 32):
        r = edge // row_bytes
        rows.update(range(r - 2, r + 3))
    rows = sorted(r for r in rows if 0 <= r < n)
    assert any(r * row_bytes >= (1 << 32) for r in rows)
    return torch.tensor(rows, device=DEV)


def _md(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def _act(t, act):
    return [t, torch.relu(t), torch.nn.functional.gelu(t)][act]


def _is_unsupported(exc):
    return f"code {hip.POEM_E_UNSUPPORTED}," in str(exc)


# ---- GEMM ------------------------------------------------------------------------------------------------------------------
# K = 1024: X, Y and the residual each hold 4.3 GB (rows past 2^32 bytes from row 1048576 on); a ragged last row tile.
M_K1024 = (1 << 32) // (1024 * 4) + 4099


@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm_rows_past_4gib_k1024(act):
    M, N, K = M_K1024, 1024, 1024
    x = _randn((M, K), 11 + act)
    w = _randn((N, K), 12 + act, 1.0 / math.sqrt(K))
    b = _randn((N,), 13 + act)
    r = _randn((M, N), 14 + act)
    rows = _rows_across(M, K * 4)
    xr = x[rows].double()
    ref = _act(xr @ w.double().T + b.double(), act) + r[rows].double()
    y = hip.gemm(x, hip.pack_linear(w), N, bias=b, residual=r, act=act)
    assert _md(y[rows], ref) < 2e-5
    del y, r
    y = hip.gemm_ex(x, hip.pack_linear(w), M, N, K, bias=b, act=act)        # the operands-from-L2 entry point, row-major
    assert _md(y[rows], _act(xr @ w.double().T + b.double(), act)) < 2e-5


def test_gemm_rows_past_4gib_k256_and_split_refusal():
    # K = 256: 4.3 M rows of 1 KiB (the panel kernel's width), N = 256
    M, N, K = (1 << 32) // (256 * 4) + 3001, 256, 256
    x = _randn((M, K), 21)
    w = _randn((N, K), 22, 1.0 / math.sqrt(K))
    b = _randn((N,), 23)
    r = _randn((M, N), 24)
    rows = _rows_across(M, K * 4)
    y = hip.gemm(x, hip.pack_linear(w), N, bias=b, residual=r, act=1)
    ref = torch.relu(x[rows].double() @ w.double().T + b.double()) + r[rows].double()
    assert _md(y[rows], ref) < 2e-5
    del y, r
    # the split-precision panel GEMM addresses X through one descriptor: refused past 4 GiB of X, never a wrong answer
    with pytest.raises(RuntimeError) as e:
        hip.gemm_split(x, w, bias=b)
    assert _is_unsupported(e.value), str(e.value)


# ---- cross attention -------------------------------------------------------------------------------------------------------
def _xattn_ref(q, k, v, heads, s):
    """float64 softmax attention of sample s (test_hip_parity.test_cross_attention's reference)."""
    C = q.shape[-1]
    dh = C // heads
    sp = lambda t: t[s].double().cpu().view(-1, heads, dh).permute(1, 0, 2)   # noqa: E731
    a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(dh), -1)
    return (a @ sp(v)).permute(1, 0, 2).reshape(-1, C)


@pytest.mark.parametrize("C,heads,merged", [(1024, 4, False), (256, 4, True)])
def test_cross_attention_largest_accepted_batch_and_refusal(C, heads, merged):
    """The K / V images are addressed with 32-bit signed offsets: each may hold up to 2 GiB.  The largest batch under that
    (127 samples at C = 1024, 511 at C = 256, NK = 4096) must be exact in its last samples, whose key tiles sit just below
    2^31 bytes; one more sample must be refused."""
    NQ, NK = 8, 4096
    B = (1 << 31) // (NK * C * 4) - 1
    assert hip.lib().poem_cross_attention_scratch_bytes(B, NQ, NK, C, heads) > 0
    q = _randn((B, NQ, C), 31 + C, 2.0)
    k = _randn((B, NK, C), 32 + C)
    v = _randn((B, NK, C), 33 + C)
    out = hip.cross_attention(q, k, v, heads, merged=merged)
    for s in (0, 1, B // 2, B // 2 + 1, B - 2, B - 1):
        assert _md(out[s], _xattn_ref(q, k, v, heads, s)) < 2e-5, s
    del q, k, v, out
    torch.cuda.empty_cache()
    B += 1        # images of exactly 2^31 bytes
    q, k = torch.empty(B, NQ, C, device=DEV), torch.empty(B, NK, C, device=DEV)
    fn = hip.lib().poem_cross_attention_merged if merged else hip.lib().poem_cross_attention
    scratch = torch.empty(16, dtype=torch.uint8, device=DEV)     # (the size is refused before the scratch is looked at)
    rc = fn(q.data_ptr(), k.data_ptr(), k.data_ptr(), q.data_ptr(), B, NQ, NK, C, heads, scratch.data_ptr(), 16, hip.stream())
    assert rc == hip.POEM_E_UNSUPPORTED, rc


# ---- vector attention ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [None, 48])
def test_vector_attention_samples_past_4gib(nk):
    """B = 260 samples of 4096 value rows at C = 1024: v holds 4.4 GB, samples 128 and 256 start at 2^31 and 2^32 bytes.
    nk=None: the 32-column kernel; nk=48: MODE 4 (two 32-column chunks, online softmax)."""
    B, NS, C, Q = 260, 4096, 1024, 4
    K = 32 if nk is None else nk
    g = torch.Generator(device=DEV).manual_seed(41 + K)
    qxyz = torch.rand(B, Q, 3, generator=g, device=DEV) * 2 - 1
    sxyz = torch.rand(B, NS, 3, generator=g, device=DEV) * 2 - 1
    # distinct random neighbour ids per (sample, query)
    idx = torch.rand(B, Q, NS, generator=g, device=DEV).topk(K, dim=-1).indices.int().contiguous()
    q = _randn((B, Q, C), 42)
    k = _randn((B, NS, C), 43)
    v = _randn((B, NS, C), 44)
    w = {}
    for i, (n, shp) in enumerate((("fc_delta.0", (C, 3)), ("fc_delta.2", (C, C)), ("fc_gamma.0", (C, C)), ("fc_gamma.2", (C, C)))):
        w["p." + n + ".weight"] = _randn(shp, 50 + i, 1.0 / math.sqrt(shp[1]))
        w["p." + n + ".bias"] = _randn((shp[0],), 60 + i, 0.1)
    out = hip.vector_attention(qxyz, sxyz, None, idx, q, k, v, w["p.fc_delta.0.weight"], w["p.fc_delta.0.bias"],
                               hip.pack_linear(w["p.fc_delta.2.weight"]), w["p.fc_delta.2.bias"],
                               hip.pack_linear(w["p.fc_gamma.0.weight"]), w["p.fc_gamma.0.bias"],
                               hip.pack_linear(w["p.fc_gamma.2.weight"]), w["p.fc_gamma.2.bias"], nk=nk)
    wd = {key: t.double().cpu() for key, t in w.items()}
    for s in (0, 127, 128, 255, 256, 259):
        ik = idx[s : s + 1].long()
        gather = lambda t: po.index_points(t[s : s + 1].double().cpu(), ik.cpu())   # noqa: E731
        ref = po._vec_attn_core(wd, "p.", q[s : s + 1].double().cpu(), gather(k), gather(v),
                                qxyz[s : s + 1].double().cpu()[:, :, None] - gather(sxyz), C)
        assert _md(out[s], ref[0]) < 5e-5, s


# ---- whole path ------------------------------------------------------------------------------------------------------------
def test_whole_path_refuses_batches_past_the_attention_limit():
    """POEM-huge (C = 1024, 4096 basis points): 128 samples fill the cross attention's 2 GiB images; the forwards refuse
    such batches up front (POEM_E_UNSUPPORTED) instead of failing -- or computing -- part way.  127 is accepted."""
    spec = dict(embed=1024, nsample=4096, parametric=False, nblocks=1, seed=7)
    head = build_hip_head(spec, DEV)
    eng = head._engine_for(torch.device(DEV))
    L = hip.lib()
    for B in (128, 260):
        need = L.poem_workspace_bytes(eng.handle, B, B)
        print(f"B = {B}: poem_workspace_bytes = {need / GIB:.1f} GiB (refused: no workspace allocated)")
        dummy = torch.zeros(64, device=DEV)
        p = dummy.data_ptr()
        rc = L.poem_decoder_forward(eng.handle, p, p, p, p, B, p, None, None, p, 16, hip.stream())
        assert rc == hip.POEM_E_UNSUPPORTED, rc
        offs = (ctypes.c_int32 * (B + 1))(*range(B + 1))
        rc = L.poem_head_forward(eng.handle, p, p, p, offs, B, p, 256, 256, p, None, None, p, 16, hip.stream())
        assert rc == hip.POEM_E_UNSUPPORTED, rc
    # 127 samples pass the size check and stop at the (deliberately tiny) workspace
    rc = L.poem_decoder_forward(eng.handle, p, p, p, p, 127, p, None, None, p, 16, hip.stream())
    assert rc == -2, rc       # POEM_E_WORKSPACE
