"""Cost of neighbour counts above 32 at the medium shape (C = 256, 799 queries, 4096 basis points, B = 32): one vector
attention launch and one neighbour search at K = 64 vs K = 32, and whole-forward samples/s at 32 / 32 vs 64 / 64 (N_NEIGHBOR /
N_NEIGHBOR_QUERY).  Development tool for DESIGN / LABNOTES (not the bench contract).  Prints one JSON line."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

from poem_v2_amd import hip  # noqa: E402

DEV = "cuda:0"


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def main():
    B, Q, S, C = 32, 799, 4096, 256
    g = torch.Generator(device=DEV).manual_seed(0)
    qxyz = (torch.rand(B, Q, 3, device=DEV, generator=g) - 0.5) * 0.4
    sxyz = (torch.rand(B, S, 3, device=DEV, generator=g) - 0.5) * 0.4
    res = {}
    # ---- neighbour search (cross: 799 queries over 4096 basis points)
    t32 = timeit(lambda: hip.knn(qxyz, sxyz))
    t64 = timeit(lambda: hip.knn(qxyz, sxyz, k=64))
    res["knn_ms_k32"], res["knn_ms_k64"], res["knn_ratio"] = t32, t64, t64 / t32
    # ---- vector attention (plain form, cross shape)
    q = torch.randn(B, Q, C, device=DEV, generator=g)
    k = torch.randn(B, S, C, device=DEV, generator=g)
    v = torch.randn(B, S, C, device=DEV, generator=g)
    w = [torch.randn(C, 3, device=DEV, generator=g) / math.sqrt(3), torch.randn(C, device=DEV, generator=g) * 0.1]
    for _ in range(3):
        w += [hip.pack_linear(torch.randn(C, C, device=DEV, generator=g) / math.sqrt(C)), torch.randn(C, device=DEV, generator=g) * 0.1]
    i32 = hip.knn(qxyz, sxyz)
    i64 = hip.knn(qxyz, sxyz, k=64)
    v32 = timeit(lambda: hip.vector_attention(qxyz, sxyz, None, i32, q, k, v, *w))
    v64 = timeit(lambda: hip.vector_attention(qxyz, sxyz, None, i64, q, k, v, *w, nk=64))
    res["vecattn_ms_k32"], res["vecattn_ms_k64"], res["vecattn_ratio"] = v32, v64, v64 / v32
    # ---- whole forward
    from util import batch_to, build_hip_head, case_setup
    for kn in (32, 64):
        spec = dict(embed=C, nsample=S, views=[8] * B, seed=3, parametric=False, knn=kn, knn_query=kn)
        batch = case_setup(spec)[3]
        head = build_hip_head(spec, DEV)
        feat, metas, rj = batch_to(batch, DEV)
        with torch.no_grad():
            ms = timeit(lambda: head(feat, metas, rj), n=20)
        res[f"forward_ms_{kn}_{kn}"] = ms
        res[f"samples_per_s_{kn}_{kn}"] = B / ms * 1e3
        del head
    print(json.dumps(res))


if __name__ == "__main__":
    main()
