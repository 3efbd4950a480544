"""Cost of ``poem_render_mesh`` next to one head forward of the same batch, timed with HIP events in one process:
32 samples x 8 views x 2 meshes (prediction + ground truth) at 256 x 256, V = 778.  The face list comes from ``--faces FILE.npy``
(MANO's closed faces on a licensed machine) or a generated closed mesh of 778 vertices / 1552 faces."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):       # (tests/util.py builds the head the way the suite does)
    sys.path.insert(0, _p)
import poem_v2_amd as pk  # noqa: E402


def generated_mesh(nverts=778):
    """A closed ellipsoid of a hand's size with exactly `nverts` vertices: a latitude / longitude grid of rings plus two poles."""
    rings, seg = 97, 8                                     # 97 * 8 + 2 = 778
    assert rings * seg + 2 == nverts
    th = np.linspace(0, np.pi, rings + 2)[1:-1]
    ph = np.arange(seg) * 2 * np.pi / seg
    v = [[0, 0, 1.0]] + [[np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)] for t in th for p in ph] + [[0, 0, -1.0]]
    f = [[0, 1 + s, 1 + (s + 1) % seg] for s in range(seg)]
    for r in range(rings - 1):
        for s in range(seg):
            a, b = 1 + r * seg + s, 1 + r * seg + (s + 1) % seg
            f += [[a, a + seg, b], [b, a + seg, b + seg]]
    last = 1 + (rings - 1) * seg
    f += [[nverts - 1, last + (s + 1) % seg, last + s] for s in range(seg)]
    return np.array(v) * [0.04, 0.03, 0.09], np.array(f, dtype=np.int32)


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(steps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--faces", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    mesh, faces = generated_mesh()
    if a.faces:
        faces = np.load(a.faces).astype(np.int32)
    views = [a.views] * a.batch
    b = pk.inputs.synthetic_batch(views, seed=0)
    K, T = b["img_metas"]["cam_intr"].to(dev), b["img_metas"]["cam_extr"].to(dev)
    centre = b["reference_joints"][:, 9:10].to(dev)
    verts = torch.stack([torch.tensor(mesh, dtype=torch.float32, device=dev)[None] + centre,
                         torch.tensor(mesh, dtype=torch.float32, device=dev)[None] + centre + 0.004]).contiguous()
    bg = torch.randint(0, 256, (sum(views), a.size, a.size, 3), dtype=torch.uint8, device=dev)
    r = pk.MeshRenderer(faces, dev)
    fid = r.render(verts, K, T, views, background=bg, return_face_id=True)[1]
    covered = float((fid >= 0).float().mean())
    t_render = timed(lambda: r.render(verts, K, T, views, background=bg), a.warmup, a.steps)
    from util import build_hip_head
    spec = dict(embed=256, nsample=4096, views=views, seed=0, parametric=False)
    head = build_hip_head(spec, dev)
    feat, rj = b["mlvl_feat"].to(dev), b["reference_joints"].to(dev)
    metas = dict(b["img_metas"])
    metas["cam_intr"], metas["cam_extr"] = K, T
    with torch.no_grad():
        t_head = timed(lambda: head(feat, metas, rj), a.warmup, a.steps)
    print(json.dumps({"samples": a.batch, "views": a.views, "meshes": 2, "image": a.size, "nverts": 778, "nfaces": int(len(faces)),
                      "covered_pixel_share": round(covered, 4), "render_ms": round(t_render, 4), "head_forward_ms_embed256": round(t_head, 4),
                      "render_over_head": round(t_render / t_head, 4)}))


if __name__ == "__main__":
    main()
