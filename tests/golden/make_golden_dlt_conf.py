"""Golden data for the confidence-aware DLT from the upstream reference (build container only, like make_golden.py):
the reference's own ``triangulate_dlt`` (lib/utils/triangulation.py:111-148), imported by path, on seeded cases at the release
geometry -- 21 joints, 2..10 views per sample, ragged, cameras and joints from ``synthetic_batch`` as dlt.npz draws them.

Every input is an fp32 value and is handed to upstream as float64, so the recorded answer is the fp64 SVD's, not a float32
SVD's own round-off.  Upstream does not return how many cameras it used: its ``triangulate_one_point_dlt`` is wrapped for the
run and the length of each point set noted.  Per case: uv (BN,21,2), conf (BN,21), K (BN,3,3), T (BN,4,4) master->camera (the
``Extrs`` argument), E = camera->master, X (B,21,3) the joints that were projected, out (B,21,3) float64, count (B,21).

  all       (a) every confidence above the threshold 0.5; noise-free 2-D points
  occluded  (b) one or two views per sample with low confidence and 2-D points far off; the others noise-free.  ``plain`` is
            upstream's unweighted ``batch_triangulate_dlt_torch`` on the same points: more than 1 cm from X on every sample
  carry     (c) per sample a joint where one camera clears 0.5, so the threshold drops -- and later joints whose selection
            differs from a fresh 0.5 because upstream's lowered threshold carries over (asserted here; ``count_fresh`` records
            the per-joint counts of single-joint calls)
  high      (c') threshold 0.93 against confidences in (0.3, 0.95): many drops
  zero, neg (d) threshold 0 (one confidence exactly 0: 0 > 0 is false, that camera is left out) and threshold -0.1

Every joint of every case ends with at least two selected cameras, two of whose rays meet at sin(angle) > 0.3 (asserted).

  python tests/golden/make_golden_dlt_conf.py   ->  tests/golden/dlt_conf.npz"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path[:0] = [ROOT, GOLDEN]
sys.dont_write_bytecode = True

import ref_harness as rh  # noqa: E402
from poem_v2_amd.inputs import synthetic_batch  # noqa: E402

BAR = 5e-6            # metres: tests/test_dlt.py's bar for the plain DLT against the reference
MIN_SIN = 0.3


def upstream():
    spec = importlib.util.spec_from_file_location("ref_tri", os.path.join(rh.REF_ROOT, "lib", "utils", "triangulation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rig(views, seed):
    """fp32 K, E, T = inv(E), X of the synthetic rig and the fp64 projection of X into every view (BN,21,2)."""
    b = synthetic_batch(views, seed=seed)
    K, E = b["img_metas"]["cam_intr"], b["img_metas"]["cam_extr"]
    T = torch.linalg.inv(E)
    X = b["reference_joints"]
    vs = np.repeat(np.arange(len(views)), views)
    K64, T64, X64 = K.double().numpy(), T.double().numpy(), X.double().numpy()[vs]
    pc = np.einsum("nrc,njc->njr", T64[:, :3, :3], X64) + T64[:, None, :3, 3]
    q = np.einsum("nrc,njc->njr", K64, pc)
    return K.numpy(), E.numpy(), T.numpy(), X.numpy(), q[..., :2] / q[..., 2:]


def run_upstream(mod, uv, conf, K, T, views, thr):
    """Per sample, as a caller's loop would: upstream's triangulate_dlt on float64 copies; the cameras it used per joint."""
    offs = np.concatenate([[0], np.cumsum(views)])
    outs, counts = [], []
    inner = mod.triangulate_one_point_dlt
    try:
        def noted(points_2d_set, Ks, Extrs):
            counts[-1].append(len(points_2d_set))
            return inner(points_2d_set, Ks, Extrs)
        mod.triangulate_one_point_dlt = noted
        for s, e in zip(offs[:-1], offs[1:]):
            counts.append([])
            outs.append(mod.triangulate_dlt(uv[s:e].astype(np.float64), conf[s:e].astype(np.float64), K[s:e].astype(np.float64),
                                            T[s:e].astype(np.float64), thr))
    finally:
        mod.triangulate_one_point_dlt = inner
    return np.stack(outs), np.asarray(counts, dtype=np.int32)


def fresh_counts(mod, uv, conf, K, T, views, thr):
    """What each joint would select if it started from `thr` itself: single-joint calls of upstream's function."""
    offs = np.concatenate([[0], np.cumsum(views)])
    out = np.zeros((len(views), uv.shape[1]), dtype=np.int32)
    for j in range(uv.shape[1]):
        _, c = run_upstream(mod, uv[:, j:j + 1], conf[:, j:j + 1], K, T, views, thr)
        out[:, j] = c[:, 0]
    assert offs[-1] == uv.shape[0]
    return out


def check_rays(conf, count, E, X, views, thr_final):
    """Every joint: the cameras with conf > its final threshold are `count` many, >= 2, and two of their rays are well apart."""
    offs = np.concatenate([[0], np.cumsum(views)])
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        centres = E[s:e, :3, 3].astype(np.float64)
        for j in range(X.shape[1]):
            sel = np.where(conf[s:e, j].astype(np.float64) > thr_final[b, j])[0]
            assert len(sel) == count[b, j] >= 2, (b, j, sel, count[b, j])
            d = X[b, j].astype(np.float64) - centres[sel]
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            best = max(np.linalg.norm(np.cross(d[a], d[c])) for a in range(len(sel)) for c in range(a + 1, len(sel)))
            assert best > MIN_SIN, (b, j, sel, best)


def final_thresholds(conf, views, thr):
    """The threshold each joint ends with (the lowering loop alone, for check_rays)."""
    offs = np.concatenate([[0], np.cumsum(views)])
    out = np.zeros((len(views), conf.shape[1]))
    for b, (s, e) in enumerate(zip(offs[:-1], offs[1:])):
        t = float(thr)
        for j in range(conf.shape[1]):
            while t > 0 and (conf[s:e, j].astype(np.float64) > t).sum() <= 1:
                t -= 0.05
            out[b, j] = t
    return out


def build():
    """-> {name: array} of the fixture (tests/test_dlt_confidence.py calls this to check that dlt_conf.npz regenerates)."""
    mod = upstream()
    rec, meta = {}, {}

    def record(name, views, thr, uv, conf, K, E, T, X, **extra):
        uv, conf = uv.astype(np.float32), conf.astype(np.float32)
        out, count = run_upstream(mod, uv, conf, K, T, views, thr)
        check_rays(conf, count, E, X, views, final_thresholds(conf, views, thr))
        for k, v in dict(uv=uv, conf=conf, K=K, E=E, T=T, X=X, out=out, count=count, **extra).items():
            rec[f"{name}.{k}"] = v
        meta[name] = dict(views=[int(v) for v in views], threshold=thr)
        print(f"{name}: views {views} thr {thr}  cameras used {count.min()}..{count.max()}  "
              f"max |out - X| = {np.abs(out - X).max():.3e} m")
        return out, count

    # (a) every confidence above the threshold, noise-free points
    views = [3, 10, 2, 6, 8]
    K, E, T, X, clean = rig(views, 51)
    rng = np.random.RandomState(151)
    out, count = record("all", views, 0.5, clean, rng.uniform(0.6, 0.95, clean.shape[:2]), K, E, T, X)
    assert (count == np.asarray(views)[:, None]).all()
    assert np.abs(out - X).max() < BAR

    # (b) occluded views: low confidence, points far off; the rest noise-free
    views = [4, 7, 10, 5, 3, 9]
    K, E, T, X, clean = rig(views, 52)
    rng = np.random.RandomState(152)
    uv, conf = clean.copy(), rng.uniform(0.6, 0.95, clean.shape[:2])
    offs = np.concatenate([[0], np.cumsum(views)])
    for s, n in zip(offs[:-1], views):
        for v in rng.choice(np.arange(1, n), size=2 if n >= 6 else 1, replace=False):      # never the master view
            ang = rng.uniform(0, 2 * np.pi)
            uv[s + v] += rng.uniform(90.0, 130.0) * np.array([np.cos(ang), np.sin(ang)]) + rng.normal(0, 6.0, (21, 2))
            conf[s + v] = rng.uniform(0.05, 0.3, 21)
    uv32 = uv.astype(np.float32)
    plain = np.concatenate([mod.batch_triangulate_dlt_torch(
        torch.from_numpy(uv32[s:e].astype(np.float64))[None], torch.from_numpy(K[s:e].astype(np.float64))[None],
        torch.from_numpy(T[s:e].astype(np.float64))[None]).numpy() for s, e in zip(offs[:-1], offs[1:])])
    miss = np.linalg.norm(plain - X, axis=-1)
    assert miss.min() > 0.01, miss.min()                  # upstream's unweighted DLT: > 1 cm off on EVERY joint
    out, count = record("occluded", views, 0.5, uv, conf, K, E, T, X, plain=plain)
    assert (count < np.asarray(views)[:, None]).all()
    assert np.abs(out - X).max() < BAR
    print(f"occluded: unweighted DLT misses by {miss.min() * 100:.2f}..{miss.max() * 100:.2f} cm")

    # (c) the threshold drops at one joint and stays lowered for the sample's following joints
    views = [5, 3, 8, 4]
    K, E, T, X, clean = rig(views, 53)
    rng = np.random.RandomState(153)
    uv = clean + 1.5 * rng.standard_normal(clean.shape)
    conf = rng.uniform(0.6, 0.95, clean.shape[:2])
    offs = np.concatenate([[0], np.cumsum(views)])
    for s, n in zip(offs[:-1], views):
        j0 = rng.randint(2, 8)
        conf[s:s + n, j0] = rng.uniform(0.05, 0.25, n)
        conf[s, j0] = rng.uniform(0.7, 0.9)                          # the master alone clears 0.5 ...
        conf[s + 1 + rng.randint(0, 2), j0] = rng.uniform(0.36, 0.44)  # ... 0.45 still leaves one, 0.40 finds this one
        for j in range(j0 + 1, 21):                                  # later joints: views between the two thresholds
            for v in range(2, n):
                if rng.rand() < 0.35:
                    conf[s + v, j] = rng.uniform(0.41, 0.49)
    conf32 = conf.astype(np.float32)
    fresh = fresh_counts(mod, uv.astype(np.float32), conf32, K, T, views, 0.5)
    out, count = record("carry", views, 0.5, uv, conf, K, E, T, X, count_fresh=fresh)
    differs = count != fresh
    assert differs.any(axis=1).all(), "a sample without a carried-over selection"     # the point of the case
    first = differs.argmax(axis=1)
    assert (final_thresholds(conf32, views, 0.5)[np.arange(len(views)), first] < 0.45).all()
    print(f"carry: joints whose selection differs from a fresh threshold, per sample: {differs.sum(axis=1).tolist()}")

    # (c') a high threshold: many drops.  Any two cameras may end up as the selected pair, so at most four views of the ring of
    # eight: no two of them face each other
    views = [4, 2, 3, 4]
    K, E, T, X, clean = rig(views, 54)
    rng = np.random.RandomState(154)
    uv = clean + 1.5 * rng.standard_normal(clean.shape)
    conf = rng.uniform(0.3, 0.95, clean.shape[:2])
    first = np.concatenate([[0], np.cumsum(views)])[:-1]
    conf[first] = rng.uniform(0.5, 0.95, (len(views), 21))           # views 0 and 1 stay usable
    conf[first + 1] = rng.uniform(0.5, 0.95, (len(views), 21))
    record("high", views, 0.93, uv, conf, K, E, T, X)

    # (d) threshold <= 0
    views = [4, 2, 7]
    K, E, T, X, clean = rig(views, 55)
    rng = np.random.RandomState(155)
    uv = clean + 1.5 * rng.standard_normal(clean.shape)
    conf = rng.uniform(0.02, 0.95, clean.shape[:2])
    conf[3, 5] = 0.0                                                 # 0 > 0 is false: upstream leaves this camera out
    out, count = record("zero", views, 0.0, uv, conf, K, E, T, X)
    assert count[0, 5] == 3 and count.sum() == 21 * sum(views) - 1
    conf[3, 5] = 0.0
    out, count = record("neg", views, -0.1, uv, conf, K, E, T, X)
    assert (count == np.asarray(views)[:, None]).all()

    rec["meta"] = np.frombuffer(json.dumps(dict(cases=meta, bar=BAR)).encode(), dtype=np.uint8)
    return rec


if __name__ == "__main__":
    rec = build()
    path = os.path.join(GOLDEN, "dlt_conf.npz")
    np.savez_compressed(path, **rec)
    print(f"dlt_conf: {len(rec) - 1} arrays, {os.path.getsize(path) / 1e3:.0f} kB")
