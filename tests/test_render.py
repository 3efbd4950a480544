"""The renderer's kernels (csrc/render.hip) on the GPU against the fp64 restatement of tests/test_render_host.py.

Stable pixels.  A pixel is compared when the restatement gives the same hit or miss at the pixel and at its four samples offset by
(+-0.01, +-0.01) px, and the same depth to within the depth bar once the slope of the pixel's own face over the offset is allowed for
(test_render_host.ref_stable): silhouettes and occlusion boundaries drop out, interior edges stay.  The share of covered pixels that are
not stable is asserted <= 1 % in every case.  Computed with the restatement alone on the CPU before the first GPU run: see UNSTABLE.

Depth bar (per pixel), from the fp32 arithmetic in front of and inside the barycentric divide z = (E0 + E1 + E2) / (E0/z0 + E1/z1 + E2/z2):
  * the divide, the three products and two sums of each side, 1/z_i and the vertex z (three fma and an add): <= 16 roundings of relative
    size 2^-24 on z itself                                                                      -> 16 * 2^-24 * z
  * the projected vertices differ from the fp64 ones by eps_pos px: the camera-frame coordinate carries 6 roundings (rounded inverse
    extrinsic, three products / fma, the add) of its absolute term sum m, so d(x, z) <= 6 * 2^-24 * m and
    du <= f / z * (1 + |x / z|) * 6 * 2^-24 * m + 4 * 2^-24 * (|u - c| + |c|) (the divide, the product, the add); the edge
    functions add 8 * 2^-24 * d of a face's diameter d in px (their products are at most d^2 wide against an area of the order d^2).
    Moving the sample point by eps_pos against a face changes its depth by |grad z| * eps_pos, and may hand the pixel to the
    neighbour across an interior edge, whose plane is within |grad z'| * eps_pos there     -> eps_pos * (|grad z| + |grad z'|)
    with the restatement's face at the pixel and the steepest of its faces at the four offset samples (nothing the kernel returns
    enters the bar).
Largest observed on an MI355X (2026-10-17, every case prints its figures): depth error 2.5e-7 m (case `duplicate`), 0.24 of the pixel's
bar at most (case `F257`); eps_pos 1.4e-4 .. 3.0e-4 px (1.4e-3 for the image-sized faces of `soup`); colour steps 0 or 1.  LABNOTES.md,
"Renderer"."""
import functools
import os

import numpy as np
import pytest
import torch

import poem_v2_amd as pk
from poem_v2_amd import hip
from test_render_host import DELTA, STABILITY_OFFSETS, geodesic_sphere, ref_raster, ref_skeleton, ref_stable, ref_vertices  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
RADII = np.array([0.05, 0.04, 0.035])                 # 25 px at f = 300, z = 0.6
FOCAL = 300.0


def _rot(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _cameras(n, H, W, rng, shift=(0.0, 0.0), focal=FOCAL):
    K = np.zeros((n, 3, 3), np.float32)
    T = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        K[i] = [[focal, 0, (W - 1) / 2 + shift[0] + rng.uniform(-2, 2)], [0, focal, (H - 1) / 2 + shift[1] + rng.uniform(-2, 2)], [0, 0, 1]]
        T[i] = np.eye(4)
        T[i, :3, :3] = _rot(rng.uniform(-0.02, 0.02, 3) + 1e-9)
        T[i, :3, 3] = rng.uniform(-0.008, 0.008, 3)
    return K, T


def _ellipsoids(B, rng, occluder, freq=6):
    sv, sf = geodesic_sphere(freq)
    verts = []
    for _ in range(B):
        c = np.array([0.0, 0.0, 0.6]) + rng.uniform(-0.004, 0.004, 3)
        v = (sv * RADII) @ _rot(rng.uniform(-1, 1, 3)).T + c
        if occluder:
            v = np.concatenate([v, (sv * RADII * 0.7) @ _rot(rng.uniform(-1, 1, 3)).T + c + [0.035, 0.012, -0.12]])
        verts.append(v)
    faces = np.concatenate([sf, sf + len(sv)]) if occluder else sf
    return np.stack(verts).astype(np.float32), faces.astype(np.int32)


def _soup(rng):
    """300 faces on one tile of a 64 x 64 image: 40 that cover the whole image at depths 0.5 .. 0.7 -- the nearest of them LAST in index
    order, behind the 256 entries a list holds -- and 260 small ones inside tile (1, 1), all farther than every large face."""
    tri, z = [], []
    big = rng.permutation(np.linspace(0.5, 0.7, 40))
    small_z = 0.8
    order = list(big[big > big.min()][:39])
    for d in order[:20]:
        tri.append([[-400 + rng.uniform(-9, 9), -300], [500, -300 + rng.uniform(-9, 9)], [30 + rng.uniform(-9, 9), 600]]), z.append([d] * 3)
    for _ in range(260):
        p = rng.uniform(17, 30, 2)
        tri.append([p, p + rng.uniform(0.8, 2.5, 2) * [1, 0.2], p + rng.uniform(0.8, 2.5, 2) * [0.1, 1]]), z.append(list(small_z + rng.uniform(0, 0.05, 3)))
    for d in order[20:] + [big.min()]:
        tri.append([[-400 + rng.uniform(-9, 9), -300], [500, -300 + rng.uniform(-9, 9)], [30 + rng.uniform(-9, 9), 600]]), z.append([d] * 3)
    uv, z = np.array(tri, np.float64).reshape(-1, 2), np.array(z, np.float64).reshape(-1)
    verts = np.stack([(uv[:, 0] - 31.5) / FOCAL * z, (uv[:, 1] - 31.5) / FOCAL * z, z], axis=1)
    return verts[None].astype(np.float32), np.arange(900, dtype=np.int32).reshape(300, 3)


CASES = {
    #                views      H    W   what
    "64_occluded":  ([1],       64,  64, dict(occluder=True)),
    "50x70_ragged": ([1, 3, 2], 50,  70, dict()),
    "256_zeroarea": ([1],       256, 256, dict(extra="zero_area")),
    "half_outside": ([1],       64,  64, dict(shift=(-30.0, 6.0))),
    "behind_near":  ([1],       64,  64, dict(near="vertex")),
    # partial meshes show their cut edges: larger on screen (f = 600: 50 px) and coarser, so that the cap of 1 % holds
    "F1":           ([1],       128, 128, dict(nfaces=1, freq=1, focal=600.0)),
    "F256":         ([1],       128, 128, dict(nfaces=256, freq=4, focal=600.0)),
    "F257":         ([1],       128, 128, dict(nfaces=257, freq=4, focal=600.0)),
    "duplicate":    ([1],       64,  64, dict(extra="duplicate")),
    "soup":         ([1],       64,  64, dict(soup=True)),
}
# share of covered pixels that are not stable, from the restatement alone (CPU, before the first GPU run); cap 1 %
UNSTABLE = {"64_occluded": "14 / 1761 = 0.80 %", "50x70_ragged": "50 / 9073 = 0.55 %", "256_zeroarea": "8 / 1490 = 0.54 %",
            "half_outside": "5 / 745 = 0.67 %", "behind_near": "5 / 1505 = 0.33 %", "F1": "2 / 977 = 0.21 %", "F256": "18 / 5591 = 0.32 %",
            "F257": "24 / 5419 = 0.44 %", "duplicate": "5 / 1528 = 0.33 %", "soup": "0 / 4096"}


@functools.lru_cache(maxsize=None)
def scene(name):
    views, H, W, opt = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    B, BN = len(views), sum(views)
    K, T = _cameras(BN, H, W, rng, opt.get("shift", (0.0, 0.0)), opt.get("focal", FOCAL))
    if opt.get("soup"):
        verts, faces = _soup(rng)
        K[:] = [[FOCAL, 0, 31.5], [0, FOCAL, 31.5], [0, 0, 1]]
        T[:] = np.eye(4)
    else:
        verts, faces = _ellipsoids(B, rng, opt.get("occluder", False), opt.get("freq", 6))
    near = 0.01
    if "nfaces" in opt:
        # the first faces in generation order: whole patches of the icosahedron; the single face is the one nearest the camera
        faces = faces[:opt["nfaces"]] if opt["nfaces"] > 1 else faces[[np.argmin(verts[0, faces, 2].sum(1))]]
    if opt.get("extra") == "zero_area":
        faces = np.concatenate([faces, [[5, 5, 9]]]).astype(np.int32)
    if opt.get("extra") == "duplicate":
        faces = np.concatenate([faces, faces[:120]]).astype(np.int32)
    if opt.get("near") == "vertex":        # one front vertex of sample 0 lies just in front of the plane in both of its views
        pc = [(verts[0].astype(np.float64) - T[v, :3, 3]) @ T[v, :3, :3].astype(np.float64) for v in range(BN)]
        order = np.argsort(pc[0][:, 2])
        near = float(np.float32(0.5 * (max(p[order[0], 2] for p in pc) + min(p[order[1:], 2].min() for p in pc))))
        assert all(p[order[0], 2] < near < p[order[1:], 2].min() for p in pc)
    bg = rng.randint(0, 256, size=(BN, H, W, 3)).astype(np.uint8)
    return dict(views=views, H=H, W=W, K=K, T=T, verts=verts, faces=faces, near=near, bg=bg)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per view: the five stability samples of the restatement and eps_pos."""
    s = scene(name)
    lights, albedo = pk.render.default_lights(), np.float32(pk.render.DEFAULT_ALBEDO)
    out, v = [], 0
    for b, n in enumerate(s["views"]):
        for _ in range(n):
            uvz, col = ref_vertices(s["verts"][b], s["faces"], s["K"][v], s["T"][v], lights, albedo)
            samples = ref_raster(uvz, col, s["faces"], s["H"], s["W"], s["near"], STABILITY_OFFSETS)
            Ti = np.linalg.inv(s["T"][v].astype(np.float64))
            m = (np.abs(s["verts"][b].astype(np.float64)) @ np.abs(Ti[:3, :3]).T + np.abs(Ti[:3, 3])).max()
            front = uvz[:, 2] >= s["near"]
            c = np.array([s["K"][v][0, 2], s["K"][v][1, 2]], np.float64)
            foc = float(s["K"][v][0, 0])
            du = (foc / uvz[front, 2] * (1 + np.abs(uvz[front, :2] - c).max(1) / foc) * 6 * EPS * m
                  + 4 * EPS * (np.abs(uvz[front, :2] - c).max(1) + np.abs(c).max())).max()
            tri = uvz[s["faces"]][front[s["faces"]].all(1)][:, :, :2]
            diam = max(np.abs(tri - tri[:, [1, 2, 0]]).max(), 1.0)
            out.append(dict(samples=samples, eps_pos=du + 8 * EPS * diam))
            v += 1
    return out


def depth_bar(r):
    """The per-pixel depth bar of the module docstring, from the restatement alone: |grad z'| is the steepest of the faces that win
    at the pixel's four offset samples -- the offsets point into all four quadrants, so a neighbour that the kernel may prefer within
    eps_pos << 0.01 px of an edge is among them."""
    hit, z, _, _, grad = r["samples"][0]
    other = np.max([g for _, _, _, _, g in r["samples"][1:]], axis=0)
    return 16 * EPS * np.where(hit, z, 0.0) + r["eps_pos"] * (grad + other)


def _dev(a, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


@functools.lru_cache(maxsize=None)
def rendered(name):
    s = scene(name)
    r = pk.MeshRenderer(s["faces"], DEV)
    r.near_z = s["near"]
    rgb, depth, fid = r.render(_dev(s["verts"]), _dev(s["K"]), _dev(s["T"]), s["views"], background=_dev(s["bg"]), return_depth=True,
                               return_face_id=True)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), depth.cpu().numpy(), fid.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_render_matches_the_fp64_restatement(name):
    s, ref = scene(name), reference(name)
    rgb, depth, fid = rendered(name)
    assert rgb.shape == (sum(s["views"]), s["H"], s["W"], 3) and rgb.dtype == np.uint8
    covered = unstable = 0
    worst = dict(depth_over_bar=0.0, depth=0.0, colour=0)
    for v, r in enumerate(ref):
        hit, z, f, col, grad = r["samples"][0]
        ghit = fid[v] >= 0
        zg = np.where(ghit, depth[v], 0.0).astype(np.float64)
        bar = depth_bar(r)
        stable = ref_stable(r["samples"], bar)
        covered += int(hit.sum())
        unstable += int((hit & ~stable).sum())
        assert np.array_equal(ghit, np.isfinite(depth[v]))
        assert np.array_equal(ghit[stable], hit[stable]), f"view {v}: hit / miss differs on {int((ghit != hit)[stable].sum())} stable pixels"
        both = stable & hit
        err = np.abs(zg - np.where(hit, z, 0.0))[both]
        if err.size:
            k = np.argmax(err / bar[both])
            worst["depth_over_bar"] = max(worst["depth_over_bar"], float((err / bar[both])[k]))
            worst["depth"] = max(worst["depth"], float(err.max()))
        want = np.minimum((col * 255.0).astype(np.int64), 255)
        dc = np.abs(rgb[v].astype(np.int64) - want).max(-1)
        worst["colour"] = max(worst["colour"], int(dc[both].max()) if both.any() else 0)
        # with a background, every pixel that nothing covers is the background, bit for bit
        assert np.array_equal(rgb[v][~ghit], s["bg"][v][~ghit])
    share = unstable / max(covered, 1)
    print(f"render[{name}]: covered {covered} px, unstable {unstable} ({100 * share:.3f} %), worst depth error {worst['depth']:.3e} m = "
          f"{worst['depth_over_bar']:.3f} of its bar, worst colour step {worst['colour']}")
    assert covered > 0 and share <= 0.01, (covered, unstable)
    assert worst["depth_over_bar"] <= 1.0, worst
    assert worst["colour"] <= 1, worst
    opt = CASES[name][3]
    if opt.get("extra") == "duplicate":
        assert fid.max() < len(s["faces"]) - 120                           # the copies have the higher indices: never reported
    if opt.get("extra") == "zero_area":
        assert (fid != len(s["faces"]) - 1).all()
    if opt.get("soup"):
        assert (fid == 299).all()                                          # the nearest face is the last one, past the list's 256


def test_a_vertex_behind_near_takes_its_faces_and_nothing_else():
    s = scene("behind_near")
    rgb, depth, fid = rendered("behind_near")
    r = pk.MeshRenderer(s["faces"], DEV)
    rgb0, depth0, fid0 = (t.cpu().numpy() for t in r.render(_dev(s["verts"]), _dev(s["K"]), _dev(s["T"]), s["views"], background=_dev(s["bg"]),
                                                            return_depth=True, return_face_id=True))
    pc = (s["verts"][0].astype(np.float64) - s["T"][0, :3, 3]) @ s["T"][0, :3, :3].astype(np.float64)
    gone = np.nonzero((s["faces"] == np.argmin(pc[:, 2])).any(1))[0]
    assert len(gone) in (5, 6) and np.isin(fid0, gone).any() and not np.isin(fid, gone).any()
    keep = ~np.isin(fid0, gone)
    assert np.array_equal(fid[keep], fid0[keep]) and np.array_equal(depth[keep], depth0[keep]) and np.array_equal(rgb[keep], rgb0[keep])


def test_two_meshes_in_one_call_equal_two_calls_and_runs_repeat():
    s = scene("50x70_ragged")
    r = pk.MeshRenderer(s["faces"], DEV)
    va = _dev(s["verts"])
    vb = _dev(s["verts"][::-1] + np.float32([0.01, -0.005, 0.02]))
    args = (_dev(s["K"]), _dev(s["T"]), s["views"])
    kw = dict(background=_dev(s["bg"]), return_depth=True, return_face_id=True)
    both = r.render(torch.stack([va, vb]), *args, **kw)
    again = r.render(torch.stack([va, vb]), *args, **kw)
    one = [r.render(x, *args, **kw) for x in (va, vb)]
    for k in range(3):
        assert both[k].shape[0] == 2 and torch.equal(both[k], again[k])
        assert torch.equal(both[k][0], one[0][k]) and torch.equal(both[k][1], one[1][k])
    assert torch.equal(both[0][0], _dev(rendered("50x70_ragged")[0]))
    assert not torch.equal(both[0][0], both[0][1])
    white = r.render(va, *args, image_size=(s["H"], s["W"]), return_face_id=True)
    assert (white[0][white[1] < 0] == 255).all()


def _abi_render(r, s, verts, rgb, depth, fid, ws, ws_bytes):
    """poem_render_mesh through the C ABI with raw pointers; verts (M,B,V,3) on the device.  Returns the code."""
    K, T = _dev(s["K"]), _dev(s["T"])
    offs = _dev(np.concatenate([[0], np.cumsum(s["views"])]).astype(np.int32))
    vf_off, vf_ids = r.csr(verts.shape[2])
    rc = hip.lib().poem_render_mesh(verts.data_ptr(), r.faces.data_ptr(), vf_off.data_ptr(), vf_ids.data_ptr(), K.data_ptr(), T.data_ptr(),
                                    offs.data_ptr(), None, r.lights.data_ptr(), 3, r.albedo.data_ptr(), 0.01, rgb, depth, fid,
                                    verts.shape[0], len(s["views"]), verts.shape[2], len(s["faces"]), s["H"], s["W"], ws, ws_bytes, hip.stream())
    torch.cuda.synchronize()
    return rc


def _poison(nbytes):
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("name", ["50x70_ragged", "64_occluded"])           # byte stores (W % 4 != 0) and packed dword stores
def test_guard_bytes_around_the_outputs_stay(name):
    s = scene(name)
    r = pk.MeshRenderer(s["faces"], DEV)
    BN, H, W, G = sum(s["views"]), s["H"], s["W"], 256
    n = BN * H * W
    bufs = [_poison(G + n * 3 + G), _poison(G + n * 4 + G), _poison(G + n * 4 + G)]
    verts = _dev(s["verts"])[None].contiguous()
    need = hip.lib().poem_render_workspace_bytes(BN, verts.shape[2], 1)
    ws = _poison(need + 2 * G)
    assert _abi_render(r, s, verts, bufs[0].data_ptr() + G, bufs[1].data_ptr() + G, bufs[2].data_ptr() + G, ws.data_ptr() + G, need) == 0
    for b in bufs + [ws]:
        assert (b[:G] == 0xA5).all() and (b[-G:] == 0xA5).all()
    fid = bufs[2][G:-G].view(torch.int32).view(BN, H, W).cpu().numpy()
    assert np.array_equal(fid, rendered(name)[2])
    # an rgb that is not 4-byte aligned takes the byte stores whatever the width: same pixels, same guards
    odd = _poison(G + n * 3 + G)
    assert _abi_render(r, s, verts, odd.data_ptr() + G + 1, None, None, ws.data_ptr() + G, need) == 0
    assert (odd[:G + 1] == 0xA5).all() and (odd[G + 1 + n * 3:] == 0xA5).all()
    assert torch.equal(odd[G + 1:G + 1 + n * 3], bufs[0][G:-G])
    # a workspace that holds no view is refused
    assert _abi_render(r, s, verts, bufs[0].data_ptr() + G, None, None, ws.data_ptr() + G, 8) == -2


def test_a_workspace_for_fewer_views_draws_those_views_and_stays_inside_it():
    """Two meshes, six views, a workspace for three: mesh 1's vertices must land inside the three-view workspace (not at the stride
    of the batch's six), views 0..2 of both meshes are drawn, the planes of views 3..5 are not touched."""
    s = scene("50x70_ragged")
    r = pk.MeshRenderer(s["faces"], DEV)
    BN, H, W, G = sum(s["views"]), s["H"], s["W"], 4096
    verts = torch.stack([_dev(s["verts"]), _dev(s["verts"] + np.float32([0.004, 0.002, 0.01]))]).contiguous()
    full = r.render(verts, _dev(s["K"]), _dev(s["T"]), s["views"], image_size=(H, W), return_depth=True, return_face_id=True)
    L = hip.lib()
    V = verts.shape[2]
    cap = 3
    need = L.poem_render_workspace_bytes(cap, V, 2)
    assert need == cap * 2 * V * 24 and need < L.poem_render_workspace_bytes(BN, V, 2)
    n = 2 * BN * H * W
    ws, rgb, depth, fid = _poison(G + need + G), _poison(n * 3), _poison(n * 4), _poison(n * 4)
    assert _abi_render(r, s, verts, rgb.data_ptr(), depth.data_ptr(), fid.data_ptr(), ws.data_ptr() + G, need) == 0
    assert (ws[:G] == 0xA5).all() and (ws[-G:] == 0xA5).all()
    assert not (ws[G:-G].view(2 * cap * V, 24) == 0xA5).all(1).any()          # every slot of the smaller workspace was written
    for got, want, width in ((rgb, full[0], 3), (depth, full[1].view(torch.uint8), 4), (fid, full[2].view(torch.uint8), 4)):
        got, want = got.view(2, BN, H * W * width), want.reshape(2, BN, H * W * width)
        assert torch.equal(got[:, :cap], want[:, :cap])
        assert (got[:, cap:] == 0xA5).all()


def test_csr_table_is_built_for_the_vertex_count_rendered():
    """Faces that name only the first vertices of a longer vertex array: the kernel reads an offset pair for every vertex it is
    given, so the table must have V + 1 entries for that V (the tail = empty lists).  A read past a shorter table cannot be seen from
    the device's results (the kernel clamps what it reads), so the table's length is what is asserted, next to the result."""
    s = scene("F256")
    V, used = s["verts"].shape[1], int(s["faces"].max()) + 1
    assert used < V
    r = pk.MeshRenderer(s["faces"], DEV)
    off, ids = r.csr(V)
    assert off.numel() == V + 1 and ids.numel() == 3 * len(s["faces"]) and (off[used:] == ids.numel()).all()
    assert r.csr(used)[0].numel() == used + 1 and torch.equal(r.csr(used)[0], off[:used + 1])
    args = (_dev(s["K"]), _dev(s["T"]), s["views"])
    kw = dict(image_size=(s["H"], s["W"]), return_depth=True, return_face_id=True)
    long, short = r.render(_dev(s["verts"]), *args, **kw), r.render(_dev(s["verts"][:, :used]), *args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(long, short))


def test_top_left_fill_rule_on_pixel_centres():
    """A square [8, 24]^2 of two triangles whose edges run through pixel centres: left and top edge are in, right and bottom edge out,
    and the diagonal's pixels are drawn once (by either face)."""
    verts = np.float32([[[8, 8, 1], [24, 8, 1], [24, 24, 1], [8, 24, 1]]])
    K, T = np.float32([[[1, 0, 0], [0, 1, 0], [0, 0, 1]]]), np.eye(4, dtype=np.float32)[None]
    for faces in ([[0, 1, 2], [0, 2, 3]], [[2, 1, 0], [3, 0, 2]], [[1, 2, 0], [2, 3, 0]]):
        r = pk.MeshRenderer(np.int32(faces), DEV)
        rgb, fid = r.render(_dev(verts), _dev(K), _dev(T), [1], image_size=(32, 32), return_face_id=True)
        want = np.zeros((32, 32), bool)
        want[8:24, 8:24] = True
        assert np.array_equal(fid[0].cpu().numpy() >= 0, want), faces


def test_skeleton_matches_the_disc_and_capsule_rule():
    rng = np.random.RandomState(11)
    H, W, n = 50, 70, 3
    img = rng.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
    joints = rng.uniform([5, 5], [W - 5, H - 5], size=(n, 21, 2))
    joints[1, :6] += [[-40.0, 20.0]]                       # joints outside the image
    joints[2, :4] = np.round(joints[2, :4])                 # integer positions: boundaries that run through pixel centres
    joints[2, 5] = [300.0, -200.0]                          # a capsule that enters from far outside
    joints = joints.astype(np.float32)
    out = pk.draw_skeleton(_dev(img), _dev(joints)).cpu().numpy()
    painted = near = 0
    for v in range(n):
        want, dist = ref_skeleton(img[v], joints[v].astype(np.float64), pk.render.skeleton_colours())
        clear = dist > 1e-3
        assert np.array_equal(out[v][clear], want[clear]), v
        painted += int((want != img[v]).any(-1).sum())
        near += int((~clear).sum())
    print(f"skeleton: painted {painted} px, within 1e-3 px of a boundary {near}")
    assert painted > 500 and near <= 0.01 * painted


def test_project_to_views_is_the_vertex_stage():
    s = scene("50x70_ragged")
    uv = pk.project_to_views(_dev(s["verts"]), _dev(s["K"]), _dev(s["T"]), s["views"]).cpu().numpy()
    v = 0
    for b, n in enumerate(s["views"]):
        for _ in range(n):
            want = ref_vertices(s["verts"][b], s["faces"], s["K"][v], s["T"][v], pk.render.default_lights(), pk.render.DEFAULT_ALBEDO)[0]
            assert np.abs(uv[v] - want[:, :2]).max() <= reference("50x70_ragged")[v]["eps_pos"]
            v += 1


def test_drawing_callback_writes_every_view(tmp_path):
    from test_render_host import _decode_png
    rng = np.random.RandomState(5)
    views, H, W = [2, 3], 64, 64
    K, T = _cameras(5, H, W, rng)
    verts, faces = _ellipsoids(2, rng, False)
    image = torch.tensor(rng.randint(0, 256, size=(5, 3, H, W)).astype(np.float32) / 255.0 - 0.5, device=DEV)
    joints = torch.tensor(verts[:, :21].copy(), device=DEV)
    cb = pk.DrawingHandCallback(str(tmp_path / "draw"), faces)
    cb({"pred_verts_3d": _dev(verts), "pred_joints_3d": joints},
       {"image": image, "cam_view_num": views, "target_cam_intr": torch.tensor(K), "target_cam_extr": torch.tensor(T),
        "master_verts_3d": torch.tensor(verts + np.float32(0.003)), "master_joints_3d": joints.cpu() + 0.003}, 7)
    files = sorted(os.listdir(tmp_path / "draw"))
    assert files == sorted(f"step7_frame{i}_view{j}{g}.png" for i, n in enumerate(views) for j in range(n) for g in ("", "_GT"))
    v = 0
    for i, n in enumerate(views):
        for j in range(n):
            a = _decode_png(str(tmp_path / "draw" / f"step7_frame{i}_view{j}.png"))
            g = _decode_png(str(tmp_path / "draw" / f"step7_frame{i}_view{j}_GT.png"))
            assert a.shape == g.shape == (H, 3 * W, 3)
            want = ((image[v].cpu().numpy().astype(np.float32) + np.float32(0.5)) * np.float32(255.0)).transpose(1, 2, 0).astype(np.uint8)
            assert np.array_equal(a[:, :W], want) and np.array_equal(g[:, :W], want)
            assert (a[:, W:2 * W] != want).any() and (a[:, 2 * W:] != want).any() and (a[:, 2 * W:] != g[:, 2 * W:]).any()
            v += 1
