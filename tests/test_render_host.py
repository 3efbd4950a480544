"""Host side of the renderer (poem_v2_amd/render.py, csrc/render.hip): CSR adjacency, PNG writer, ctypes table, command line -- and the
fp64 restatement that tests/test_render.py holds the kernels against.

The restatement is brute force: every pixel's edge functions against every face (dense, fp64; chunked for memory only -- no tile, bin
or bounding box skips a pair), then the nearest inside face per pixel by a sort.  It shares no structure with the kernel.  Upstream
renders through opendr / OpenGL, which is absent here: no pixel of the reference can be produced, so pixel-centre convention (integer
coordinates are centres), top-left fill rule, light model and hard edges are this project's own and are restated here."""
import importlib.util
import os
import re
import struct
import zlib

import numpy as np
import pytest

import poem_v2_amd as pk
from poem_v2_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 0.01                                                   # px: offset of the four stability samples


# ---- generated meshes ------------------------------------------------------------------------------------------------------------
def geodesic_sphere(n=6):
    """Frequency-n subdivision of the icosahedron pushed onto the unit sphere: V = 10 n^2 + 2, F = 20 n^2 (n = 6: 362, 720),
    outward-wound."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    iv = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
                   [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    ifc = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
           (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    index, verts, faces = {}, [], []

    def vid(p):
        key = tuple(np.round(p / np.linalg.norm(p), 9))
        if key not in index:
            index[key] = len(verts)
            verts.append(p / np.linalg.norm(p))
        return index[key]

    for a, b, c in ifc:
        A, B, C = iv[a], iv[b], iv[c]
        g = [[vid((A * (n - i - j) + B * i + C * j) / n) for j in range(n - i + 1)] for i in range(n + 1)]
        for i in range(n):
            for j in range(n - i):
                faces.append((g[i][j], g[i + 1][j], g[i][j + 1]))
                if j < n - i - 1:
                    faces.append((g[i + 1][j], g[i + 1][j + 1], g[i][j + 1]))
    return np.array(verts), np.array(faces, dtype=np.int32)


# ---- fp64 restatement ---------------------------------------------------------------------------------------------------------------
def ref_vertices(verts, faces, K, T_c2m, lights, albedo):
    """fp64: (V,3) master-frame vertices -> (u, v, z) and Lambert colours in the camera frame (normals by scatter-add over corners)."""
    verts, K, lights = np.asarray(verts, np.float64), np.asarray(K, np.float64), np.asarray(lights, np.float64).reshape(-1, 6)
    Ti = np.linalg.inv(np.asarray(T_c2m, np.float64))
    pc = verts @ Ti[:3, :3].T + Ti[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        uvz = np.stack([K[0, 0] * pc[:, 0] / pc[:, 2] + K[0, 2], K[1, 1] * pc[:, 1] / pc[:, 2] + K[1, 2], pc[:, 2]], axis=1)
    fn = np.cross(pc[faces[:, 1]] - pc[faces[:, 0]], pc[faces[:, 2]] - pc[faces[:, 0]])
    nrm = np.zeros_like(pc)
    for k in range(3):
        np.add.at(nrm, faces[:, k], fn)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.divide(nrm, ln, out=np.zeros_like(nrm), where=ln > 0)
    shade = np.zeros_like(pc)
    for L in lights:
        d = L[:3] - pc
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        shade += L[3:] * np.maximum(0.0, (nrm * d).sum(1))[:, None]
    return uvz, np.clip(np.asarray(albedo, np.float64) * shade, 0.0, 1.0)


def ref_raster(uvz, col, faces, H, W, near, offsets=((0.0, 0.0),)):
    """fp64 brute force.  For every sample offset: (hit (H,W) bool, depth (inf = miss), face id (-1 = miss), colour (H,W,3) in [0,1],
    |grad z| of the winning face in m / px).  Nearest depth wins, the lower face index at equal depth; top-left fill rule; faces with
    a vertex nearer than `near` or without area are dropped; no back-face culling."""
    faces = np.asarray(faces)
    P = H * W
    tri = uvz[faces]                                                         # (F,3,3)
    with np.errstate(invalid="ignore"):
        area2 = ((tri[:, 1, 0] - tri[:, 0, 0]) * (tri[:, 2, 1] - tri[:, 0, 1]) - (tri[:, 1, 1] - tri[:, 0, 1]) * (tri[:, 2, 0] - tri[:, 0, 0]))
        ok = (tri[:, :, 2] >= near).all(1) & (area2 != 0) & np.isfinite(tri).all((1, 2))
    fidx = np.nonzero(ok)[0]
    tri, sgn = tri[fidx], np.sign(area2[fidx])
    # edge i lies opposite vertex i: E_i(p) = A_i x + B_i y + C_i, positive inside
    j, k = [1, 2, 0], [2, 0, 1]
    A = sgn[:, None] * -(tri[:, k, 1] - tri[:, j, 1])
    B = sgn[:, None] * (tri[:, k, 0] - tri[:, j, 0])
    C = -(A * tri[:, j, 0] + B * tri[:, j, 1])
    topleft = (A > 0) | ((A == 0) & (B > 0))
    iz = 1.0 / tri[:, :, 2]
    margin = 2.0 * max(abs(o) for off in offsets for o in off) * (np.abs(A) + np.abs(B)) + 1e-300
    ys, xs = np.divmod(np.arange(P), W)
    cf, cp = [], []
    for p0 in range(0, P, 8192):                                             # dense pass: every face against every pixel
        xy1 = np.stack([xs[p0:p0 + 8192], ys[p0:p0 + 8192], np.ones(len(xs[p0:p0 + 8192]))]).astype(np.float64)
        for f0 in range(0, len(fidx), 128):
            sl = slice(f0, f0 + 128)
            E = np.stack([A[sl], B[sl], C[sl]], axis=2).reshape(-1, 3) @ xy1       # (Fc*3, Pc)
            cand = (E >= -margin[sl].reshape(-1, 1)).reshape(-1, 3, E.shape[1]).all(1)
            f, p = np.nonzero(cand)                                           # a pair outside `margin` is outside at every sample
            cf.append(f + f0)
            cp.append(p + p0)
    cf, cp = np.concatenate(cf), np.concatenate(cp)
    out = []
    for ox, oy in offsets:
        x, y = xs[cp] + ox, ys[cp] + oy
        E = A[cf] * x[:, None] + B[cf] * y[:, None] + C[cf]
        inside = ((E > 0) | ((E == 0) & topleft[cf])).all(1)
        f, p, E = cf[inside], cp[inside], E[inside]
        q = E * iz[f]
        z = E.sum(1) / q.sum(1)
        order = np.lexsort((fidx[f], z, p))
        first = order[np.r_[True, p[order][1:] != p[order][:-1]]] if len(order) else order
        hit, depth, fid = np.zeros(P, bool), np.full(P, np.inf), np.full(P, -1, np.int64)
        rgb, grad = np.ones((P, 3)), np.zeros(P)
        w = q[first] / q[first].sum(1, keepdims=True)
        hit[p[first]], depth[p[first]], fid[p[first]] = True, z[first], fidx[f[first]]
        rgb[p[first]] = np.clip((w[:, :, None] * col[faces[fidx[f[first]]]]).sum(1), 0.0, 1.0)
        # 1/z = (sum_i E_i / z_i) / |area2| is linear in the pixel: grad z = -z^2 grad(1/z)
        ga = (A[f[first]] * iz[f[first]]).sum(1) / np.abs(area2[fidx[f[first]]])
        gb = (B[f[first]] * iz[f[first]]).sum(1) / np.abs(area2[fidx[f[first]]])
        grad[p[first]] = z[first] ** 2 * np.hypot(ga, gb)
        out.append((hit.reshape(H, W), depth.reshape(H, W), fid.reshape(H, W), rgb.reshape(H, W, 3), grad.reshape(H, W)))
    return out


STABILITY_OFFSETS = ((0.0, 0.0), (DELTA, DELTA), (DELTA, -DELTA), (-DELTA, DELTA), (-DELTA, -DELTA))


def ref_stable(samples, bar):
    """Stable pixels: the four samples at (+-DELTA, +-DELTA) give the pixel's hit or miss, and its depth to within the depth bar once
    the slope of the pixel's own face over the offset (|grad z| * sqrt(2) * DELTA) is allowed for -- a neighbour across an interior
    edge passes (the surface is continuous there), a silhouette or an occlusion boundary does not."""
    hit, depth, _, _, grad = samples[0]
    stable = np.ones_like(hit)
    allow = bar + grad * (2.0 ** 0.5) * DELTA * 1.05
    for h, d, _, _, _ in samples[1:]:
        stable &= h == hit
        with np.errstate(invalid="ignore"):
            stable &= ~hit | ~h | (np.abs(np.where(h & hit, d - depth, 0.0)) <= allow)
    return stable


def ref_skeleton(image, joints, colours):
    """fp64 disc / capsule rule -> (painted image, distance of every pixel to the nearest shape boundary in px)."""
    H, W = image.shape[:2]
    out = image.copy()
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    near = np.full((H, W), np.inf)
    col8 = np.minimum((np.clip(np.asarray(colours, np.float32), 0, 1) * np.float32(255.0)).astype(np.int64), 255).astype(np.uint8)
    for j in range(21):
        d = np.hypot(xs - joints[j, 0], ys - joints[j, 1]) - 6.0
        if j > 0:
            a = joints[0] if j % 4 == 1 else joints[j - 1]
            s = joints[j] - a
            t = np.clip(((xs - a[0]) * s[0] + (ys - a[1]) * s[1]) / max(s @ s, 1e-300), 0.0, 1.0)
            d = np.minimum(d, np.hypot(xs - a[0] - t * s[0], ys - a[1] - t * s[1]) - 1.5)
        out[d <= 0] = col8[j]
        near = np.minimum(near, np.abs(d))
    return out, near


# ---- CPU tests --------------------------------------------------------------------------------------------------------------------------
def test_geodesic_mesh_is_the_issue_s_size_and_closed():
    v, f = geodesic_sphere(6)
    assert v.shape == (362, 3) and f.shape == (720, 3)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert ((n * v[f].mean(1)).sum(1) > 0).all()                              # outward winding
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    assert (np.unique(e, axis=0, return_counts=True)[1] == 2).all()           # every edge has two faces


def test_csr_adjacency_equals_dict_of_lists():
    rng = np.random.RandomState(3)
    V, F = 57, 200
    faces = rng.randint(0, V - 3, size=(F, 3))                                # (the last vertices touch no face)
    faces[7] = (5, 5, 9)                                                      # a face that names a vertex twice
    off, ids = pk.render.vertex_face_csr(faces, V)
    around = {i: [] for i in range(V)}
    for f, tri in enumerate(faces):
        for i in tri:
            around[int(i)].append(f)
    assert off.dtype == np.int32 and ids.dtype == np.int32 and off.shape == (V + 1,) and ids.shape == (3 * F,)
    for i in range(V):
        assert ids[off[i]:off[i + 1]].tolist() == around[i], i
    with pytest.raises(ValueError):
        pk.render.vertex_face_csr(np.array([[0, 1, V]]), V)


def _decode_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks.append((tag, data))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, bits, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (bits, comp, filt, lace) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 3 if ctype == 2 else 1
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * ch)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape((h, w, 3) if ch == 3 else (h, w))


def test_save_png_round_trips(tmp_path):
    rng = np.random.RandomState(0)
    for shape in ((5, 7, 3), (1, 1, 3), (9, 4)):
        a = rng.randint(0, 256, size=shape).astype(np.uint8)
        pk.save_png(str(tmp_path / "a.png"), a)
        assert np.array_equal(_decode_png(str(tmp_path / "a.png")), a)
    with pytest.raises(ValueError):
        pk.save_png(str(tmp_path / "b.png"), np.zeros((4, 4, 3), np.float32))


def test_render_ctypes_signatures_match_the_header():
    """Argument by argument: a drifted ctypes table would pass a pointer where the library reads an int."""
    import ctypes
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "poem_hip.h")).read(), flags=re.S)
    L = hip.lib()
    for name in ("poem_render_workspace_bytes", "poem_render_mesh", "poem_project_points", "poem_draw_skeleton"):
        m = re.search(r"\b(size_t|int)\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, re.S)
        assert m, name
        want = []
        for arg in m.group(2).split(","):
            arg = arg.strip()
            want.append(ctypes.c_void_p if "*" in arg else {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}[
                re.sub(r"\s*\w+$", "", arg)])
        res, args = hip.SIGNATURES[name]
        assert res == {"size_t": ctypes.c_size_t, "int": ctypes.c_int}[m.group(1)] and args == want, name
        assert hasattr(L, name)
    assert L.poem_render_workspace_bytes(6, 362, 2) == 6 * 362 * 2 * 24 and L.poem_render_workspace_bytes(0, 362, 1) == 0
    # argument checks run on the host before any launch
    assert L.poem_render_mesh(*([None] * 9), 3, None, 0.01, *([None] * 3), 1, 1, 4, 2, 8, 8, None, 0, None) == -1
    assert L.poem_draw_skeleton(None, None, None, None, 1, 8, 8, None) == -1
    assert L.poem_project_points(None, None, None, None, None, 1, 1, 1, None) == -1


def test_restatement_depth_on_a_sphere_is_the_ray_sphere_depth():
    """The fp64 yardstick against closed form: a unit-sphere mesh of radius r at (0, 0, z0); away from the silhouette the depth along
    the pixel's ray differs from the analytic sphere's by the chord sag of the faceting only."""
    v, f = geodesic_sphere(6)
    r, z0, foc, H, W = 0.05, 0.6, 300.0, 64, 64
    K = np.array([[foc, 0, 32.0], [0, foc, 32.0], [0, 0, 1]])
    uvz, col = ref_vertices(v * r + [0, 0, z0], f, K, np.eye(4), pk.render.default_lights(), pk.render.DEFAULT_ALBEDO)
    hit, depth, fid, rgb, grad = ref_raster(uvz, col, f, H, W, 0.01)[0]
    ys, xs = np.mgrid[0:H, 0:W]
    d = np.stack([(xs - 32.0) / foc, (ys - 32.0) / foc, np.ones((H, W))], axis=-1)
    dd, dc = (d * d).sum(-1), d[..., 2] * z0
    disc = dc * dc - dd * (z0 * z0 - r * r)
    rad = np.hypot(xs - 32.0, ys - 32.0)
    inner = rad < 0.8 * r * foc / z0                                           # 20 of the 25 px
    assert hit[inner].all() and not hit[rad > 1.05 * r * foc / z0].any()
    za = (dc - np.sqrt(np.maximum(disc, 0))) / dd                              # nearest intersection's z (d_z = 1)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    sag = r * (1 - ((fn / np.linalg.norm(fn, axis=1, keepdims=True)) * v[f[:, 0]]).sum(1).min())     # deepest face plane below the sphere
    err = (depth - za)[inner]
    # the mesh lies inside the sphere: depth >= analytic; the radial sag is stretched along the ray by 1 / cos(incidence), at most
    # 1 / 0.6 at 0.8 r (5 % for the ray's own tilt against the radius)
    assert err.min() > -1e-12 and err.max() < 1.05 * sag / 0.6, (err.min(), err.max(), sag)
    assert (fid[inner] >= 0).all() and (rgb[inner] <= 1).all() and (grad[inner] < 0.01).all()


def test_eval_single_parses_faces_and_draw_dir():
    spec = importlib.util.spec_from_file_location("eval_single_cli", os.path.join(ROOT, "scripts", "eval_single.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    base = "--cfg c.yaml --dataset HO3D --view_min 2 --view_max 4 --model small -g 0".split()
    a = m.build_parser().parse_args(base)
    assert a.faces is None and a.draw_dir == "./draw" and not a.draw
    a = m.build_parser().parse_args(base + ["--draw", "--faces", "f.npy", "--draw-dir", "/tmp/x"])
    assert a.draw and a.faces == "f.npy" and a.draw_dir == "/tmp/x"


def test_renderer_refuses_cpu_tensors():
    import torch
    with pytest.raises(RuntimeError):
        pk.MeshRenderer(np.array([[0, 1, 2]]), "cpu")
    with pytest.raises(RuntimeError):
        pk.draw_skeleton(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 21, 2))
    with pytest.raises(RuntimeError):
        pk.project_to_views(torch.zeros(1, 4, 3), torch.zeros(1, 3, 3), torch.zeros(1, 4, 4), [1])
