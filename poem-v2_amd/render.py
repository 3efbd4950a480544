"""Device-side drawing of a result: the mesh rendered into every view, the 2-D skeleton, and the ``--draw`` callback of
``scripts/eval_single.py`` (upstream: ``DrawingHandCallback``, lib/utils/testing.py:101-192, on opendr / OpenGL / cv2 on the host).

Kernels: csrc/render.hip through ``poem_render_mesh`` / ``poem_project_points`` / ``poem_draw_skeleton`` (include/poem_hip.h).  Meshes,
cameras and images stay on the GPU; the callback copies the finished uint8 panels to the host once per step.  Pixel-centre
convention, fill rule, light model and the hard (not anti-aliased) edges are this project's own: DESIGN.md section 7, row R."""
import colorsys
import os
import struct
import zlib

import numpy as np
import torch

from . import hip

NEAR_Z = 0.01          # metres: faces with a vertex nearer than this (or behind the camera) are not drawn


def vertex_face_csr(faces, nverts):
    """(F,3) faces -> (offsets (V+1), face ids (3F)) int32: the faces around vertex i are ``ids[offsets[i]:offsets[i+1]]`` in
    ascending face order, one entry per corner (a face that names a vertex twice is listed twice and adds nothing to its normal)."""
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    if faces.size == 0 or faces.min() < 0 or faces.max() >= nverts:
        raise ValueError(f"faces must be a non-empty (F,3) array of vertex ids in [0, {nverts})")
    flat = faces.reshape(-1)
    order = np.argsort(flat, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=nverts))])
    return offsets.astype(np.int32), (order // 3).astype(np.int32)


def default_lights():
    """(3,6) position | colour of the three point lights of upstream's ``simple_renderer`` (lib/viztools/opendr_renderer.py:137-172):
    back, left and right light, each rotated by 120 degrees about Y, in the camera frame."""
    a = np.radians(120.0)
    ry = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    pos = np.array([[-200.0, -100.0, -100.0], [800.0, 10.0, 300.0], [-500.0, 500.0, 1000.0]]) @ ry
    col = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.7, 0.7, 0.7]])
    return np.concatenate([pos, col], axis=1).astype(np.float32)


DEFAULT_ALBEDO = (0.65, 0.74, 0.86)


def skeleton_colours():
    """(21,3) in [0,1]: grey wrist, one hue per finger (thumb red, index amber, middle green, ring blue, little violet), brighter
    towards the tip."""
    out = [(0.6, 0.6, 0.6)]
    for hue in (0.0, 0.11, 0.33, 0.6, 0.8):
        out += [colorsys.hsv_to_rgb(hue, 0.85, val) for val in (0.55, 0.7, 0.85, 1.0)]
    return np.asarray(out, dtype=np.float32)


_PALETTE = {}


def _offsets(cam_view_num, device):
    views = [int(v) for v in cam_view_num]
    return views, torch.tensor(np.concatenate([[0], np.cumsum(views)]).astype(np.int32), device=device)


def _check_cameras(cam_intr, cam_extr, BN):
    if tuple(cam_intr.shape) != (BN, 3, 3) or tuple(cam_extr.shape) != (BN, 4, 4):
        raise RuntimeError(f"cameras {tuple(cam_intr.shape)} / {tuple(cam_extr.shape)} do not match cam_view_num ({BN} views)")


class MeshRenderer:
    """Renders (B,V,3) or (M,B,V,3) master-frame meshes that share one face list into every view of a ragged batch."""

    def __init__(self, faces, device, lights=None, albedo=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("libpoem_hip operates on device tensors only (no CPU path)")
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[1] != 3 or not np.issubdtype(faces.dtype, np.integer) or faces.size == 0 or faces.min() < 0:
            raise ValueError(f"faces must be a non-empty (F,3) integer array, got {faces.dtype} {faces.shape}")
        self.nverts = int(faces.max()) + 1
        self._faces_host = faces.astype(np.int32)
        self.faces = torch.tensor(self._faces_host, device=self.device).contiguous()
        self._csr = {}
        self.csr(self.nverts)
        lights = default_lights() if lights is None else np.asarray(lights, dtype=np.float32).reshape(-1, 6)
        self.lights = torch.tensor(lights, device=self.device).contiguous()
        self.albedo = torch.tensor(np.asarray(DEFAULT_ALBEDO if albedo is None else albedo, dtype=np.float32).reshape(3), device=self.device)
        self.near_z = NEAR_Z
        self.workspace = None

    def csr(self, nverts):
        """(vf_offsets (nverts+1), vf_faces (3F)) on the device for meshes of `nverts` >= faces.max() + 1 vertices: the kernel reads
        an offset pair per vertex it renders, so the table is built for that count (vertices no face names get empty lists)."""
        if nverts not in self._csr:
            off, ids = vertex_face_csr(self._faces_host, nverts)
            self._csr[nverts] = (torch.tensor(off, device=self.device), torch.tensor(ids, device=self.device))
        return self._csr[nverts]

    def render(self, verts, cam_intr, cam_extr, cam_view_num, background=None, return_depth=False, return_face_id=False,
               image_size=None):
        """-> uint8 (BN,H,W,3), or (M,BN,H,W,3) for (M,B,V,3) input; with the flags a tuple (rgb, depth fp32, face id int32).
        ``background`` (BN,H,W,3) uint8 fixes the size; without one the image is white and ``image_size`` = (H, W) is needed."""
        if verts.dim() not in (3, 4) or verts.shape[-1] != 3:
            raise RuntimeError(f"verts {tuple(verts.shape)}: expected ([M,] B, V, 3)")
        stacked = verts.dim() == 4
        v4 = verts if stacked else verts[None]
        views, offs = _offsets(cam_view_num, self.device)
        M, B, V, BN = v4.shape[0], v4.shape[1], v4.shape[2], sum(views)
        if B != len(views) or V < self.nverts:
            raise RuntimeError(f"verts {tuple(verts.shape)}: expected ([M,] {len(views)}, V >= {self.nverts}, 3)")
        _check_cameras(cam_intr, cam_extr, BN)
        if background is not None:
            if background.dim() != 4 or background.shape[0] != BN or background.shape[3] != 3:
                raise RuntimeError(f"background {tuple(background.shape)}: expected ({BN}, H, W, 3)")
            H, W = int(background.shape[1]), int(background.shape[2])
        elif image_size is not None:
            H, W = int(image_size[0]), int(image_size[1])
        else:
            raise RuntimeError("render() needs a background or an image_size")
        L = hip.lib()
        vf_offsets, vf_faces = self.csr(V)
        need = L.poem_render_workspace_bytes(BN, V, M)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        rgb = torch.empty(M, BN, H, W, 3, dtype=torch.uint8, device=self.device)
        depth = torch.empty(M, BN, H, W, dtype=torch.float32, device=self.device) if return_depth else None
        fid = torch.empty(M, BN, H, W, dtype=torch.int32, device=self.device) if return_face_id else None
        with torch.cuda.device(self.device):
            # (exactly `need` bytes: the library reads the number of views it may draw from the workspace's size)
            hip.check(L.poem_render_mesh(hip.ptr(v4), self.faces.data_ptr(), vf_offsets.data_ptr(), vf_faces.data_ptr(),
                                         hip.ptr(cam_intr), hip.ptr(cam_extr), offs.data_ptr(), hip.ptr(background, torch.uint8),
                                         hip.ptr(self.lights), self.lights.shape[0], hip.ptr(self.albedo), float(self.near_z), rgb.data_ptr(),
                                         hip.ptr(depth), None if fid is None else fid.data_ptr(), M, B, V, self.faces.shape[0], H, W,
                                         self.workspace.data_ptr(), need, hip.stream()), "poem_render_mesh")
        out = [rgb, depth, fid]
        if not stacked:
            out = [None if t is None else t[0] for t in out]
        out = [t for t, want in zip(out, (True, return_depth, return_face_id)) if want]
        return out[0] if len(out) == 1 else tuple(out)


def project_to_views(points, cam_intr, cam_extr, cam_view_num):
    """points (B,P,3) master frame -> (BN,P,2) pixel coordinates in every view of each point's sample (the renderer's vertex stage)."""
    views, offs = _offsets(cam_view_num, hip_device(points))
    B, P, BN = points.shape[0], points.shape[1], sum(views)
    if points.dim() != 3 or points.shape[2] != 3 or B != len(views):
        raise RuntimeError(f"points {tuple(points.shape)}: expected ({len(views)}, P, 3)")
    _check_cameras(cam_intr, cam_extr, BN)
    uv = torch.empty(BN, P, 2, dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        hip.check(hip.lib().poem_project_points(hip.ptr(points), hip.ptr(cam_intr), hip.ptr(cam_extr), offs.data_ptr(), hip.ptr(uv), B, P,
                                                BN, hip.stream()), "poem_project_points")
    return uv


def draw_skeleton(image_u8, joints_uv, colours=None):
    """image_u8 (BN,H,W,3) uint8, joints_uv (BN,21,2) pixels -> a copy with the 2-D skeleton painted over it (hard edges)."""
    dev = hip_device(image_u8)
    if image_u8.dim() != 4 or image_u8.shape[3] != 3 or tuple(joints_uv.shape) != (image_u8.shape[0], 21, 2):
        raise RuntimeError(f"draw_skeleton: image {tuple(image_u8.shape)}, joints {tuple(joints_uv.shape)}")
    if colours is None:
        if dev not in _PALETTE:                              # the project's palette is uploaded once per device
            _PALETTE[dev] = torch.tensor(skeleton_colours(), device=dev)
        col = _PALETTE[dev]
    else:
        col = torch.tensor(np.asarray(colours, dtype=np.float32).reshape(21, 3), device=dev)
    out = torch.empty_like(image_u8)
    with torch.cuda.device(dev):
        hip.check(hip.lib().poem_draw_skeleton(hip.ptr(image_u8, torch.uint8), hip.ptr(joints_uv), hip.ptr(col),
                                               out.data_ptr(), image_u8.shape[0], image_u8.shape[1], image_u8.shape[2], hip.stream()),
                  "poem_draw_skeleton")
    return out


def hip_device(t):
    if not t.is_cuda:
        raise RuntimeError("libpoem_hip operates on device tensors only (no CPU path)")
    return t.device


def save_png(path, array):
    """(H,W,3) or (H,W) uint8 array -> 8-bit PNG, standard library only (zlib + struct)."""
    a = np.ascontiguousarray(np.asarray(array))
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError(f"save_png takes (H,W,3) or (H,W) uint8, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, -1)], axis=1).tobytes()      # filter type 0 in front of each row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


class DrawingHandCallback:
    """``__call__(preds, inputs, step_idx)`` writes ``step{S}_frame{i}_view{j}.png`` and ``..._GT.png`` under ``img_draw_dir``: a row
    [input | 2-D skeleton | mesh over the input] -- upstream's layout at ``with_mayavi_mesh=False, with_skeleton_3d=False``.
    preds: ``pred_verts_3d`` (B,V,3), ``pred_joints_3d`` (B,21,3); inputs: ``image`` (BN,3,H,W) normalised as the transform leaves it
    (p / 255 - 0.5), ``cam_view_num``, ``target_cam_intr``, ``target_cam_extr``, ``master_verts_3d``, ``master_joints_3d``.
    Any batch size (upstream's ``reshape(2, ...)`` ties it to two samples)."""

    def __init__(self, img_draw_dir, faces, lights=None, albedo=None):
        self.img_draw_dir = img_draw_dir
        os.makedirs(img_draw_dir, exist_ok=True)
        self.faces = np.asarray(faces)
        self.lights, self.albedo = lights, albedo
        self.renderer = None

    def panels(self, preds, inputs):
        """-> (2, BN, H, 3W, 3) uint8 on the device: prediction rows, then ground-truth rows."""
        verts = preds["pred_verts_3d"]
        dev = hip_device(verts)
        if self.renderer is None or self.renderer.device != dev:
            self.renderer = MeshRenderer(self.faces, dev, self.lights, self.albedo)
        views = [int(v) for v in inputs["cam_view_num"]]
        B, V = verts.shape[0], verts.shape[1]
        f32 = dict(device=dev, dtype=torch.float32)
        K = torch.as_tensor(inputs["target_cam_intr"]).reshape(-1, 3, 3).to(**f32).contiguous()
        T = torch.as_tensor(inputs["target_cam_extr"]).reshape(-1, 4, 4).to(**f32).contiguous()
        image = (inputs["image"].to(**f32) + 0.5).mul(255.0).clamp_(0.0, 255.0).permute(0, 2, 3, 1).to(torch.uint8).contiguous()
        gt_v = torch.as_tensor(inputs["master_verts_3d"]).to(**f32).reshape(B, V, 3)
        gt_j = torch.as_tensor(inputs["master_joints_3d"]).to(**f32).reshape(B, 21, 3)
        both_v = torch.stack([verts.to(**f32), gt_v]).contiguous()
        both_j = torch.cat([preds["pred_joints_3d"].to(**f32), gt_j], dim=1).contiguous()                  # (B,42,3): one projection
        mesh = self.renderer.render(both_v, K, T, views, background=image)                                 # (2,BN,H,W,3)
        uv = project_to_views(both_j, K, T, views)
        skel = torch.stack([draw_skeleton(image, uv[:, :21].contiguous()), draw_skeleton(image, uv[:, 21:].contiguous())])
        return torch.cat([image[None].expand(2, -1, -1, -1, -1), skel, mesh], dim=3)

    def __call__(self, preds, inputs, step_idx, **kwargs):
        host = self.panels(preds, inputs).cpu().numpy()                    # the one device -> host copy of the step
        v = 0
        for i, n in enumerate(int(c) for c in inputs["cam_view_num"]):
            for j in range(n):
                stem = os.path.join(self.img_draw_dir, f"step{step_idx}_frame{i}_view{j}")
                save_png(stem + ".png", host[0, v])
                save_png(stem + "_GT.png", host[1, v])
                v += 1

    def on_finished(self):
        pass
