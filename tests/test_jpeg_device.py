"""The device JPEG route on the GPU: ``poem_jpeg_reconstruct`` (csrc/jpeg.hip) through the C ABI, ``transform.warp_views`` on
``EncodedImage`` handles, the record reader with ``image_decode="device"`` and ``eval_single.py --image-decode device``.  The
yardstick is PIL on the same bytes (or the host route of the same pipeline) and every comparison is exact."""
import importlib.util
import io
import os
import random

import numpy as np
import pytest
import torch

import jpeg_util as ju
import poem_v2_amd as pk
from poem_v2_amd import hip, wds
from poem_v2_amd.transform import jpeg_counts, reset_jpeg_counts, warp_views

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5
OCCLUDED_HANDLES = 3             # of 6 views, the ones left without a patch by the draws of seed 3 (the rest are materialised)
VARIANTS = [dict(quality=30), dict(quality=100), dict(quality=90, optimize=True), dict(quality=95, restart_marker_blocks=1)]


def reconstruct_device(streams, shift=0, gap=5, coef_pad=0, out_pad=0):
    """One ``poem_jpeg_reconstruct`` call on `streams` -> (list of (H, W, 3) arrays or None, the whole output buffer, offsets,
    descs).  The output base is `shift` bytes off a 256-byte boundary, `gap` guard bytes sit between images; `coef_pad` / `out_pad`
    move every coefficient range / every image that many bytes up (to put them past 4 GiB)."""
    L = hip.lib()
    descs, coef, totals = ju.entropy_decode(streams)
    n = len(streams)
    offs, pos = [], out_pad
    for d in descs:
        offs.append(pos)
        pos += (d.height * d.width * 3 if d.status == 0 else 0) + gap
    cdev = torch.empty(coef_pad + coef.nbytes, dtype=torch.uint8, device=DEV)
    cdev[coef_pad:] = torch.from_numpy(coef.view(np.uint8)).to(DEV)
    for d in descs:
        d.coef_offset += coef_pad
    ddev = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    odev = torch.tensor(offs, dtype=torch.int64, device=DEV)
    buf = torch.empty(pos + shift + 256, dtype=torch.uint8, device=DEV)
    buf[max(out_pad - 64, 0):].fill_(GUARD)
    out = buf[shift:shift + pos]
    ws = torch.empty(max(L.poem_jpeg_workspace_bytes(totals[1]), 16), dtype=torch.uint8, device=DEV)
    rc = L.poem_jpeg_reconstruct(ddev.data_ptr(), cdev.data_ptr(), cdev.numel(), odev.data_ptr(), out.data_ptr(), out.numel(), n,
                                 totals[1], totals[2], ws.data_ptr(), ws.numel(), hip.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    tail = out[out_pad:].cpu().numpy()
    imgs = [tail[o - out_pad:o - out_pad + d.height * d.width * 3].reshape(d.height, d.width, 3) if d.status == 0 else None
            for o, d in zip(offs, descs)]
    return imgs, tail, [o - out_pad for o in offs], descs


def _streams(h, w, amp=25):
    rgb, grey = ju.make_image(h, w, amp), ju.make_image(h, w, amp, grey=True)
    out = []
    for kw in VARIANTS:
        out += [(f"{s}-{kw}", ju.encode(rgb, s, **kw)) for s in ju.SAMPLINGS] + [(f"grey-{kw}", ju.encode(grey, **kw))]
    return out


@pytest.mark.parametrize("h,w", ju.SIZES, ids=[f"{h}x{w}" for h, w in ju.SIZES])
def test_single_images_equal_pil(h, w):
    for amp in (25, 120):
        for name, data in _streams(h, w, amp):
            imgs, tail, offs, _ = reconstruct_device([data])
            assert imgs[0] is not None and np.array_equal(imgs[0], ju.pil_decode(data)), (name, amp)
            assert (tail[h * w * 3:] == GUARD).all(), name                  # nothing written behind the image


def test_narrow_images_equal_pil():
    """Width <= 4: chroma replicated, not interpolated (libjpeg's rule for a component at most 2 samples wide); 5 and 6: the first
    widths on the fancy path.  Solo calls and one ragged call."""
    cases = ju.narrow()
    refs = [ju.pil_decode(d) for _, d in cases]
    imgs = reconstruct_device([d for _, d in cases], shift=1)[0]
    bad = [n for (n, _), img, ref in zip(cases, imgs, refs) if img is None or not np.array_equal(img, ref)]
    assert not bad, bad
    for (n, d), ref in list(zip(cases, refs))[::9]:
        assert np.array_equal(reconstruct_device([d])[0][0], ref), n


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_ragged_batch_equals_solo_and_leaves_padding(shift):
    specs = [(33, 50, "420", 0), (8, 8, "444", 1), (17, 9, "422", 2), (29, 37, None, 3), (1, 1, "420", 0), (40, 24, "422", 1),
             (7, 70, "420", 2), (16, 16, None, 3), (40, 24, "444", 0)]
    streams = [ju.encode(ju.make_image(h, w, 120, seed=i, grey=s is None), **({} if s is None else {"sampling": s}), **VARIANTS[v])
               for i, (h, w, s, v) in enumerate(specs)]
    streams.insert(4, ju.encode(ju.make_image(16, 16, 25), "420", quality=75, progressive=True))      # a refused one in the middle
    imgs, tail, offs, descs = reconstruct_device(streams, shift=shift)
    written = np.zeros(tail.size, bool)
    for i, (data, img, o) in enumerate(zip(streams, imgs, offs)):
        if i == 4:
            assert img is None and descs[i].status == 1
            continue
        solo = reconstruct_device([data])[0][0]
        assert np.array_equal(img, solo) and np.array_equal(img, ju.pil_decode(data)), i
        written[o:o + img.size] = True
    assert (tail[~written] == GUARD).all()                                   # the bytes between and behind the images


def test_tile_coverage_at_camera_size():
    rng = np.random.default_rng(5)
    for (h, w, s) in [(480, 640, "420"), (478, 642, "422")]:
        y, x = np.mgrid[0:h, 0:w]
        img = np.clip(np.stack([x * 255 // (w - 1), y * 255 // (h - 1), (x + y) % 256], -1) + rng.integers(-40, 41, (h, w, 3)), 0,
                      255).astype(np.uint8)
        data = ju.encode(img, s, quality=90)
        out = reconstruct_device([data], shift=0 if s == "420" else 1)[0][0]
        assert np.array_equal(out, ju.pil_decode(data)), (h, w, s)


def test_offsets_past_4_gib():
    """Coefficients and pixels of a call may lie anywhere in buffers of any size: both are addressed with 64-bit byte offsets."""
    free, _ = torch.cuda.mem_get_info()
    assert free > 10 * 2 ** 30, "the MI355X has 288 GB; this test needs 9"
    data = [ju.encode(ju.make_image(33, 50, 120), "420", quality=90), ju.encode(ju.make_image(17, 9, 25), "422", quality=75)]
    imgs, tail, _, descs = reconstruct_device(data, shift=3, coef_pad=2 ** 32 + 4096, out_pad=2 ** 32 + 7)
    assert descs[0].coef_offset > 2 ** 32
    for d, img in zip(data, imgs):
        assert np.array_equal(img, ju.pil_decode(d))


def test_workspace_query_and_refusals_of_the_call():
    L = hip.lib()
    descs, coef, totals = ju.entropy_decode([ju.grid()[3][1]])
    d = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    c = torch.from_numpy(coef.view(np.uint8)).to(DEV)
    o = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.full((256,), GUARD, dtype=torch.uint8, device=DEV)
    need = L.poem_jpeg_workspace_bytes(totals[1])
    assert need == 64 * totals[1]
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    args = (d.data_ptr(), c.data_ptr(), c.numel(), o.data_ptr(), out.data_ptr(), out.numel(), 1, totals[1], totals[2])
    assert L.poem_jpeg_reconstruct(*args, None, 0, hip.stream()) == -2                       # POEM_E_WORKSPACE
    assert L.poem_jpeg_reconstruct(*args, ws.data_ptr(), need - 1, hip.stream()) == -2
    assert L.poem_jpeg_reconstruct(*args[:5], 8 * 8 * 3 - 1, *args[6:], ws.data_ptr(), need, hip.stream()) == 0   # too small an output:
    torch.cuda.synchronize()                                                                                      # the image is left out
    assert (out.cpu().numpy() == GUARD).all()


# ---- warp_views ---------------------------------------------------------------------------------------------------------------------
def _png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.getvalue()


@pytest.mark.parametrize("out", ["f32", "u8"])
def test_warp_views_on_handles_equals_arrays(out):
    jpgs = [ju.encode(ju.make_image(33, 50, 120), "420", quality=90), ju.encode(ju.make_image(40, 24, 25), "422", quality=75),
            ju.encode(ju.make_image(29, 37, 25, grey=True), quality=95, restart_marker_blocks=1)]
    prog = ju.encode(ju.make_image(17, 9, 25), "420", quality=75, progressive=True)
    png = wds.decode_rgb8(_png(ju.make_image(16, 16, 120)))
    mixed = [wds.EncodedImage(jpgs[0]), png, wds.EncodedImage(jpgs[1]), wds.EncodedImage(prog), wds.EncodedImage(jpgs[2])]
    arrays = [ju.pil_decode(jpgs[0]), png, ju.pil_decode(jpgs[1]), ju.pil_decode(prog), ju.pil_decode(jpgs[2])]
    rng = np.random.default_rng(11)
    affines = [np.array([[1.3 * np.cos(a), -1.1 * np.sin(a), 3.5 + i], [0.9 * np.sin(a), 1.2 * np.cos(a), -2.25 + i]])
               for i, a in enumerate(rng.uniform(-0.6, 0.6, 5))]
    gains = rng.uniform(0.7, 1.3, (5, 3))
    reset_jpeg_counts()
    got = warp_views(mixed, affines, (36, 28), gains=gains, device=DEV, out=out)
    assert jpeg_counts() == {"taken": 3, "refused": 1}
    ref = warp_views(arrays, affines, (36, 28), gains=gains, device=DEV, out=out)
    assert jpeg_counts() == {"taken": 3, "refused": 1}                      # arrays do not count
    assert got.dtype == ref.dtype and torch.equal(got, ref)
    plain = warp_views(mixed, affines, (36, 28), device=DEV, out=out)       # and without gains
    assert torch.equal(plain, warp_views(arrays, affines, (36, 28), device=DEV, out=out))


# ---- shards ---------------------------------------------------------------------------------------------------------------------------
def _jpeg_records(frames, cams, raw, flip=False):
    recs = []
    for i in range(frames):
        rec = pk.inputs.synthetic_frame(i, n_cams=cams, raw=raw)
        out = {(k[:-4] + ".jpg" if k.endswith(".png") else k): v for k, v in rec.items()}
        if flip:
            out["label.pyd"]["request_flip"] = True
        recs.append(out)
    return recs


def _batch(url, mode, seed, view_range=None, **tf):
    random.seed(seed)
    np.random.seed(seed)
    node = wds.dataset_cfg(url, view_range=view_range, image_size=(64, 64), device=DEV, **tf)
    dset = wds.MultiviewWebDataset(node, is_train=bool(tf.get("aug")), defer_images=True, image_decode=mode)
    frames = list(dset)
    handles = sum(isinstance(x, wds.EncodedImage) for f in frames for x in f["raw_image"])
    out = wds.collation_random_n_views(frames, transform=dset.transform)
    return out, (random.random(), float(np.random.rand())), handles


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k].cpu(), b[k].cpu()), k
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert str(a[k]) == str(b[k]), k


@pytest.mark.parametrize("case", ["plain", "flip", "aug_occlusion"])
def test_shard_frames_equal_the_host_route(tmp_path, case):
    url = str(tmp_path / "Synth_mv_test-000000.tar")
    # 64x48 views; with the occlusion on, 320x240: a patch is only drawn when it fits inside the view, and at 64x48 none ever does
    raw = (320, 240) if case == "aug_occlusion" else (64, 48)
    wds.write_shard(url, _jpeg_records(2, 3, raw, flip=case == "flip"), quality=95)
    tf = dict(aug=True, OCCLUSION=True, OCCLUSION_PROB=0.9) if case == "aug_occlusion" else {}
    host, host_rng, none = _batch(url, "host", 3, **tf)
    reset_jpeg_counts()
    dev, dev_rng, handles = _batch(url, "device", 3, **tf)
    counts = jpeg_counts()
    _same(host, dev)
    assert host_rng == dev_rng                                  # both routes consumed the generators alike
    assert host["image"].shape == (6, 3, 64, 64) and counts == {"taken": 6 if case == "flip" else handles, "refused": 0} and none == 0
    # flip: the mirror warp decoded the 6 handles on the device and handed arrays on; occlusion (seed 3): the views that got a patch
    # were materialised on the host, the others stayed handles
    assert handles == {"plain": 6, "flip": 0, "aug_occlusion": OCCLUDED_HANDLES}[case]


# ---- scripts/eval_single.py ---------------------------------------------------------------------------------------------------------
def test_eval_single_image_decode_device(tmp_path):
    spec = importlib.util.spec_from_file_location("eval_single_jpeg", os.path.join(ROOT, "scripts", "eval_single.py"))
    es = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(es)
    args = es.build_cli().parse_args(["--cfg", "x", "--dataset", "DexYCB", "--view_min", "2", "--view_max", "4", "--model", "small",
                                         "-g", "0", "--shards", "d", "--image-decode", "device"])
    assert args.image_decode == "device"
    assert not hasattr(es.build_cli().parse_args(["--cfg", "x", "--dataset", "DexYCB", "--view_min", "2", "--view_max", "4",
                                                     "--model", "small", "-g", "0"]), "image_decode")
    cfg = es.default_cfg()
    view_range = es.edit_cfg(cfg, "DexYCB", "small", [2, 4])
    shard_dir = tmp_path / "shards"
    shard_dir.mkdir()
    urls = wds.expand_urls(os.path.join(str(shard_dir), os.path.basename(cfg["DATASET"]["TEST"]["TARGET"]["URLS"])))
    per = -(-4 // len(urls))
    for si, u in enumerate(urls):
        recs = [pk.inputs.synthetic_frame(si * per + i, n_cams=4, raw=(160, 120)) for i in range(per)]
        wds.write_shard(u, [{(k[:-4] + ".jpg" if k.endswith(".png") else k): v for k, v in r.items()} for r in recs], quality=95)
    kw = dict(shard_dir=str(shard_dir), dataset="DexYCB", epoch_size=4, batch_size=2, backbone="resnet18", backbone_engine="hip")
    lines = {}
    for mode in ("host", "device"):
        random.seed(0)
        np.random.seed(0)
        lines[mode] = es.evaluate_shards(cfg, view_range, "small", torch.device(DEV), image_decode=mode, **kw)
    assert set(lines["device"]) - set(lines["host"]) == {"jpeg_device_fraction"} and set(lines["host"]) <= set(lines["device"])
    assert lines["device"]["jpeg_device_fraction"] == 1.0 and lines["host"]["samples"] == 4
    for k in set(lines["host"]) - {"samples_per_s_rank0"}:
        assert lines["host"][k] == lines["device"][k], k
