"""Huffman decoding on the device (csrc/jpeg_entropy.hip): the kernels against the plain-loop host driver of the same algorithm
(``poem_jpeg_entropy_parallel_host``) and against the serial decoder (``poem_jpeg_entropy_decode``) -- same verdicts, same
coefficient bytes, guard bytes around every buffer untouched --, then the route end to end: ``warp_views(jpeg_entropy="device")``,
``image_decode="device-entropy"`` shards and ``evaluate_shards``.  Every comparison is exact."""
import importlib.util
import io
import os
import random

import numpy as np
import pytest
import torch

import jpeg_entropy_util as eu
import jpeg_util as ju
import poem_v2_amd as pk
from poem_v2_amd import wds
from poem_v2_amd.transform import jpeg_counts, reset_jpeg_counts, warp_views

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def good():
    """The grid, the narrow set and the saturated noise, with the serial decoder's result: computed once."""
    cases = eu.good_streams()
    streams = [d for _, d in cases]
    return [n for n, _ in cases], streams, ju.entropy_decode(streams, threads=8)


@pytest.mark.parametrize("subseq", [16, 0])
def test_kernels_equal_both_host_decoders(good, subseq):
    """548 ragged images in ONE call: statuses all 0, descriptors untouched, coefficients byte-equal to the serial decoder and to
    the host driver, and the rounds the host driver took."""
    names, streams, (rd, rc, rt) = good
    d, c, status, rounds, totals = eu.device_decode(streams, subseq)
    assert status == [0] * len(streams) and totals[:4] == rt and bytes(d) == bytes(rd)
    assert not eu.same_result(d, c, rd, rc, names)
    assert np.array_equal(c[:rt[0] // 2], rc[:rt[0] // 2])
    hd, hc, ht, hrounds = eu.parallel_host(streams, subseq)
    assert np.array_equal(c[:rt[0] // 2], hc[:rt[0] // 2]) and rounds == hrounds
    subs = eu.sub_counts(streams, subseq)
    assert all(r <= s for r, s in zip(rounds, subs))


def test_targeted_streams_on_the_device():
    cases = eu.targeted_streams()
    streams = [d for _, d in cases]
    rd, rc, rt = ju.entropy_decode(streams)
    for subseq, lanes in ((16, 64), (0, 0)):
        d, c, status, rounds, totals = eu.device_decode(streams, subseq, lanes)
        assert status == [0] * len(cases) and bytes(d) == bytes(rd)
        assert not eu.same_result(d, c, rd, rc, [n for n, _ in cases])


def test_damaged_streams_are_refused_cleanly_beside_good_ones(good):
    """About 100 cases of the damage sweep and the ten named refusals in one call, good streams in between: every verdict is the
    serial decoder's, the good neighbours are taken and equal, the statuses stand in the descriptors too, and the guard bytes
    around coefficients, statuses and workspace are untouched (checked by device_decode)."""
    names, streams, _ = good
    damaged = eu.damage_sweep()[::4] + list(eu.refusal_cases().items())
    cases = []
    for k, item in enumerate(damaged):
        cases.append(item)
        if k % 5 == 0:
            cases.append((names[(7 * k) % len(names)], streams[(7 * k) % len(names)]))
    all_streams = [d for _, d in cases]
    rd, rc, rt = ju.entropy_decode(all_streams)
    refused = sum(x.status != 0 for x in rd)
    assert 40 < refused < len(cases) - 30
    for subseq in (16, 0):
        d, c, status, rounds, totals = eu.device_decode(all_streams, subseq)
        assert not eu.same_result(d, c, rd, rc, [n for n, _ in cases])
        assert [x.status for x in d] == status                           # what poem_jpeg_reconstruct will skip
        assert [s == 0 for s in status] == [x.status == 0 for x in rd]
        hd, hc, ht, hr = eu.parallel_host(all_streams, subseq)
        assert [x.status for x in hd] == status                         # the kernels give the driver's code, not only its verdict


@pytest.mark.parametrize("lanes", [64, 0, 1024])
def test_more_subsequences_than_lanes(lanes):
    """96 x 128 noise at q95: over 600 subsequences of 16 bytes, so the lanes of a 64-wide workgroup stride ten times and the fixed
    point takes many rounds; also beside a small image, whose workgroup finishes early."""
    big, small = eu.large_stream(), ju.grid()[3][1]
    streams = [small, big, small]
    assert eu.sub_counts(streams, 16)[1] > 600
    rd, rc, rt = ju.entropy_decode(streams)
    d, c, status, rounds, totals = eu.device_decode(streams, 16, lanes)
    assert status == [0, 0, 0] and not eu.same_result(d, c, rd, rc)
    assert rounds[1] > 4 and rounds == eu.parallel_host(streams, 16)[3]


# ---- warp_views ---------------------------------------------------------------------------------------------------------------------
def _png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return wds.decode_rgb8(buf.getvalue())


def _affines(n, seed=11):
    rng = np.random.default_rng(seed)
    return [np.array([[1.3 * np.cos(a), -1.1 * np.sin(a), 3.5 + i], [0.9 * np.sin(a), 1.2 * np.cos(a), -2.25 + i]])
            for i, a in enumerate(rng.uniform(-0.6, 0.6, n))], rng.uniform(0.7, 1.3, (n, 3))


@pytest.mark.parametrize("out", ["f32", "u8"])
def test_warp_views_with_device_entropy_equals_pil(out):
    jpgs = [ju.encode(ju.make_image(33, 50, 120), "420", quality=90), ju.encode(ju.make_image(40, 24, 25), "422", quality=75),
            ju.encode(ju.make_image(29, 37, 25, grey=True), quality=95, restart_marker_blocks=1),
            ju.encode(ju.make_image(17, 9, 25), "444", quality=90, optimize=True)]
    affines, gains = _affines(4)
    reset_jpeg_counts()
    got = warp_views([wds.EncodedImage(j) for j in jpgs], affines, (36, 28), gains=gains, device=DEV, out=out, jpeg_entropy="device")
    assert jpeg_counts() == {"taken": 4, "refused": 0, "entropy_device": 4, "redone": 0}
    ref = warp_views([ju.pil_decode(j) for j in jpgs], affines, (36, 28), gains=gains, device=DEV, out=out)
    assert got.dtype == ref.dtype and torch.equal(got, ref)
    marked = warp_views([wds.EncodedImage(j, entropy="device") for j in jpgs], affines, (36, 28), gains=gains, device=DEV, out=out)
    assert torch.equal(marked, ref) and jpeg_counts()["entropy_device"] == 8          # a handle's own mark selects the route too


@pytest.mark.parametrize("out", ["f32", "u8"])
def test_mixed_call_with_a_damaged_scan_is_redone_on_the_host_route(out):
    good = [ju.encode(ju.make_image(33, 50, 120), "420", quality=90), ju.encode(ju.make_image(40, 24, 25), "422", quality=75)]
    prog = ju.encode(ju.make_image(17, 9, 25), "420", quality=75, progressive=True)           # refused by the headers
    base = eu.damage_bases()[0][1]
    hurt = base[:eu.scan_start(base) + 40] + b"\xff\xd9"                                     # the scan ends early: refused there
    assert [x.status for x in ju.entropy_decode([prog, hurt])[0]] == [1, 2]
    png = _png(ju.make_image(16, 16, 120))
    streams = [good[0], None, prog, hurt, good[1]]
    mixed = [png if s is None else wds.EncodedImage(s) for s in streams]
    affines, gains = _affines(5)
    reset_jpeg_counts()
    host = warp_views(mixed, affines, (36, 28), gains=gains, device=DEV, out=out)
    assert jpeg_counts() == {"taken": 2, "refused": 2}
    reset_jpeg_counts()
    got = warp_views(mixed, affines, (36, 28), gains=gains, device=DEV, out=out, jpeg_entropy="device")
    assert jpeg_counts() == {"taken": 2, "refused": 2, "entropy_device": 0, "redone": 1}
    assert torch.equal(got, host)
    arrays = [png if s is None else ju.pil_decode(s) for s in streams]
    pil = warp_views(arrays, affines, (36, 28), gains=gains, device=DEV, out=out)
    for v in (0, 1, 2, 4):                                                                   # the good images' pixels are PIL's
        assert torch.equal(got[v], pil[v]), v
    # without the damaged one nothing is redone: the header refusal goes to PIL before the upload
    reset_jpeg_counts()
    keep = [0, 1, 2, 4]
    got = warp_views([mixed[v] for v in keep], [affines[v] for v in keep], (36, 28), gains=gains[keep], device=DEV, out=out,
                     jpeg_entropy="device")
    assert jpeg_counts() == {"taken": 2, "refused": 1, "entropy_device": 2, "redone": 0}
    assert torch.equal(got, pil[keep])


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


def _batch(url, mode, seed, **tf):
    random.seed(seed)
    np.random.seed(seed)
    node = wds.dataset_cfg(url, image_size=(64, 64), device=DEV, **tf)
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
    raw = (320, 240) if case == "aug_occlusion" else (64, 48)
    wds.write_shard(url, _jpeg_records(2, 3, raw, flip=case == "flip"), quality=95)
    tf = dict(aug=True, OCCLUSION=True, OCCLUSION_PROB=0.9) if case == "aug_occlusion" else {}
    host, host_rng, none = _batch(url, "host", 3, **tf)
    reset_jpeg_counts()
    dev, dev_rng, handles = _batch(url, "device-entropy", 3, **tf)
    counts = jpeg_counts()
    _same(host, dev)
    assert host_rng == dev_rng and none == 0 and host["image"].shape == (6, 3, 64, 64)
    assert counts["redone"] == 0 and counts["refused"] == 0 and counts["entropy_device"] == counts["taken"] > 0
    if case == "plain":
        assert handles == 6 and counts["taken"] == 6


# ---- scripts/eval_single.py ---------------------------------------------------------------------------------------------------------
def test_eval_single_image_decode_device_entropy(tmp_path):
    spec = importlib.util.spec_from_file_location("eval_single_jpeg_entropy", os.path.join(ROOT, "scripts", "eval_single.py"))
    es = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(es)
    args = es.build_cli().parse_args(["--cfg", "x", "--dataset", "DexYCB", "--view_min", "2", "--view_max", "4", "--model", "small",
                                         "-g", "0", "--shards", "d", "--image-decode", "device-entropy"])
    assert args.image_decode == "device-entropy"
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
    for mode in ("host", "device-entropy"):
        random.seed(0)
        np.random.seed(0)
        lines[mode] = es.evaluate_shards(cfg, view_range, "small", torch.device(DEV), image_decode=mode, **kw)
    assert set(lines["device-entropy"]) - set(lines["host"]) == {"jpeg_device_fraction"}
    assert lines["device-entropy"]["jpeg_device_fraction"] == 1.0 and lines["host"]["samples"] == 4
    assert pk.transform.jpeg_counts()["entropy_device"] > 0 and pk.transform.jpeg_counts()["redone"] == 0
    for k in set(lines["host"]) - {"samples_per_s_rank0"}:
        assert lines["host"][k] == lines["device-entropy"][k], k
