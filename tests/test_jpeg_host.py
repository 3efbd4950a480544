"""The device JPEG route, host side (no GPU): the arithmetic of csrc/jpeg.h against PIL -- once restated in numpy (jpeg_util, with
its own Huffman reader) and once through the library's plain loops --, the entropy decoder against that restatement, what is
refused, the ``EncodedImage`` handle and the record reader's ``images=`` / ``image_decode=`` keywords.  Every comparison is
``array_equal`` against ``np.asarray(Image.open(...).convert("RGB"))`` on the same bytes: there is no tolerance."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_util as ju
import poem_v2_amd as pk
from poem_v2_amd import hip, wds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def grid_decoded():
    """One entropy decode of all 384 cases (8 threads) + the library's host reconstruction."""
    streams = [d for _, d in ju.grid()]
    descs, coef, totals = ju.entropy_decode(streams, threads=8)
    return descs, coef, totals, ju.reconstruct_host(descs, coef, totals)


def test_numpy_restatement_equals_pil_on_the_grid():
    bad = [name for (name, data), ref in zip(ju.grid(), ju.grid_reference()) if not np.array_equal(ju.decode(data), ref)]
    assert not bad, bad


def test_entropy_decode_matches_the_restatement(grid_decoded):
    descs, coef, totals, _ = grid_decoded
    blocks = quads = 0
    for (name, data), d in zip(ju.grid(), descs):
        p = ju.parse(data)
        assert d.status == 0, name                                                     # admission: no fallback on the grid
        assert (d.height, d.width, d.ncomp, d.hs, d.vs) == (p["height"], p["width"], p["ncomp"], p["hs"], p["vs"]), name
        assert (d.block_base, d.quad_base) == (blocks, quads) and d.coef_offset % 16 == 0, name
        for c in range(d.ncomp):
            assert (d.blocks_h[c], d.blocks_w[c]) == p["coef"][c].shape[:2], name
            assert np.array_equal(np.ctypeslib.as_array(d.quant[c]), p["quant"][c]), name
            assert np.array_equal(ju.desc_coef(d, coef, c), p["coef"][c]), name
        blocks += sum(d.blocks_h[c] * d.blocks_w[c] for c in range(d.ncomp))
        quads += d.height * ((d.width + 3) // 4)
    assert totals[1:] == [blocks, quads, 384]


def test_entropy_decode_does_not_depend_on_threads(grid_decoded):
    descs8, coef8, totals8, _ = grid_decoded
    descs1, coef1, totals1 = ju.entropy_decode([d for _, d in ju.grid()], threads=1)
    assert totals1 == totals8 and bytes(descs1) == bytes(descs8) and np.array_equal(coef1, coef8)
    descs0, coef0, totals0 = ju.entropy_decode([d for _, d in ju.grid()], threads=1000)       # clamped to the library's maximum
    assert totals0 == totals8 and np.array_equal(coef0, coef8)


def test_host_reconstruction_equals_pil(grid_decoded):
    outs = grid_decoded[3]
    bad = [name for (name, _), out, ref in zip(ju.grid(), outs, ju.grid_reference()) if out is None or not np.array_equal(out, ref)]
    assert not bad, bad


def test_narrow_images_are_taken_and_equal():
    """Width <= 4 at 4:2:2 / 4:2:0: libjpeg replicates a chroma component at most 2 samples wide instead of interpolating it
    (jdsample.c); widths 5 and 6 are the first on the fancy path.  Restatement, entropy decoder and host loops, all against PIL."""
    cases = ju.narrow()
    refs = [ju.pil_decode(d) for _, d in cases]
    descs, coef, totals = ju.entropy_decode([d for _, d in cases])
    outs = ju.reconstruct_host(descs, coef, totals)
    assert [d.status for d in descs] == [0] * len(cases)
    bad = [n for (n, d), o, r in zip(cases, outs, refs) if not np.array_equal(o, r) or not np.array_equal(ju.decode(d), r)]
    assert not bad, bad
    # the rule matters: interpolating the 2-wide chroma of a 16x4 image moves pixels
    p = ju.parse(dict(cases)["16x4-a120-420-q100"])
    wide = ju.reconstruct(p)
    p["width"] = 6                                         # the same planes read as a wider image take the fancy path
    assert not np.array_equal(ju.reconstruct(p)[:, :4], wide)


def test_saturated_noise_is_taken_and_equal():
    for sampling in ("444", "420"):
        data = ju.encode(ju.saturated_noise(), sampling, quality=100)
        descs, coef, totals = ju.entropy_decode([data])
        assert descs[0].status == 0 and ju.block_l1(ju.parse(data)) <= 5900
        assert np.array_equal(ju.reconstruct_host(descs, coef, totals)[0], ju.pil_decode(data))
        assert np.array_equal(ju.decode(data), ju.pil_decode(data))


def test_range_guard_admits_what_the_issue_measured():
    """The bound of csrc/jpeg.h (block L1 <= 5900) against the data it must admit, with room to spare: the grid (this grid's largest
    block measures 4041) and saturated 0/255 noise at quality 100 (5043); and the DQT-patched streams lie far outside it."""
    worst = max(ju.block_l1(ju.parse(data)) for _, data in ju.grid())
    noise = ju.block_l1(ju.parse(ju.encode(ju.saturated_noise(), "444", quality=100)))
    assert worst <= 5900 and noise <= 5900, (worst, noise)
    assert ju.block_l1(ju.parse(_patch_dqt(ju.encode(ju.make_image(40, 24, 120), "422", quality=100), 16))) > 4 * 5900


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _patch_dqt(data, value):
    """Every entry of every 8-bit quantisation table -> value."""
    out, pos = bytearray(data), 2
    while out[pos + 1] != 0xDA:
        ln = int.from_bytes(out[pos + 2:pos + 4], "big")
        if out[pos + 1] == 0xDB:
            p = pos + 4
            while p < pos + 2 + ln:
                out[p + 1:p + 65] = bytes([value]) * 64
                p += 65
        pos += 2 + ln
    return bytes(out)


def _find(data, marker):
    pos = 2
    while data[pos + 1] != marker:
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    return pos


def _refusal_cases():
    from PIL import Image
    rgb = ju.make_image(40, 24, 120)
    base = ju.encode(rgb, "422", quality=100)
    cases = {}
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=75, progressive=True)
    cases["progressive"] = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(np.dstack([rgb, rgb[..., :1]]), "CMYK").save(buf, format="JPEG", quality=75)
    cases["cmyk"] = buf.getvalue()
    for v in (16, 64, 255):
        cases[f"dqt{v}"] = _patch_dqt(base, v)
    sos = _find(base, 0xDA)
    cases["cut_mid_scan"] = base[:sos + (len(base) - sos) // 2]
    dht = _find(base, 0xC4)
    bad = bytearray(base)
    bad[dht + 5:dht + 21] = bytes([255]) * 16                      # 255 codes of every length: not a prefix code
    cases["corrupt_huffman"] = bytes(bad)
    sof = _find(base, 0xC0)
    assert base[sof + 11] == 0x21 and base[sof + 14] == 0x11     # 2x1 luma, 1x1 chroma
    bad = bytearray(base)
    bad[sof + 14] = 0x21                                           # Cb sampling -> 2x1
    cases["chroma_2x1"] = bytes(bad)
    bad = bytearray(base)                                          # 'R','G','B' component ids (frame and scan headers): libjpeg reads
    for k, ch in enumerate(b"RGB"):                                # them as RGB unless a JFIF / Adobe segment says otherwise
        bad[sof + 10 + 3 * k] = ch
        bad[sos + 5 + 2 * k] = ch
    cases["rgb_ids"] = bytes(bad)
    app0 = _find(base, 0xE0)
    cases["rgb_ids_no_jfif"] = bytes(bad[:app0]) + bytes(bad[app0 + 2 + int.from_bytes(base[app0 + 2:app0 + 4], "big"):])
    return cases


@pytest.fixture(scope="module")
def refusals():
    return _refusal_cases()


@pytest.mark.parametrize("name", ["progressive", "cmyk", "dqt16", "dqt64", "dqt255", "cut_mid_scan", "corrupt_huffman", "chroma_2x1", "rgb_ids",
                                  "rgb_ids_no_jfif"])
def test_refused_and_the_handle_still_follows_pil(refusals, name):
    from PIL import Image
    data = refusals[name]
    descs, coef, totals = ju.entropy_decode([data, ju.grid()[0][1]])          # beside a good stream: that one is still taken
    assert descs[0].status in (1, 2, 3) and descs[1].status == 0 and totals[3] == 1
    assert np.array_equal(ju.reconstruct_host(descs, coef, totals)[1], ju.grid_reference()[0])
    try:
        with Image.open(io.BytesIO(data)) as im:
            ref = np.asarray(im.convert("RGB"))
    except Exception as e:                                                     # where PIL raises, so does the handle
        try:
            h = wds.EncodedImage(data)
        except ValueError:
            return
        with pytest.raises(type(e)):
            np.asarray(h)
        return
    assert np.array_equal(np.asarray(wds.EncodedImage(data)), ref)


def test_the_refusal_set_is_exactly_the_named_one(refusals, grid_decoded):
    """Nothing of the grid (nor the saturated-noise stream, test above) is refused: the cap on fallbacks there is zero; and the
    named streams are refused for the reason that fits them."""
    assert [d.status for d in grid_decoded[0]] == [0] * 384
    descs, _, _ = ju.entropy_decode(list(refusals.values()))
    got = {k: d.status for k, d in zip(refusals, descs)}
    assert got == {"progressive": 1, "cmyk": 1, "dqt16": 3, "dqt64": 3, "dqt255": 3, "cut_mid_scan": 2, "corrupt_huffman": 2,
                   "chroma_2x1": 1, "rgb_ids": 1, "rgb_ids_no_jfif": 1}, got


def test_argument_checks_and_the_size_query():
    import ctypes
    L = hip.lib()
    data = ju.grid()[5][1]
    buf = np.frombuffer(data, np.uint8)
    ptrs, lens = (ctypes.c_void_p * 1)(buf.ctypes.data), (ctypes.c_int64 * 1)(len(data))
    descs, totals = (pk.jpeg.JpegDesc * 1)(), (ctypes.c_int64 * 4)()
    assert L.poem_jpeg_entropy_decode(None, lens, 1, descs, None, 0, totals, 1) == -1
    assert L.poem_jpeg_entropy_decode(ptrs, lens, 0, descs, None, 0, totals, 1) == -1
    assert L.poem_jpeg_entropy_decode(ptrs, lens, 65536, descs, None, 0, totals, 1) == -4      # POEM_E_UNSUPPORTED, before any read
    assert L.poem_jpeg_entropy_decode(ptrs, lens, 1, descs, None, 0, totals, 1) == 0 and totals[0] == descs[0].coef_bytes > 0
    coef = np.zeros(totals[0] // 2 + 8, np.int16)
    coef = coef[(-coef.ctypes.data % 16) // 2:]
    guard = coef.copy()
    assert L.poem_jpeg_entropy_decode(ptrs, lens, 1, descs, coef.ctypes.data, totals[0] - 2, totals, 1) == -2     # POEM_E_WORKSPACE
    assert np.array_equal(coef, guard)                                                                            # nothing written
    assert L.poem_jpeg_entropy_decode(ptrs, lens, 1, descs, coef.ctypes.data + 2, totals[0], totals, 1) == -1     # misaligned
    assert L.poem_jpeg_workspace_bytes(10) == 640 and L.poem_jpeg_workspace_bytes(0) == 0
    assert L.poem_jpeg_reconstruct(None, None, 0, None, None, 0, 1, 1, 1, None, 0, None) == -1


# ---- handles and the record reader --------------------------------------------------------------------------------------------
def test_encoded_image_shape_and_pixels():
    for (name, data), ref in list(zip(ju.grid(), ju.grid_reference()))[::7]:
        h = wds.EncodedImage(data)
        assert h.shape == ref.shape == np.shape(h) and h.size == ref.size and h.dtype == np.uint8 and h.ndim == 3, name
        assert np.array_equal(np.asarray(h), ref), name
    patched = np.array(h, copy=True)
    patched[0:1, 0:1, :] = 7.9                                   # what the occlusion patch does: float -> uint8 on assignment
    assert patched[0, 0, 0] == 7
    with pytest.raises(ValueError):
        wds.EncodedImage(b"\x89PNG....")


def test_decode_record_leaves_only_jpeg_members_encoded():
    from PIL import Image
    rgb = ju.make_image(17, 9, 25)
    png = io.BytesIO()
    Image.fromarray(rgb).save(png, format="PNG")
    jpg = ju.encode(rgb, "420", quality=90)
    rec = {"__key__": "k", "image_0.jpg": jpg, "image_1.png": png.getvalue(), "image_2.jpeg": jpg, "note.txt": b"x"}
    host = wds.decode_record(dict(rec))
    assert host.keys() == wds.decode_record(dict(rec), images="host").keys()
    dev = wds.decode_record(dict(rec), images="device")
    assert isinstance(dev["image_0.jpg"], wds.EncodedImage) and isinstance(dev["image_2.jpeg"], wds.EncodedImage)
    assert isinstance(dev["image_1.png"], np.ndarray) and np.array_equal(dev["image_1.png"], rgb) and dev["note.txt"] == "x"
    for k in ("image_0.jpg", "image_2.jpeg"):
        assert isinstance(host[k], np.ndarray) and np.array_equal(np.asarray(dev[k]), host[k]) and dev[k].shape == host[k].shape
    with pytest.raises(ValueError):
        wds.decode_record(dict(rec), images="gpu")


def _write_jpeg_shard(path, frames=2, cams=3, raw=(64, 48), flip=False):
    recs = []
    for i in range(frames):
        rec = pk.inputs.synthetic_frame(i, n_cams=cams, raw=raw)
        out = {}
        for k, v in rec.items():
            out[k[:-4] + ".jpg" if k.endswith(".png") else k] = v
        if flip:
            out["label.pyd"]["request_flip"] = True
        recs.append(out)
    wds.write_shard(path, recs, quality=95)
    return recs


def test_host_keyword_gives_todays_frames(tmp_path):
    """``image_decode="host"`` (and no keyword) yields exactly the frames of the parent: same keys, same raw pixels, same labels.
    Deferred images, so nothing here needs the GPU."""
    url = str(tmp_path / "Synth_mv_test-000000.tar")
    _write_jpeg_shard(url)
    node = wds.dataset_cfg(url, device="cpu")
    a = list(wds.MultiviewWebDataset(node, is_train=False, defer_images=True))
    b = list(wds.MultiviewWebDataset(node, is_train=False, defer_images=True, image_decode="host"))
    c = list(wds.MultiviewWebDataset(node, is_train=False, defer_images=True, image_decode="device"))
    assert len(a) == len(b) == len(c) == 2
    for fa, fb, fc in zip(a, b, c):
        assert fa.keys() == fb.keys() == fc.keys()
        for k in fa:
            if k == "raw_image":
                assert all(isinstance(x, np.ndarray) for x in fa[k] + fb[k]) and all(isinstance(x, wds.EncodedImage) for x in fc[k])
                assert all(np.array_equal(x, y) and np.array_equal(x, np.asarray(z)) for x, y, z in zip(fa[k], fb[k], fc[k]))
            elif isinstance(fa[k], np.ndarray):
                assert np.array_equal(fa[k], fb[k]) and np.array_equal(fa[k], fc[k]), k
            elif not isinstance(fa[k], list) or not any(isinstance(x, np.ndarray) for x in fa[k]):
                assert fa[k] == fb[k] == fc[k], k
    with pytest.raises(ValueError):
        wds.MultiviewWebDataset(node, is_train=False, image_decode="gpu")


def test_occlusion_patch_materialises_a_handle_on_the_host():
    t = pk.build_transform(pk.CN({"TYPE": "SimpleTransform3DMultiView", "AUG": False, "DEVICE": "cpu"}),
                           data_preset=pk.CN({"IMAGE_SIZE": [64, 64], "CENTER_IDX": 9}), is_train=False)
    rec = pk.inputs.synthetic_frame(0, n_cams=1, raw=(64, 48))
    lab = {k: v[0] for k, v in rec["label.pyd"].items() if isinstance(v, list)}
    h = wds.EncodedImage(ju.encode(rec["image_0.png"], "420", quality=95))
    draw = pk.transform.ViewDraw(lab["bbox_center"], lab["bbox_scale"], patch=(3, 2, 5, 4, np.full((4, 5, 3), 200.7)))
    plain = pk.transform.ViewDraw(lab["bbox_center"], lab["bbox_scale"])
    out = t.frame_labels([h, h], [lab, lab], [draw, plain])
    ref = np.asarray(h).copy()
    ref[2:6, 3:8, :] = 200
    assert isinstance(out[0]["raw_image"], np.ndarray) and np.array_equal(out[0]["raw_image"], ref)
    assert out[1]["raw_image"] is h


# ---- the stand-alone sanitizer program ------------------------------------------------------------------------------------------
def test_hostcheck_builds_and_exits_zero(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_hostcheck")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "jpeg_hostcheck.cpp"),
           os.path.join(ROOT, "poem-v2_amd", "csrc", "jpeg.cpp"), "-o", exe, "-lpthread"]
    probe = tmp_path / "probe.cpp"                                 # does this compiler have the sanitizer runtimes at all?
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(cmd[:6] + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime: " + probed.stderr[-300:])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    files = []
    for i, (data) in enumerate([ju.encode(ju.make_image(17, 9, 25), "420", quality=75),
                                ju.encode(ju.make_image(16, 16, 120), "422", quality=95, restart_marker_blocks=1),
                                ju.encode(ju.make_image(8, 8, 25, grey=True), quality=90, optimize=True)]):
        files.append(str(tmp_path / f"case{i}.jpg"))
        with open(files[-1], "wb") as f:
            f.write(data)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert " 0 bad" in run.stdout, run.stdout
