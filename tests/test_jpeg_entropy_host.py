"""The parallel entropy decoder, host side (no GPU): ``poem_jpeg_entropy_parallel_host`` -- the plain-loop driver of the algorithm
the kernels run (csrc/jpeg_entropy.h: subsequences, fixed point, prefix sum, write pass, DC pass, block pass) -- against the serial
decoder ``poem_jpeg_entropy_decode``.  Everywhere: the same verdict (taken / refused), header-stage codes equal, and where taken the
same coefficient BYTES; there is no tolerance.  Plus the keyword plumbing of the route and the ABI's argument checks."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_entropy_util as eu
import jpeg_util as ju
import poem_v2_amd as pk
from poem_v2_amd import hip, wds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [16, 128]


@pytest.fixture(scope="module")
def serial_good():
    streams = [d for _, d in eu.good_streams()]
    return streams, ju.entropy_decode(streams, threads=8)


def _check_rounds(streams, rounds, subseq):
    subs = eu.sub_counts(streams, subseq)
    over = [(i, r, s) for i, (r, s) in enumerate(zip(rounds, subs)) if r > s]
    assert not over, over


@pytest.mark.parametrize("subseq", SIZES)
def test_grid_narrow_and_saturated_noise_equal_the_serial_decoder(serial_good, subseq):
    """All 384 grid streams, the 162 narrow ones and the saturated noise: every one taken (the cap on fallbacks is zero) and
    byte-equal, descriptors included."""
    streams, (rd, rc, rt) = serial_good
    d, c, totals, rounds = eu.parallel_host(streams, subseq)
    assert [x.status for x in d] == [0] * len(streams) == [x.status for x in rd]
    assert totals == rt and bytes(d) == bytes(rd)
    assert not eu.same_result(d, c, rd, rc, [n for n, _ in eu.good_streams()])
    assert np.array_equal(c[:rt[0] // 2], rc[:rt[0] // 2])
    _check_rounds(streams, rounds, subseq)


@pytest.mark.parametrize("subseq", SIZES)
def test_named_refusals_get_the_serial_verdict(subseq):
    cases = eu.refusal_cases()
    streams = list(cases.values()) + [ju.grid()[0][1]]                 # beside a good stream: that one is still taken
    rd, rc, rt = ju.entropy_decode(streams)
    d, c, totals, rounds = eu.parallel_host(streams, subseq)
    assert not eu.same_result(d, c, rd, rc, list(cases) + ["good"])
    got = {k: x.status for k, x in zip(cases, d)}
    for k in ("progressive", "cmyk", "chroma_2x1", "rgb_ids", "rgb_ids_no_jfif"):      # header stage: the code itself
        assert got[k] == 1, got
    assert got["corrupt_huffman"] == 2 and all(got[k] in (2, 3) for k in ("dqt16", "dqt64", "dqt255", "cut_mid_scan")), got
    assert d[len(cases)].status == 0 and totals[3] == rt[3] == 1
    _check_rounds(streams, rounds, subseq)


@pytest.mark.parametrize("subseq", SIZES)
def test_damage_sweep_gets_the_serial_verdict(subseq):
    """360 seeded single-byte edits and truncations inside the scans of a 4:2:0 q75 stream, a 4:4:4 q90 optimised one (codes
    longer than 9 bits: the slow path) and a 4:2:2 q95 one with a restart marker after every MCU."""
    cases = eu.damage_sweep()
    streams = [d for _, d in cases]
    rd, rc, rt = ju.entropy_decode(streams)
    d, c, totals, rounds = eu.parallel_host(streams, subseq)
    assert not eu.same_result(d, c, rd, rc, [n for n, _ in cases])
    taken = sum(x.status == 0 for x in rd)
    assert 20 < taken < len(cases) - 100, taken                         # the sweep holds both kinds, in numbers
    _check_rounds(streams, rounds, subseq)


@pytest.mark.parametrize("subseq", SIZES)
def test_targeted_streams(subseq):
    """Flat images (DC + EOB blocks, with 1-bit codes several MCUs end inside one byte), ZRL-bearing blocks, restart intervals
    longer and shorter than a subsequence (and past RST7), greyscale."""
    cases = eu.targeted_streams()
    streams = [d for _, d in cases]
    rd, rc, rt = ju.entropy_decode(streams)
    assert [x.status for x in rd] == [0] * len(cases)
    d, c, totals, rounds = eu.parallel_host(streams, subseq)
    assert bytes(d) == bytes(rd) and not eu.same_result(d, c, rd, rc, [n for n, _ in cases])
    _check_rounds(streams, rounds, subseq)
    for (name, data), x in zip(cases, rd):                              # the streams are what their names say
        p = ju.parse(data)
        if name.startswith("flat"):
            assert all(not cc[..., 1:].any() for cc in p["coef"]), name
    for name in ("hf77-grey-q90", "hf77-444-q90"):                                  # a run of 16 zeros and more in front of a
        zz = ju.parse(dict(cases)[name])["coef"][0][..., ju.ZIGZAG].reshape(-1, 64)   # coefficient: coded with ZRL symbols
        runs = [np.diff(np.flatnonzero(np.concatenate([[1], b[1:]]))).max(initial=0) for b in zz]
        assert max(runs) > 16, name


def test_restart_intervals_span_and_share_subsequences():
    """What `rst-long` / `rst-short` are for, checked on the bytes: an interval longer than one subsequence, and several inside one."""
    cases = dict(eu.targeted_streams())

    def gaps(data):
        seg = data[eu.scan_start(data):]
        at = [i for i in range(len(seg) - 1) if seg[i] == 0xFF and 0xD0 <= seg[i + 1] <= 0xD7]
        return np.diff(at)
    assert gaps(cases["rst-long-444"]).min() > 128 and gaps(cases["rst-long-420"]).max() > 128
    assert gaps(cases["rst-short-flat"]).max() < 16 and gaps(cases["rst-short-grey"]).max() < 16
    seg = cases["rst-2-grey"][eu.scan_start(cases["rst-2-grey"]):]
    assert seg.count(b"\xff\xd7") >= 1 and seg.count(b"\xff\xd0") >= 2                                  # the numbering wraps


def test_result_does_not_depend_on_the_subsequence_size():
    cases = eu.targeted_streams() + eu.good_streams()[::9] + eu.damage_sweep()[::7] + [("large", eu.large_stream())]
    streams = [d for _, d in cases]
    ref = None
    for subseq in (16, 32, 128, 1024):
        d, c, totals, rounds = eu.parallel_host(streams, subseq)
        verdict = [x.status == 0 for x in d]
        coefs = [c[a:b].copy() for (a, b), ok in zip(eu.taken_ranges(d), verdict) if ok]
        if ref is None:
            ref = (verdict, coefs)
        assert verdict == ref[0] and all(np.array_equal(x, y) for x, y in zip(coefs, ref[1])), subseq
        _check_rounds(streams, rounds, subseq)
    assert eu.sub_counts([eu.large_stream()], 16)[0] > 600


def test_a_tail_the_serial_decoder_reads_out_of_the_last_bits():
    """A truncation that leaves whole MCUs inside the last (< 8) bits in front of the end: the serial decoder reads on there, and
    so must the parallel one (jpeg_finish's tail).  Flat greyscale with optimised tables has 1-bit codes: every cut is tried."""
    data = dict(eu.targeted_streams())["flat-grey-opt"]
    lo = eu.scan_start(data)
    streams = [data[:cut] for cut in range(lo, len(data) + 1)] + [data[:cut] + b"\xff\xd9" for cut in range(lo, len(data))]
    rd, rc, rt = ju.entropy_decode(streams)
    for subseq in SIZES:
        d, c, totals, rounds = eu.parallel_host(streams, subseq)
        assert not eu.same_result(d, c, rd, rc)


# ---- the stand-alone sanitizer program ------------------------------------------------------------------------------------------
def test_entropycheck_builds_and_exits_zero(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_entropycheck")
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "jpeg_entropycheck.cpp"),
           os.path.join(ROOT, "poem-v2_amd", "csrc", "jpeg.cpp"), "-o", exe, "-lpthread"]
    probe = tmp_path / "probe.cpp"                                 # does this compiler have the sanitizer runtimes at all?
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run(cmd[:6] + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if probed.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime: " + probed.stderr[-300:])
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-2000:]
    files = []
    for i, data in enumerate([ju.encode(ju.make_image(17, 9, 25), "420", quality=75),
                              ju.encode(ju.make_image(16, 16, 120), "422", quality=95, restart_marker_blocks=1),
                              ju.encode(ju.make_image(16, 24, 0, grey=True), quality=30, optimize=True)]):
        files.append(str(tmp_path / f"case{i}.jpg"))
        with open(files[-1], "wb") as f:
            f.write(data)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert " 0 bad" in run.stdout, run.stdout


# ---- keywords ------------------------------------------------------------------------------------------------------------------
def test_device_entropy_keyword_yields_marked_handles(tmp_path):
    rgb = ju.make_image(17, 9, 25)
    jpg = ju.encode(rgb, "420", quality=90)
    rec = {"__key__": "k", "image_0.jpg": jpg, "note.txt": b"x"}
    dev = wds.decode_record(dict(rec), images="device")
    ent = wds.decode_record(dict(rec), images="device-entropy")
    assert isinstance(ent["image_0.jpg"], wds.EncodedImage) and type(ent["image_0.jpg"]) is type(dev["image_0.jpg"])
    assert ent["image_0.jpg"].data == dev["image_0.jpg"].data and ent["image_0.jpg"].shape == dev["image_0.jpg"].shape
    assert ent["image_0.jpg"].entropy == "device" and dev["image_0.jpg"].entropy is None and wds.EncodedImage(jpg).entropy is None
    assert np.array_equal(np.asarray(ent["image_0.jpg"]), ju.pil_decode(jpg))
    with pytest.raises(ValueError):
        wds.decode_record(dict(rec), images="device-huffman")
    url = str(tmp_path / "Synth_mv_test-000000.tar")
    recs = []
    for i in range(2):
        r = pk.inputs.synthetic_frame(i, n_cams=3, raw=(64, 48))
        recs.append({(k[:-4] + ".jpg" if k.endswith(".png") else k): v for k, v in r.items()})
    wds.write_shard(url, recs, quality=95)
    node = wds.dataset_cfg(url, device="cpu")
    frames = list(wds.MultiviewWebDataset(node, is_train=False, defer_images=True, image_decode="device-entropy"))
    assert len(frames) == 2 and all(isinstance(x, wds.EncodedImage) and x.entropy == "device" for f in frames for x in f["raw_image"])
    with pytest.raises(ValueError):
        wds.MultiviewWebDataset(node, is_train=False, image_decode="entropy")


def test_the_switch_defaults_to_host_and_rejects_other_values():
    import inspect
    t = pk.transform
    assert t.JPEG_ENTROPY == "host"
    assert inspect.signature(t.warp_views).parameters["jpeg_entropy"].default is None          # None: the switch decides
    with pytest.raises(ValueError):
        t.set_jpeg_entropy("gpu")
    t.set_jpeg_entropy("device", subseq=64, wg_threads=128)
    try:
        assert (t.JPEG_ENTROPY, t.JPEG_SUBSEQ, t.JPEG_WG_THREADS) == ("device", 64, 128)
    finally:
        t.set_jpeg_entropy("host", subseq=0, wg_threads=0)
    assert t.JPEG_ENTROPY == "host"
    with pytest.raises(ValueError):
        t.warp_views([np.zeros((8, 8, 3), np.uint8)], [np.eye(3)], (8, 8), jpeg_entropy="gpu")
    t.reset_jpeg_counts()
    assert t.jpeg_counts() == {"taken": 0, "refused": 0}                 # the new counters appear once the device route has run


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks_and_the_size_query():
    L = hip.lib()
    data = ju.grid()[5][1]
    buf = np.frombuffer(data, np.uint8)
    ptrs, lens = (ctypes.c_void_p * 1)(buf.ctypes.data), (ctypes.c_int64 * 1)(len(data))
    descs, scans, totals = (pk.jpeg.JpegDesc * 1)(), (eu.JpegScan * 1)(), (ctypes.c_int64 * 8)()
    prep = L.poem_jpeg_entropy_prepare
    assert prep(None, lens, 1, 0, descs, scans, None, 0, None, 0, totals) == -1
    assert prep(ptrs, lens, 0, 0, descs, scans, None, 0, None, 0, totals) == -1
    assert prep(ptrs, lens, 1, 0, descs, None, None, 0, None, 0, totals) == -1
    for bad in (8, 24, 2048, -16):
        assert prep(ptrs, lens, 1, bad, descs, scans, None, 0, None, 0, totals) == -1
    assert prep(ptrs, lens, 65536, 0, descs, scans, None, 0, None, 0, totals) == -4
    assert prep(ptrs, lens, 1, 16, descs, scans, None, 0, None, 0, totals) == 0
    ref, _, rt = ju.entropy_decode([data])
    seg = len(data) - eu.scan_start(data)
    assert list(totals[:4]) == rt and list(totals[4:]) == [(seg + 15) & ~15, scans[0].table_count, -(-seg // 16), -(-seg // 16)]
    assert (descs[0].coef_offset, descs[0].block_base, descs[0].quad_base, descs[0].coef_bytes) == (0, 0, 0, ref[0].coef_bytes)
    assert (scans[0].byte_offset, scans[0].byte_count, scans[0].sub_base, scans[0].sub_count) == (0, seg, 0, -(-seg // 16))
    assert 2 <= scans[0].table_count <= 6 and totals[5] == scans[0].table_count
    tables = eu._aligned(int(totals[5]) * eu.HUFF_BYTES)
    packed = eu._aligned(int(totals[4]), fill=0x5A)
    guard = packed.copy()
    args = (ptrs, lens, 1, 16, descs, scans, tables.ctypes.data)
    assert prep(*args, totals[5], packed.ctypes.data, totals[4] - 1, totals) == -2                    # POEM_E_WORKSPACE ...
    assert prep(*args, totals[5] - 1, packed.ctypes.data, totals[4], totals) == -2
    assert np.array_equal(packed, guard)                                                              # ... and nothing written
    assert prep(*args, totals[5], packed.ctypes.data + 4, totals[4], totals) == -1                    # misaligned
    assert prep(ptrs, lens, 1, 16, descs, scans, None, totals[5], packed.ctypes.data, totals[4], totals) == -1
    assert prep(*args, totals[5], packed.ctypes.data, totals[4], totals) == 0
    assert bytes(packed[:seg]) == data[eu.scan_start(data):] and not packed[seg:].any()
    # the host driver
    par = L.poem_jpeg_entropy_parallel_host
    d4, t4, rounds = (pk.jpeg.JpegDesc * 1)(), (ctypes.c_int64 * 4)(), (ctypes.c_int32 * 1)()
    assert par(None, lens, 1, 16, d4, None, 0, t4, rounds) == -1
    assert par(ptrs, lens, 0, 16, d4, None, 0, t4, rounds) == -1
    assert par(ptrs, lens, 1, 48, d4, None, 0, t4, rounds) == -1
    assert par(ptrs, lens, 65536, 16, d4, None, 0, t4, rounds) == -4
    assert par(ptrs, lens, 1, 16, d4, None, 0, t4, None) == 0 and list(t4) == rt
    coef = eu._aligned(rt[0], np.int16, fill=0x33)
    keep = coef.copy()
    assert par(ptrs, lens, 1, 16, d4, coef.ctypes.data, rt[0] - 2, t4, rounds) == -2 and np.array_equal(coef, keep)
    assert par(ptrs, lens, 1, 16, d4, coef.ctypes.data + 2, rt[0], t4, rounds) == -1
    # the device call: everything is checked before anything is launched (no GPU here)
    dev = L.poem_jpeg_entropy_device
    assert L.poem_jpeg_entropy_workspace_bytes(0, 10) == 0 and L.poem_jpeg_entropy_workspace_bytes(1, -1) == 0
    need = L.poem_jpeg_entropy_workspace_bytes(3, 100)
    assert need >= 16 + 100 * 62 and need % 16 == 0 and L.poem_jpeg_entropy_workspace_bytes(3, 101) > need
    assert dev(None, None, None, 0, None, 0, 1, 0, 0, 0, 0, None, 0, None, None, 0, None) == -1
    fake = 1 << 20                                                                                   # aligned, never dereferenced
    ok = [fake, fake, fake, 1, fake, 16, 1, 16, 256, 1, 1, fake, 128, fake, fake, need, None]

    def call(**kw):
        names = ["descs", "scans", "tables", "table_count", "packed", "packed_bytes", "n", "subseq", "wg", "subs", "blocks", "coef",
                 "coef_bytes", "status", "ws", "ws_bytes", "stream"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return dev(*a)
    assert call(n=0) == -1 and call(n=65536) == -4 and call(packed_bytes=-1) == -1 and call(coef_bytes=-1) == -1 and call(subs=-1) == -1
    assert call(subseq=24) == -1 and call(subseq=2048) == -1 and call(wg=96) == -1 and call(wg=2048) == -1 and call(wg=32) == -1
    assert call(coef=fake + 2) == -1 and call(packed=fake + 8) == -1 and call(ws=fake + 4) == -1 and call(status=fake + 1) == -1
    assert call(ws=None) == -2 and call(ws_bytes=need - 1, subs=100, n=3) == -2
