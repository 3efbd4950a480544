"""Shared by test_jpeg_entropy_host.py / test_jpeg_entropy_device.py: the streams the parallel entropy decoder is held to (made with
PIL at test time through jpeg_util), the seeded damage sweep, and ctypes helpers around ``poem_jpeg_entropy_parallel_host`` /
``poem_jpeg_entropy_prepare`` / ``poem_jpeg_entropy_device``.  The yardstick is always the serial decoder
(``jpeg_util.entropy_decode`` = ``poem_jpeg_entropy_decode``): same verdict, same coefficient bytes where taken."""
import ctypes
import functools
import io

import numpy as np

import jpeg_util as ju


class JpegScan(ctypes.Structure):
    """include/poem_hip.h poem_jpeg_scan_t"""
    _fields_ = [("byte_offset", ctypes.c_int64), ("byte_count", ctypes.c_int64), ("sub_base", ctypes.c_int64),
                ("sub_count", ctypes.c_int32), ("restart", ctypes.c_int32), ("table_base", ctypes.c_int32),
                ("table_count", ctypes.c_int32), ("dc_sel", ctypes.c_uint8 * 3), ("ac_sel", ctypes.c_uint8 * 3),
                ("reserved", ctypes.c_uint8 * 2)]


HUFF_BYTES = 1424
assert ctypes.sizeof(JpegScan) == 48


def _aligned(nbytes, dtype=np.uint8, fill=0):
    raw = np.full(nbytes + 16, fill, np.uint8)
    off = -raw.ctypes.data % 16
    return raw[off:off + nbytes].view(dtype)


def _pointers(streams):
    n = len(streams)
    bufs = [np.frombuffer(s, np.uint8) for s in streams]
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_int64 * n)(*[len(s) for s in streams])
    return bufs, ptrs, lens


def parallel_host(streams, subseq):
    """-> (descs, coef int16 ndarray, totals, rounds list) through the size query and one call of the host driver."""
    from poem_v2_amd import hip, jpeg
    L = hip.lib()
    n = len(streams)
    bufs, ptrs, lens = _pointers(streams)
    descs = (jpeg.JpegDesc * n)()
    totals = (ctypes.c_int64 * 4)()
    rounds = (ctypes.c_int32 * n)()
    assert L.poem_jpeg_entropy_parallel_host(ptrs, lens, n, subseq, descs, None, 0, totals, rounds) == 0
    coef = _aligned(max(int(totals[0]), 16), np.int16)
    assert L.poem_jpeg_entropy_parallel_host(ptrs, lens, n, subseq, descs, coef.ctypes.data, coef.nbytes, totals, rounds) == 0
    return descs, coef, [int(t) for t in totals], list(rounds)


def sub_counts(streams, subseq):
    """Subsequences of every stream (0 where the headers refuse it), from the prepare call's size query."""
    from poem_v2_amd import hip, jpeg
    n = len(streams)
    bufs, ptrs, lens = _pointers(streams)
    descs, scans, totals = (jpeg.JpegDesc * n)(), (JpegScan * n)(), (ctypes.c_int64 * 8)()
    assert hip.lib().poem_jpeg_entropy_prepare(ptrs, lens, n, subseq, descs, scans, None, 0, None, 0, totals) == 0
    return [s.sub_count for s in scans]


def taken_ranges(descs):
    return [(d.coef_offset // 2, (d.coef_offset + d.coef_bytes) // 2) for d in descs]


def same_result(descs, coef, ref_descs, ref_coef, names=None):
    """Names (or indices) of the images whose verdict, header-stage code or coefficients differ from the reference's."""
    bad = []
    for i, (d, r) in enumerate(zip(descs, ref_descs)):
        name = names[i] if names else i
        if (d.status == 0) != (r.status == 0) or (r.status == 1 and d.status != 1):
            bad.append((name, d.status, r.status))
        elif r.status == 0:
            a, b = r.coef_offset // 2, (r.coef_offset + r.coef_bytes) // 2
            if d.coef_offset != r.coef_offset or d.coef_bytes != r.coef_bytes or not np.array_equal(coef[a:b], ref_coef[a:b]):
                bad.append((name, "coefficients"))
    return bad


# ---- streams -------------------------------------------------------------------------------------------------------------------
def _find(data, marker):
    pos = 2
    while data[pos + 1] != marker:
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    return pos


def scan_start(data):
    sos = _find(data, 0xDA)
    return sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")


def _patch_dqt(data, value):
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


@functools.lru_cache(maxsize=None)
def refusal_cases():
    """The ten named refusal streams of test_jpeg_host.py, rebuilt."""
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
    bad[dht + 5:dht + 21] = bytes([255]) * 16
    cases["corrupt_huffman"] = bytes(bad)
    sof = _find(base, 0xC0)
    bad = bytearray(base)
    bad[sof + 14] = 0x21
    cases["chroma_2x1"] = bytes(bad)
    bad = bytearray(base)
    for k, ch in enumerate(b"RGB"):
        bad[sof + 10 + 3 * k] = ch
        bad[sos + 5 + 2 * k] = ch
    cases["rgb_ids"] = bytes(bad)
    app0 = _find(base, 0xE0)
    cases["rgb_ids_no_jfif"] = bytes(bad[:app0]) + bytes(bad[app0 + 2 + int.from_bytes(base[app0 + 2:app0 + 4], "big"):])
    assert len(cases) == 10
    return cases


@functools.lru_cache(maxsize=None)
def good_streams():
    """Grid (384) + narrow (162) + saturated noise at two samplings.  -> [(id, bytes)]"""
    out = list(ju.grid()) + list(ju.narrow())
    for s in ("444", "420"):
        out.append((f"saturated-{s}", ju.encode(ju.saturated_noise(), s, quality=100)))
    return out


@functools.lru_cache(maxsize=None)
def targeted_streams():
    """What the grid does not guarantee.  -> [(id, bytes)]"""
    out = []
    flat = np.full((48, 64, 3), 90, np.uint8)
    for s in ("444", "420"):                                         # DC + EOB blocks: many blocks per subsequence
        out.append((f"flat-{s}-q30", ju.encode(flat, s, quality=30)))
        out.append((f"flat-{s}-q30opt", ju.encode(flat, s, quality=30, optimize=True)))
    out.append(("flat-grey-opt", ju.encode(flat[..., 0].copy(), quality=30, optimize=True)))     # 1-bit codes: MCUs inside one byte
    out.append(("ramp-a0-q30", ju.encode(ju.make_image(40, 56, 0), "420", quality=30)))
    y, x = np.mgrid[0:32, 0:48]
    checker = (((x + y) & 1) * 255).astype(np.uint8)                 # highest frequency only: long zero runs, ZRL symbols
    out.append(("checker-444-q100", ju.encode(np.repeat(checker[..., None], 3, -1), "444", quality=100)))
    out.append(("checker-grey-q100", ju.encode(checker, quality=100)))
    cols = ((x & 1) * 255).astype(np.uint8)
    out.append(("columns-grey-q100", ju.encode(cols, quality=100)))
    wave = np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)   # the (7, 7) basis function alone:
    hf = np.clip(128 + 100 * wave + 20 * ((x // 8 + y // 8) % 3), 0, 255).astype(np.uint8)         # 62 zeros, then the last coefficient
    out.append(("hf77-grey-q90", ju.encode(hf, quality=90)))
    out.append(("hf77-444-q90", ju.encode(np.repeat(hf[..., None], 3, -1), "444", quality=90)))
    noise = ju.make_image(40, 72, 120)
    out.append(("rst-long-420", ju.encode(noise, "420", quality=95, restart_marker_blocks=4)))   # an interval over several subsequences
    out.append(("rst-long-444", ju.encode(noise, "444", quality=100, restart_marker_blocks=9)))
    out.append(("rst-rows-444", ju.encode(noise, "444", quality=95, restart_marker_rows=1)))
    out.append(("rst-short-flat", ju.encode(flat, "444", quality=30, restart_marker_blocks=1)))  # several intervals in one subsequence
    out.append(("rst-short-grey", ju.encode(ju.make_image(24, 40, 0, grey=True), quality=30, restart_marker_blocks=1)))
    out.append(("rst-2-grey", ju.encode(ju.make_image(40, 72, 120, grey=True), quality=90, restart_marker_blocks=2)))   # RST7 -> RST0
    for amp in (0, 25, 120):
        out.append((f"grey-a{amp}", ju.encode(ju.make_image(33, 50, amp, grey=True), quality=85)))
    return out


@functools.lru_cache(maxsize=None)
def large_stream():
    """96 x 128 noise at q95, 4:4:4: about 10 KB of scan, over 600 subsequences of 16 bytes."""
    return ju.encode(ju.make_image(96, 128, 120), "444", quality=95)


@functools.lru_cache(maxsize=None)
def damage_bases():
    rgb = ju.make_image(40, 24, 120)
    return [("420-q75", ju.encode(rgb, "420", quality=75)), ("444-q90opt", ju.encode(rgb, "444", quality=90, optimize=True)),
            ("422-q95rst", ju.encode(rgb, "422", quality=95, restart_marker_blocks=1))]


@functools.lru_cache(maxsize=None)
def damage_sweep(per_base=120, seed=11):
    """Single-byte edits and truncations inside the scan of the three damage bases.  -> [(id, bytes)]"""
    rng = np.random.default_rng(seed)
    out = []
    for name, data in damage_bases():
        lo = scan_start(data)
        for k in range(per_base):
            at = int(rng.integers(lo, len(data)))
            kind = k % 5
            mut = bytearray(data)
            if kind == 0:
                mut[at] = int(rng.integers(0, 256))
            elif kind == 1:
                mut[at] ^= 1 << int(rng.integers(0, 8))
            elif kind == 2:
                mut[at] = 0xFF
            elif kind == 3:
                mut[at] = 0xD0 + int(rng.integers(0, 10))             # a restart marker's (or EOI's) second byte
            else:
                mut = mut[:at]                                        # truncation
            out.append((f"{name}-{k}-{('set', 'flip', 'ff', 'dx', 'cut')[kind]}@{at}", bytes(mut)))
    return out


# ---- the device ------------------------------------------------------------------------------------------------------------------
def device_decode(streams, subseq=0, wg_threads=0, guard=4096):
    """prepare -> upload -> poem_jpeg_entropy_device -> download.  Coefficients, statuses and workspace sit between guard bytes of
    0xA5 that are checked here.  -> (descs as downloaded, coef int16 ndarray, statuses list, rounds list, totals list)"""
    import torch
    from poem_v2_amd import hip, jpeg
    L = hip.lib()
    n = len(streams)
    bufs, ptrs, lens = _pointers(streams)
    descs, scans, totals = (jpeg.JpegDesc * n)(), (JpegScan * n)(), (ctypes.c_int64 * 8)()
    assert L.poem_jpeg_entropy_prepare(ptrs, lens, n, subseq, descs, scans, None, 0, None, 0, totals) == 0
    tables = _aligned(max(int(totals[5]), 1) * HUFF_BYTES)
    packed = _aligned(max(int(totals[4]), 16))
    assert L.poem_jpeg_entropy_prepare(ptrs, lens, n, subseq, descs, scans, tables.ctypes.data, int(totals[5]), packed.ctypes.data,
                                       packed.nbytes, totals) == 0
    dev = torch.device("cuda:0")

    def up(arr):
        return torch.from_numpy(np.frombuffer(bytes(arr), np.uint8).copy()).to(dev)

    d_descs, d_scans, d_tables, d_packed = up(descs), up(scans), up(tables), up(packed)
    coef_bytes = max(int(totals[0]), 16)
    ws_bytes = L.poem_jpeg_entropy_workspace_bytes(n, int(totals[6]))
    st_bytes = (4 * n + 15) & ~15
    d_coef = torch.full((coef_bytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    d_ws = torch.full((ws_bytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    d_status = torch.full((st_bytes + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    rc = L.poem_jpeg_entropy_device(d_descs.data_ptr(), d_scans.data_ptr(), d_tables.data_ptr(), int(totals[5]), d_packed.data_ptr(),
                                    int(totals[4]), n, subseq, wg_threads, int(totals[6]), int(totals[1]), d_coef.data_ptr() + guard,
                                    int(totals[0]), d_status.data_ptr() + guard, d_ws.data_ptr() + guard, ws_bytes, hip.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    coef_h, ws_h, st_h = d_coef.cpu().numpy(), d_ws.cpu().numpy(), d_status.cpu().numpy()
    for name, arr, used in (("coefficients", coef_h, int(totals[0])), ("workspace", ws_h, ws_bytes), ("status", st_h, 4 * n)):
        assert (arr[:guard] == 0xA5).all() and (arr[guard + used:guard + used + guard // 2] == 0xA5).all(), f"guard bytes around the {name}"
    out_descs = (jpeg.JpegDesc * n).from_buffer_copy(d_descs.cpu().numpy().tobytes())
    coef = coef_h[guard:guard + coef_bytes].copy().view(np.int16)
    status = st_h[guard:guard + 4 * n].copy().view(np.int32).tolist()
    rounds = ws_h[guard:guard + 4 * n].copy().view(np.int32).tolist()
    return out_descs, coef, status, rounds, [int(t) for t in totals]
