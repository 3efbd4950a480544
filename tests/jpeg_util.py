"""Shared by test_jpeg_host.py / test_jpeg_device.py: seeded JPEG cases made with PIL at test time, the yardstick
(``np.asarray(Image.open(...).convert("RGB"))`` on the same bytes), a numpy restatement of the reconstruction arithmetic the
device route is held to (csrc/jpeg.h: inverse DCT, fancy up-sampling, YCbCr -> RGB) with its own small Huffman reader --
independent of the C++ -- and ctypes helpers around ``poem_jpeg_entropy_decode`` / ``poem_jpeg_reconstruct[_host]``."""
import ctypes
import functools
import io

import numpy as np

SIZES = [(8, 8), (16, 16), (29, 37), (17, 9), (40, 24), (33, 50), (1, 1), (7, 70)]          # (H, W)
AMPS = [0, 25, 120]
SAMPLINGS = {"444": 0, "422": 1, "420": 2}
QUALITIES = [("q30", dict(quality=30)), ("q75", dict(quality=75)), ("q90opt", dict(quality=90, optimize=True)),
             ("q95rst", dict(quality=95, restart_marker_blocks=1)), ("q100", dict(quality=100))]


def make_image(h, w, amp, seed=0, grey=False):
    """Coordinate ramps plus uniform noise of amplitude ``amp`` -> uint8 (h, w, 3) or (h, w)."""
    rng = np.random.default_rng(seed * 7919 + h * 131 + w * 17 + amp)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], -1)
    img = np.clip(base + rng.integers(-amp, amp + 1, size=(h, w, 3)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[..., 0]) if grey else img


NARROW = [(16, 4), (16, 3), (9, 4), (2, 4), (16, 2), (16, 1), (3, 2), (16, 5), (5, 6)]      # (H, W): chroma width <= 2, and just above


@functools.lru_cache(maxsize=None)
def narrow():
    """Images at most 4 wide (libjpeg replicates their chroma instead of interpolating it) and the first widths above, at every
    sampling.  -> [(id, bytes)]"""
    out = []
    for h, w in NARROW:
        for amp in (25, 120):
            for s in SAMPLINGS:
                for qn, kw in (QUALITIES[0], QUALITIES[2], QUALITIES[4]):
                    out.append((f"{h}x{w}-a{amp}-{s}-{qn}", encode(make_image(h, w, amp), s, **kw)))
    return out


def saturated_noise(h=32, w=48, seed=3):
    return (np.random.default_rng(seed).integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)


def encode(arr, sampling="420", **kw):
    from PIL import Image
    buf = io.BytesIO()
    if arr.ndim == 2:
        Image.fromarray(arr, "L").save(buf, format="JPEG", **kw)
    else:
        Image.fromarray(arr, "RGB").save(buf, format="JPEG", subsampling=SAMPLINGS[sampling], **kw)
    return buf.getvalue()


def pil_decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def grid():
    """The 384 cases: 8 sizes x 3 noise amplitudes x (3 samplings x 5 quality settings + greyscale).  -> [(id, bytes)]"""
    out = []
    for h, w in SIZES:
        for amp in AMPS:
            rgb = make_image(h, w, amp)
            for s in SAMPLINGS:
                for qn, kw in QUALITIES:
                    out.append((f"{h}x{w}-a{amp}-{s}-{qn}", encode(rgb, s, **kw)))
            out.append((f"{h}x{w}-a{amp}-grey", encode(make_image(h, w, amp, grey=True), quality=75)))
    assert len(out) == 384
    return out


@functools.lru_cache(maxsize=None)
def grid_reference():
    """PIL's decode of every grid case, computed once."""
    return [pil_decode(data) for _, data in grid()]


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63]


class Refused(Exception):
    pass


class _Bits:
    def __init__(self, data):
        self.v, self.n = int.from_bytes(data, "big"), 8 * len(data)

    def get(self, k):
        if k > self.n:
            raise Refused("entropy data ends early")
        self.n -= k
        return (self.v >> self.n) & ((1 << k) - 1)


def _huff_table(counts, syms):
    table, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            table[(ln, code)] = syms[k]
            code, k = code + 1, k + 1
        code <<= 1
    return table


def _sym(bits, table):
    code = 0
    for ln in range(1, 17):
        code = (code << 1) | bits.get(1)
        if (ln, code) in table:
            return table[(ln, code)]
    raise Refused("no such code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def parse(data):
    """Baseline stream -> dict(height, width, ncomp, hs, vs, quant [per component (64,) natural order], coef [per component
    (blocks_h, blocks_w, 64) int16 natural order]); ``Refused`` for anything else (only what the tests feed is told apart)."""
    if data[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    pos, qt, ht, frame, ri = 2, {}, {}, None, 0
    while True:
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise Refused("bad marker")
        m, ln = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos + 4:pos + 2 + ln]
        pos += 2 + ln
        if m in (0xC0, 0xC1):
            if seg[0] != 8:
                raise Refused("precision")
            frame = dict(height=int.from_bytes(seg[1:3], "big"), width=int.from_bytes(seg[3:5], "big"),
                         comps=[(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])])
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise Refused("frame type")
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                counts = list(seg[p + 1:p + 17])
                n = sum(counts)
                ht[seg[p]] = _huff_table(counts, list(seg[p + 17:p + 17 + n]))
                p += 17 + n
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    raise Refused("16-bit quantisation table")
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = list(seg[p + 1:p + 65])
                qt[seg[p] & 15] = q
                p += 65
        elif m == 0xDD:
            ri = int.from_bytes(seg[:2], "big")
        elif m == 0xDA:
            break
    comps = frame["comps"]
    if len(comps) not in (1, 3) or seg[0] != len(comps):
        raise Refused("components")
    hs, vs = (comps[0][1], comps[0][2]) if len(comps) == 3 else (1, 1)
    if len(comps) == 3 and ((hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in comps[1:])):
        raise Refused("sampling")
    H, W = frame["height"], frame["width"]
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    tabs = [(ht[seg[2 + 2 * c] >> 4], ht[0x10 | (seg[2 + 2 * c] & 15)]) for c in range(len(comps))]
    coef = [np.zeros((my * (vs if c == 0 else 1), mx * (hs if c == 0 else 1), 64), np.int16) for c in range(len(comps))]
    # the entropy-coded segment: unstuff, split at RSTn
    chunks, cur = [], bytearray()
    while True:
        if pos >= len(data):
            raise Refused("no EOI")
        b = data[pos]
        if b != 0xFF:
            cur.append(b)
            pos += 1
        elif pos + 1 < len(data) and data[pos + 1] == 0:
            cur.append(0xFF)
            pos += 2
        elif pos + 1 < len(data) and 0xD0 <= data[pos + 1] <= 0xD7:
            chunks.append(bytes(cur))
            cur = bytearray()
            pos += 2
        else:
            chunks.append(bytes(cur))
            if not (pos + 1 < len(data) and data[pos + 1] == 0xD9):
                raise Refused("scan does not end in EOI")
            break
    mcus = [(y, x) for y in range(my) for x in range(mx)]
    per = ri if ri else len(mcus)
    if len(chunks) != -(-len(mcus) // per):
        raise Refused("restart intervals")
    for ci, chunk in enumerate(chunks):
        bits, pred = _Bits(chunk), [0] * len(comps)
        for y, x in mcus[ci * per:(ci + 1) * per]:
            for c in range(len(comps)):
                nh, nv = (hs, vs) if c == 0 else (1, 1)
                for v in range(nv):
                    for h in range(nh):
                        blk = coef[c][y * nv + v, x * nh + h]
                        s = _sym(bits, tabs[c][0])
                        pred[c] += _extend(bits.get(s), s) if s else 0
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = _sym(bits, tabs[c][1])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise Refused("block overrun")
                            blk[ZIGZAG[k]] = _extend(bits.get(s), s)
                            k += 1
    return dict(height=H, width=W, ncomp=len(comps), hs=hs, vs=vs, quant=[qt[c[3]] for c in comps], coef=coef)


def _pass(x, s):
    """x (..., 8) int64 -> (..., 8): one 1-D pass of csrc/jpeg.h, descaled by s."""
    a, b, c, d, e, f, g, h, i, j, k, l = 2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172
    x0, x1, x2, x3, x4, x5, x6, x7 = [x[..., n] for n in range(8)]
    z1 = (x2 + x6) * c
    t2, t3 = z1 - x6 * h, z1 + x2 * d
    t0, t1 = (x0 + x4) << 13, (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = x7, x5, x3, x1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * f
    t0, t1, t2, t3 = t0 * a, t1 * j, t2 * l, t3 * g
    z1, z2, z3, z4 = z1 * -e, z2 * -k, z3 * -i + z5, z4 * -b + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], -1)
    return (out + (1 << (s - 1))) >> s


def _plane(coef, quant):
    bh, bw, _ = coef.shape
    d = (coef.astype(np.int64) * quant).reshape(bh, bw, 8, 8)
    ws = _pass(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)         # columns first
    px = np.clip(_pass(ws, 18) + 128, 0, 255)                   # then rows
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _up_h(c, odd_add, even_add, shift, edge):
    """c (h, w) -> (h, 2w): out[2j] = (3 c[j] + c[j-1] + even_add) >> shift, out[2j+1] = (3 c[j] + c[j+1] + odd_add) >> shift,
    the first and last through ``edge``."""
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 2::2] = (3 * c[:, 1:] + c[:, :-1] + even_add) >> shift
    out[:, 1:-1:2] = (3 * c[:, :-1] + c[:, 1:] + odd_add) >> shift
    out[:, 0], out[:, -1] = edge(c[:, 0], even_add), edge(c[:, -1], odd_add)
    return out


def reconstruct(p):
    H, W = p["height"], p["width"]
    planes = [_plane(c, q) for c, q in zip(p["coef"], p["quant"])]
    Y = planes[0][:H, :W]
    if p["ncomp"] == 1:
        return np.repeat(Y[..., None], 3, -1).astype(np.uint8)
    ch, cw = -(-H // p["vs"]), -(-W // p["hs"])
    chroma = []
    for pl in planes[1:]:
        c = pl[:ch, :cw]
        if p["hs"] == 2 and cw <= 2:                   # libjpeg: a component at most 2 samples wide is replicated, not interpolated
            c = np.repeat(np.repeat(c, 2, 1), p["vs"], 0)
        elif p["hs"] == 2 and p["vs"] == 1:
            c = _up_h(c, 2, 1, 2, lambda v, add: v)
        elif p["hs"] == 2:
            idx = np.arange(ch)
            rows = np.empty((2 * ch, cw), np.int64)
            rows[0::2] = 3 * c + c[np.maximum(idx - 1, 0)]
            rows[1::2] = 3 * c + c[np.minimum(idx + 1, ch - 1)]
            c = _up_h(rows, 7, 8, 4, lambda v, add: (4 * v + add) >> 4)
        chroma.append(c[:H, :W] - 128)
    cb, cr = chroma
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    return reconstruct(parse(data))


def block_l1(p):
    """Largest per-block sum of |coef * quant| of a parsed stream (the quantity the range guard bounds)."""
    return max(int(np.abs(c.astype(np.int64) * q).sum(-1).max()) for c, q in zip(p["coef"], p["quant"]))


# ---- the library ------------------------------------------------------------------------------------------------------------
def entropy_decode(streams, threads=0):
    """-> (descs ctypes array, coef int16 ndarray, totals list) through the size query and one decode call."""
    from poem_v2_amd import hip, jpeg
    L = hip.lib()
    n = len(streams)
    bufs = [np.frombuffer(s, np.uint8) for s in streams]
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_int64 * n)(*[len(s) for s in streams])
    descs = (jpeg.JpegDesc * n)()
    totals = (ctypes.c_int64 * 4)()
    assert L.poem_jpeg_entropy_decode(ptrs, lens, n, descs, None, 0, totals, threads) == 0
    coef = np.zeros(max(int(totals[0]) // 2, 8) + 8, np.int16)
    off = (-coef.ctypes.data % 16) // 2                              # the library wants the buffer on 16 bytes
    coef = coef[off:off + max(int(totals[0]) // 2, 8)]
    assert L.poem_jpeg_entropy_decode(ptrs, lens, n, descs, coef.ctypes.data, coef.nbytes, totals, threads) == 0
    return descs, coef, [int(t) for t in totals]


def desc_coef(desc, coef, c):
    """Component c's coefficients of one image -> (blocks_h, blocks_w, 64) view."""
    start = desc.coef_offset // 2 + 64 * sum(desc.blocks_w[k] * desc.blocks_h[k] for k in range(c))
    return coef[start:start + 64 * desc.blocks_w[c] * desc.blocks_h[c]].reshape(desc.blocks_h[c], desc.blocks_w[c], 64)


def reconstruct_host(descs, coef, totals):
    """-> list of (H, W, 3) arrays, None for a refused image."""
    from poem_v2_amd import hip
    n = len(descs)
    sizes = [d.height * d.width * 3 if d.status == 0 else 0 for d in descs]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = np.full(max(int(offs[-1]), 1), 0xA5, np.uint8)
    rc = hip.lib().poem_jpeg_reconstruct_host(descs, coef.ctypes.data, coef.nbytes, offs.ctypes.data, out.ctypes.data, out.nbytes, n)
    assert rc == 0, rc
    return [out[offs[i]:offs[i + 1]].reshape(d.height, d.width, 3) if d.status == 0 else None for i, d in enumerate(descs)]
