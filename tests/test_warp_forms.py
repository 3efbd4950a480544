"""csrc/warp.hip -- ``warp_affine_kernel`` alone, in every form: through ``poem_warp_affine`` (ctypes) with ``m_inv`` GIVEN, so that
a test decides every coordinate, and through ``transform.warp_views``.  Everything is compared bit for bit with
``transform_oracle`` (``fixed_point_coords`` / ``warp_affine_u8`` / ``color_jitter_u8`` / ``to_tensor_normalize``); the oracle
inverts the matrix it is handed, so ``given_m_inv`` here switches that one step off for the duration of a call -- the oracle's
arithmetic is untouched.

Every output lies between guards (bytes 0xA5 / the float canary) that are checked after each launch; refused calls leave the
outputs untouched.  Sources are packed back to back with no padding, so images start at odd byte offsets.

The common range: the kernel converts double -> int with saturation at 2^31 where the oracle carries int64.  Every map here keeps
|source coordinate| * 1024 below 2^30, where the two agree (asserted on the CPU for the saturation case, the only one near it).
NaN gains are excluded: the C cast of a NaN is undefined."""
import contextlib

import numpy as np
import pytest
import torch

import transform_oracle as to

DEV = "cuda:0"
_CANARY = 0x7FC0DEAD
_BYTE = 0xA5
_GUARD = 256
OWS = (1, 3, 4, 5, 8, 255, 256, 257, 259, 260)
OHS = (1, 3, 4, 5, 9)
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3)]          # (h, w): 3 * w % 4 != 0 for w = 1, 2, 3, 5, 7


# ---- the oracle with m_inv given ---------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def given_m_inv():
    real = to.invert_2x3
    to.invert_2x3 = lambda M: np.array(M, dtype=np.float64).reshape(-1).copy()
    try:
        yield
    finally:
        to.invert_2x3 = real


def coords(m, W, H, rnd=np.rint, sat=True):
    """The oracle's fixed_point_coords with the two steps under test exchangeable (asserted equal to it in a CPU test)."""
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    ad, bd = rnd(m[0] * x * 1024.0).astype(np.int64), rnd(m[3] * x * 1024.0).astype(np.int64)
    X0 = rnd((m[1] * y + m[2]) * 1024.0).astype(np.int64) + 16
    Y0 = rnd((m[4] * y + m[5]) * 1024.0).astype(np.int64) + 16
    X, Y = (X0[:, None] + ad[None, :]) >> 5, (Y0[:, None] + bd[None, :]) >> 5
    sx, sy = X >> 5, Y >> 5
    if sat:
        sx, sy = np.clip(sx, -32768, 32767), np.clip(sy, -32768, 32767)
    return sx, sy, X & 31, Y & 31


def half_away(v):
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def ref_u8(img, m, OW, OH, gain=None, **kw):
    """The oracle's warp at given coordinates (its own when kw is empty), then its colour jitter."""
    real = to.fixed_point_coords
    if kw:
        to.fixed_point_coords = lambda M, W, H: coords(M, W, H, **kw)
    try:
        with given_m_inv():
            out = to.warp_affine_u8(img, m, (OW, OH))
    finally:
        to.fixed_point_coords = real
    return out if gain is None else to.color_jitter_u8(out, gain)


def in_range(m, OW, OH):
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    c = [abs(m[0]) * (OW - 1) + abs(m[1]) * (OH - 1) + abs(m[2]), abs(m[3]) * (OW - 1) + abs(m[4]) * (OH - 1) + abs(m[5])]
    return max(c) * 1024.0 < 2.0 ** 30


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def tiny_views(views, OW, OH, seed, first=0):
    """views tiny sources (SIZES in turn) with maps that start at the source's first row and column or just outside them (so that an
    output of a single row or column still meets the source) and spread the output to about size + 2, with a little shear;
    the LAST view's map lands wholly outside its source when there is more than one view."""
    g = np.random.default_rng(seed)
    imgs, ms = [], []
    for v in range(views):
        h, w = SIZES[(first + v) % len(SIZES)]
        imgs.append(g.integers(1, 256, size=(h, w, 3), dtype=np.uint8))
        ms.append([(w + 3) / OW * g.uniform(0.8, 1.2), g.uniform(-0.05, 0.05), g.uniform(-0.9, 0.2),
                   g.uniform(-0.002, 0.002), (h + 3) / OH * g.uniform(0.8, 1.2), g.uniform(-0.9, 0.2)])
    if views > 1:
        ms[-1][2] = 1000.25
    return imgs, np.asarray(ms)


GAINS = np.array([[0.0, 300.0, -2.0], [0.5, np.nextafter(0.5, 0.0), 2.0], [1.0, np.nextafter(1.0, 0.0), 1.0 / 3.0],
                  [1.2999, 0.7137, 1.5]])


def border_case():
    """16 x 16 source, 18 x 18 output, the identity moved by half a pixel: column 0 has sx = -1, column 16.. sx = 15 = sw - 1, rows
    likewise, all with the fraction 16/32 -- the four partial-tap patterns on whole rows and columns."""
    g = np.random.default_rng(3)
    return g.integers(1, 256, size=(16, 16, 3), dtype=np.uint8), np.array([1.0, 0.0, -0.5, 0.0, 1.0, -0.5]), 18, 18


def tie_case():
    """m0 = 1 + 2^-11: m0 x 1024 = 1024 x + x / 2 is a tie for every odd x; m3 = 2^-11 gives the y coordinate the same ties.  Half
    of them round differently under round-half-away, by one unit of 2^-10 pixel; the unit survives the >> 5 only where the low five
    bits of X0 + adelta are all ones.  m1 = 33/1024 walks X0's low bits through the rows and m2 = 3 + 31/1024 starts them at 31, so
    that some pixels of every row carry the tie into the 1/32-pixel fraction."""
    g = np.random.default_rng(4)
    img = g.integers(0, 256, size=(48, 300, 3), dtype=np.uint8)
    m = np.array([1.0 + 2.0 ** -11, 33.0 / 1024.0, 3.0 + 31.0 / 1024.0, 2.0 ** -11, 1.0, 2.0 + 15.0 / 1024.0])
    return img, m, 256, 40


def saturation_case():
    """Three views.  0: a 2 x 2 source and coordinates 65536 + (0..3): a short that wrapped would read INSIDE the source, the
    saturated one reads the border.  1: a 1 x 40000 source addressed at x = 39000..: saturation reads pixel 32767.  2: a 40000 x 1
    source, the same for y.  |coordinate| * 1024 < 2^30 (asserted)."""
    g = np.random.default_rng(6)
    imgs = [g.integers(1, 256, size=(2, 2, 3), dtype=np.uint8), g.integers(1, 256, size=(1, 40000, 3), dtype=np.uint8),
            g.integers(1, 256, size=(40000, 1, 3), dtype=np.uint8)]
    ms = np.array([[0.25, 0.0, 65536.0, 0.0, 0.25, -65536.0 * 0 + 65536.0],
                   [1.0, 0.0, 39000.25, 0.0, 0.125, -0.25],
                   [0.125, 0.0, -0.25, 1.0, 0.0, 39000.25]])
    return imgs, ms, 8, 4


# ---- CPU: every condition on the inputs ------------------------------------------------------------------------------------------------
def test_own_coordinates_are_the_oracles():
    for OW, OH in ((260, 9), (5, 3)):
        imgs, ms = tiny_views(6, OW, OH, seed=1)
        for m in ms:
            with given_m_inv():
                want = to.fixed_point_coords(m, OW, OH)
            assert all(np.array_equal(a, b) for a, b in zip(coords(m, OW, OH), want))
            assert in_range(m, OW, OH)
    M = np.array([[1.3, -0.2, 4.0], [0.1, 0.9, -3.0]])
    with given_m_inv():                                     # the switch is off again afterwards
        pass
    assert not np.array_equal(to.invert_2x3(M), M.reshape(-1))


def test_shapes_reach_the_blocks_they_are_meant_for():
    """A thread does 4 pixels, a block 256 x 4: the widths hold a scalar tail (n < 4) in a first and in a second x-block, a second
    x-block with one live thread, full blocks; the heights are off the block's four rows."""
    tail = {ow: ow % 4 for ow in OWS}
    assert {tail[1], tail[3], tail[5], tail[255]} == {1, 3} and {tail[257], tail[259]} == {1, 3}          # tails in block 0 and 1
    assert (257 + 3) // 4 - 64 == 1 and (260 + 3) // 4 - 64 == 1 and 260 % 4 == 0                            # one live thread
    assert any(oh % 4 for oh in OHS) and 4 in OHS and 9 in OHS
    assert sum(1 for h, w in SIZES if (3 * w) % 4) == len(SIZES)
    offs = np.cumsum([0] + [h * w * 3 for h, w in SIZES])
    assert any(o % 2 for o in offs[:-1]) and any(o % 4 == 2 for o in offs)


def test_border_case_holds_every_partial_tap_pattern():
    img, m, OW, OH = border_case()
    sx, sy, ax, ay = coords(m, OW, OH)
    sh, sw = img.shape[:2]
    inside_y, inside_x = (sy >= 0) & (sy < sh - 1), (sx >= 0) & (sx < sw - 1)
    for name, mask in (("sx = -1", (sx == -1) & (ax != 0) & inside_y), ("sx = sw - 1", (sx == sw - 1) & (ax != 0) & inside_y),
                       ("sy = -1", (sy == -1) & (ay != 0) & inside_x), ("sy = sh - 1", (sy == sh - 1) & (ay != 0) & inside_x)):
        assert int(mask.sum()) >= 14, (name, int(mask.sum()))
    for name, mask in (("sx = -1", (sx == -1) & (ax != 0)), ("sx = sw - 1", (sx == sw - 1) & (ax != 0)),
                       ("sy = -1", (sy == -1) & (ay != 0)), ("sy = sh - 1", (sy == sh - 1) & (ay != 0))):
        assert int(mask.sum()) >= 16, (name, int(mask.sum()))
    out = ref_u8(img, m, OW, OH)
    assert out[1:-2, 0].all() and out[0, 1:-2].all() and out[1:-2, 16].all() and out[16, 1:-2].all()      # partial taps, not border
    assert not out[:, 17].any() and not out[17].any()


def test_tie_case_depends_on_round_half_even():
    img, m, OW, OH = tie_case()
    assert in_range(m, OW, OH)
    x = np.arange(OW, dtype=np.float64)
    frac = m[0] * x * 1024.0 - np.floor(m[0] * x * 1024.0)
    assert int((frac == 0.5).sum()) == OW // 2                                  # every odd x is a tie
    a, b = coords(m, OW, OH), coords(m, OW, OH, rnd=half_away)
    moved = (a[2] != b[2]) | (a[0] != b[0]) | (a[3] != b[3]) | (a[1] != b[1])
    changed = (ref_u8(img, m, OW, OH) != ref_u8(img, m, OW, OH, rnd=half_away)).any(-1)
    print(f"ties: {int(moved.sum())} coordinates and {int(changed.sum())} output pixels depend on the rounding rule")
    assert int(changed.sum()) >= 32


def test_saturation_case_needs_the_saturation():
    imgs, ms, OW, OH = saturation_case()
    changed = 0
    for v, (img, m) in enumerate(zip(imgs, ms)):
        assert in_range(m, OW, OH)
        sat, raw = coords(m, OW, OH), coords(m, OW, OH, sat=False)
        assert not (np.array_equal(sat[0], raw[0]) and np.array_equal(sat[1], raw[1])), v
        assert max(np.abs(raw[0]).max(), np.abs(raw[1]).max()) > 32768
        changed += int((ref_u8(img, m, OW, OH) != ref_u8(img, m, OW, OH, sat=False)).any(-1).sum())
    raw = coords(ms[0], OW, OH, sat=False)
    wx, wy = raw[0].astype(np.int16), raw[1].astype(np.int16)                   # what an unsaturated short would hold
    assert ((wx >= 0) & (wx < 2) & (wy >= 0) & (wy < 2)).sum() >= 4             # taps inside the 2 x 2 source
    assert not ref_u8(imgs[0], ms[0], OW, OH).any()                             # the saturated ones read the border
    assert changed >= 8                                                         # views 1, 2: an unsaturated int reads other pixels


def test_gains_cover_truncation_and_both_clips():
    p = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2)
    for g in GAINS:
        assert not np.isnan(g).any()
    a = to.color_jitter_u8(p, GAINS[0])
    assert not a[..., 0].any() and a[..., 1].max() == 255 and not a[..., 2].any()
    b = to.color_jitter_u8(p, GAINS[1])
    even = np.arange(0, 256, 2)
    assert np.array_equal(b[..., 0].reshape(-1)[even], even // 2)               # exact integers
    assert np.array_equal(b[..., 1].reshape(-1)[even[1:]], even[1:] // 2 - 1)   # just below: truncated, not rounded
    assert (p.astype(np.float64) * 300.0 > 2 ** 8).any()                        # a cast before the clip would wrap these


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
class _Launch:
    """One poem_warp_affine call on sources packed back to back; outputs between guards."""

    def __init__(self, imgs, ms, OW, OH, gains=None, f32=True, u8=True, u8_shift=0, f32_shift=0):
        V = len(imgs)
        self.V, self.OW, self.OH = V, OW, OH
        sizes = [im.size for im in imgs]
        offs = np.cumsum([0] + sizes)
        blob = np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in imgs] + [np.full(_GUARD, 255, np.uint8)])
        self.src = torch.from_numpy(blob).to(DEV)
        self.off = torch.from_numpy(offs[:-1].astype(np.int64)).to(DEV)
        self.hw = torch.from_numpy(np.asarray([im.shape[:2] for im in imgs], np.int32)).to(DEV)
        self.m = torch.from_numpy(np.ascontiguousarray(np.asarray(ms, np.float64).reshape(V, 6))).to(DEV)
        self.g = None if gains is None else torch.from_numpy(np.ascontiguousarray(np.asarray(gains, np.float64).reshape(V, 3))).to(DEV)
        n = V * OH * OW * 3
        self.n, self.u8_shift, self.f32_shift = n, u8_shift, f32_shift
        self.u8 = torch.full((n + 2 * _GUARD + 4,), _BYTE, dtype=torch.uint8, device=DEV) if u8 else None
        self.f32 = torch.full((n + 2 * _GUARD + 4,), _CANARY, dtype=torch.int32, device=DEV) if f32 else None

    def ptrs(self):
        return (None if self.f32 is None else self.f32.data_ptr() + 4 * _GUARD + self.f32_shift,
                None if self.u8 is None else self.u8.data_ptr() + _GUARD + self.u8_shift)

    def call(self, views=None, OH=None, null=()):
        import poem_v2_amd as pk
        pf, pu = self.ptrs()
        a = dict(src=self.src.data_ptr(), off=self.off.data_ptr(), hw=self.hw.data_ptr(), m=self.m.data_ptr(),
                 g=None if self.g is None else self.g.data_ptr(), f32=pf, u8=pu)
        for k in null:
            a[k] = None
        rc = pk.hip.lib().poem_warp_affine(a["src"], a["off"], a["hw"], a["m"], a["g"], a["f32"], a["u8"],
                                           self.V if views is None else views, self.OH if OH is None else OH, self.OW, pk.hip.stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return (self.u8 is None or bool((self.u8 == _BYTE).all())) and (self.f32 is None or bool((self.f32 == _CANARY).all()))

    def take(self, what):
        """-> (u8 (V,OH,OW,3) or None, f32 (V,3,OH,OW) or None); asserts the guards."""
        u8 = f32 = None
        if self.u8 is not None:
            b, s = self.u8.cpu().numpy(), _GUARD + self.u8_shift
            assert (b[:s] == _BYTE).all() and (b[s + self.n:] == _BYTE).all(), f"{what}: a guard byte was written"
            u8 = b[s:s + self.n].reshape(self.V, self.OH, self.OW, 3)
        if self.f32 is not None:
            b = self.f32.cpu().numpy()
            s = _GUARD + self.f32_shift // 4
            assert (b[:s] == _CANARY).all() and (b[s + self.n:] == _CANARY).all(), f"{what}: a guard float was written"
            f32 = b[s:s + self.n].view(np.float32).reshape(self.V, 3, self.OH, self.OW)
        return u8, f32


def _check(imgs, ms, OW, OH, refs, gains, what, **kw):
    """The three output configurations of one input against the references (list over views of uint8 (OH,OW,3))."""
    for f32, u8 in ((False, True), (True, False), (True, True)):
        la = _Launch(imgs, ms, OW, OH, gains=gains, f32=f32, u8=u8, **kw)
        assert la.call() == 0, what
        gu, gf = la.take(f"{what} f32={f32} u8={u8}")
        for v, ref in enumerate(refs):
            if u8:
                assert np.array_equal(gu[v], ref), f"{what}: view {v} uint8 (f32={f32}): {int((gu[v] != ref).sum())} bytes differ"
            if f32:
                want = to.to_tensor_normalize(ref)
                assert np.array_equal(gf[v].view(np.uint32), want.view(np.uint32)), f"{what}: view {v} fp32 (u8={u8})"


@pytest.mark.gpu
@pytest.mark.parametrize("OW", OWS)
def test_hip_every_output_shape_and_configuration(OW):
    """Each width with each height, two views of tiny sources (the second wholly outside: all zeros), out_u8 alone, out_f32 alone and
    both in one launch, with and without gains.  For OW % 4 != 0 equality of whole rows shows that no dword store reached the next
    row; the guards show the same for the last one."""
    for OH in OHS:
        imgs, ms = tiny_views(2, OW, OH, seed=OW * 16 + OH, first=OW + OH)
        assert all(in_range(m, OW, OH) for m in ms)
        refs = [ref_u8(im, m, OW, OH) for im, m in zip(imgs, ms)]
        assert (refs[0].any() or OW * OH < 9) and not refs[1].any()
        _check(imgs, ms, OW, OH, refs, None, f"{OW}x{OH}")
        gains = GAINS[[3, 1]]
        _check(imgs, ms, OW, OH, [to.color_jitter_u8(r, g) for r, g in zip(refs, gains)], gains, f"{OW}x{OH} gains")


@pytest.mark.gpu
@pytest.mark.parametrize("views", [1, 70])
def test_hip_view_counts(views):
    """1 and 70 views (grid z), every tiny source size in turn, truly back to back: odd byte offsets, 3 * sw % 4 != 0."""
    for OW, OH in ((259, 5), (8, 3)):
        imgs, ms = tiny_views(views, OW, OH, seed=views)
        refs = [ref_u8(im, m, OW, OH) for im, m in zip(imgs, ms)]
        gains = GAINS[np.arange(views) % 4]
        _check(imgs, ms, OW, OH, refs, None, f"{views} views {OW}x{OH}")
        _check(imgs, ms, OW, OH, [to.color_jitter_u8(r, g) for r, g in zip(refs, gains)], gains, f"{views} views {OW}x{OH} gains")


@pytest.mark.gpu
def test_hip_borders_ties_and_saturation():
    img, m, OW, OH = border_case()
    _check([img], [m], OW, OH, [ref_u8(img, m, OW, OH)], None, "borders")
    img, m, OW, OH = tie_case()
    _check([img], [m], OW, OH, [ref_u8(img, m, OW, OH)], None, "ties")
    imgs, ms, OW, OH = saturation_case()
    _check(imgs, ms, OW, OH, [ref_u8(im, mm, OW, OH) for im, mm in zip(imgs, ms)], None, "saturation")


@pytest.mark.gpu
def test_hip_gains():
    """Gain 0, a gain that clips at 255, a negative gain (0), products that are exact integers and just below one (truncation), on
    every byte value: a 16 x 16 ramp through the identity."""
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    ident = np.array([1.0, 0, 0, 0, 1.0, 0])
    imgs, ms = [ramp] * len(GAINS), [ident] * len(GAINS)
    refs = [to.color_jitter_u8(ref_u8(ramp, ident, 16, 16), g) for g in GAINS]
    assert np.array_equal(ref_u8(ramp, ident, 16, 16), ramp)
    _check(imgs, ms, 16, 16, refs, GAINS, "gains, vector stores")
    refs = [r[:, :15] for r in refs]
    _check(imgs, ms, 15, 16, [np.ascontiguousarray(r) for r in refs], GAINS, "gains, scalar stores")


@pytest.mark.gpu
def test_hip_misaligned_output_bases_take_the_scalar_stores():
    """OW % 4 == 0 with out_u8 one byte and out_f32 four bytes off their alignment: the launcher routes these to the scalar stores
    (a dword store at an odd address, or a float4 store off 16 bytes, is what it must not issue); results and guards as ever."""
    for OW, OH in ((8, 3), (256, 5), (260, 4)):
        imgs, ms = tiny_views(2, OW, OH, seed=OW)
        refs = [ref_u8(im, m, OW, OH) for im, m in zip(imgs, ms)]
        for us, fs in ((1, 0), (0, 4), (1, 4), (2, 8), (3, 12)):
            _check(imgs, ms, OW, OH, refs, None, f"{OW}x{OH} u8 base +{us} f32 base +{fs}", u8_shift=us, f32_shift=fs)


@pytest.mark.gpu
def test_hip_refusals_leave_the_outputs_alone():
    imgs, ms = tiny_views(2, 8, 4, seed=9)
    la = _Launch(imgs, ms, 8, 4)
    assert la.call(views=65536) == -4 and la.untouched()                       # POEM_E_UNSUPPORTED: grid z
    assert la.call(OH=262141) == -4 and la.untouched()                         # grid y: 4 * 65535 rows
    for null in (("src",), ("off",), ("hw",), ("m",), ("f32", "u8")):
        assert la.call(null=null) == -1 and la.untouched(), null               # POEM_E_ARG
    assert la.call(views=0) == -1 and la.call(OH=0) == -1 and la.untouched()
    assert la.call(null=("g",)) == 0 and not la.untouched()                    # gains are optional


@pytest.mark.gpu
def test_hip_warp_views_gives_the_same_pixels():
    """The Python surface (it inverts the forward matrix itself) against the oracle's own path, fp32 and uint8."""
    import poem_v2_amd as pk
    g = np.random.default_rng(12)
    imgs = [g.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in SIZES + [(9, 11)]]
    Ms = [np.array([[g.uniform(20, 40), g.uniform(-2, 2), g.uniform(-5, 5)], [g.uniform(-2, 2), g.uniform(1, 3), g.uniform(-2, 2)]],
                   np.float32) for _ in imgs]
    gains = GAINS[np.arange(len(imgs)) % 4]
    for size in ((257, 5), (260, 9)):
        u8 = pk.transform.warp_views(imgs, Ms, size, gains=gains, device=DEV, out="u8").cpu().numpy()
        f32 = pk.transform.warp_views(imgs, Ms, size, device=DEV).cpu().numpy()
        for v, (im, M) in enumerate(zip(imgs, Ms)):
            ref = to.warp_affine_u8(im, M, size)
            assert np.array_equal(u8[v], to.color_jitter_u8(ref, gains[v])) and np.array_equal(f32[v], to.to_tensor_normalize(ref)), v
