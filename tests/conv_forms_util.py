"""Plain-Python side of tests/test_conv_forms.py: the routing of csrc/decode.hip's launchers mirrored (which template
instantiation a call runs, or that the entry point refuses), the fp64 / fp32 restatements of the operations, and the case
tables.  Nothing here touches the GPU; tests/test_host_logic.py checks the mirror on literal expectations and that every shape
the decoders and the backbone engines launch lands on a form the case tables cover.  TEST INFRASTRUCTURE -- NOT PRODUCT CODE."""
import torch
import torch.nn.functional as F

DEFAULTS = {"row_stager": 3, "pool_fused": 1, "pin32": 1, "s2_staging_wave": 1}


# ---------------------------------------------------------------------------------------------------------------------
# the launchers' arithmetic (decode.hip: conv3x3_m16, conv3x3_lds_ok, conv3x3_s2_shape, s2_blocks_per_cu)
def m16(cout):
    """16-row fragments pad fewer output channels than 32-row ones, and at most five tiles of them"""
    return (cout + 15) // 16 * 16 < (cout + 31) // 32 * 32 and (cout + 15) // 16 <= 5


def lds_ok(cout, h, w):
    return (cout + 31) // 32 <= 5 and 0 < w <= 64 and 256 % w == 0 and h % (256 // w) == 0 and \
        8 * (256 // w + 2) * (w + 2) <= 7 * 512


def s2_shape(cout, h, w):
    if h != w or h % 16:
        return 0
    return {(80, 64): 1, (160, 32): 2, (320, 16): 3}.get((cout, w), 0)


def s2_blocks_per_cu(tiles, cus, forced=0):
    if forced:
        return forced
    tpc = (tiles + cus - 1) // cus
    return 2 if tpc >= 2 and tpc % 3 == 1 else 3


def s2p_grid(views, h, cus, forced=0):
    """(tiles, blocks) of conv3x3_s2p_kernel: four-row output tiles dealt round-robin to persistent blocks"""
    tiles = views * (h // 2 // 4)
    return tiles, min(tiles, s2_blocks_per_cu(tiles, cus, forced) * cus)


def pool_head_fits(cout, j):
    """the fused head's pooled rows (Cout x 4 x 32) and weights (J x Cout + J) inside the idle staging tile (W = 64)"""
    tplane = (4 + 2) * (64 + 2)
    tstride = ((tplane + 15) & ~31) + 16
    return (cout * 128 + j * cout + j) * 4 <= 2 * 8 * tstride * 4


def _lds_form(cout, w, upcat, ex, ca, cb, opt):
    if m16(cout):
        ct16 = {1: 1, 3: 3}.get((cout + 15) // 16, 5)
        rw = 0
        if upcat and ca % 8 == 0 and cb % 8 == 0 and ((w == 64 and opt["row_stager"] & 1) or (w == 32 and opt["row_stager"] & 2)):
            rw = w
        return ("lds16", ct16, upcat, rw, False, ex)
    ct = min((cout + 31) // 32, 5)
    return ("lds", ct, upcat, bool(upcat and ct == 5 and opt["pin32"]), ex)


def route(kind, cin, cout, h, w, stride=1, ex=False, j=0, **options):
    """The kernel instantiation a call runs, or None where the entry point answers POEM_E_UNSUPPORTED:
      "conv3"     poem_conv3x3 / poem_conv3x3_ex (``ex``)      -> ("direct", CT, PT, EX) | ("lds", CT, UPCAT, PIN, EX) |
                                                                  ("lds16", CT16, UPCAT, RW, POOL, EX)
      "upcat"     poem_upcat_conv3x3, cin = (ca, cb)           -> the two LDS forms with UPCAT
      "pool_head" poem_upcat_conv3x3_pool_head, cin = (ca, cb) -> ("lds16", 3, True, 64, True, False)
      "down2"     poem_conv3x3_down2                           -> ("s2p", PXB, CG, MAXLD, ROWS) | ("s2", PXB, CG, MAXLD)
      "up2"       poem_conv1x1_upsample2 (cin = K, cout = C)   -> ("conv1x1_up2", 10)
      "pool"      poem_pool_conv1x1_sigmoid (cin = C, j)       -> ("pool_head",)
    options: the decode options (poem_set_decode_option), defaults as the library's."""
    opt = dict(DEFAULTS, **options)
    if kind == "conv3":
        if cin % 8 or stride not in (1, 2) or h % stride or w % stride or ((h // stride) * (w // stride)) % 32:
            return None
        if cin * (h + 2) * (w + 2) * 4 >= 1 << 31:
            return None
        if stride == 1 and lds_ok(cout, h, w):
            return _lds_form(cout, w, False, ex, 0, 0, opt)
        cot, ptiles = (cout + 31) // 32, (h // stride) * (w // stride) // 32
        ct = 5 if cot % 5 == 0 else 3 if cot % 3 == 0 else 2 if cot % 2 == 0 else 1
        return ("direct", ct, 2 if ptiles % 2 == 0 else 1, ex)
    if kind == "upcat":
        ca, cb = cin
        if ca % 8 or cb % 8 or ca + cb <= 0 or h % 2 or w % 2 or not lds_ok(cout, h, w) or (h // 2) * (w // 2) >= 1 << 20:
            return None
        return _lds_form(cout, w, True, False, ca, cb, opt)
    if kind == "pool_head":
        ca, cb = cin
        if ca % 8 or cb % 8 or ca <= 0 or cb <= 0 or w != 64 or h % 4 or not lds_ok(cout, h, w) or not m16(cout) or \
                (cout + 15) // 16 != 3 or j < 1 or j > 32 or not opt["row_stager"] & 1 or not opt["pool_fused"]:
            return None
        return ("lds16", 3, True, 64, True, False) if pool_head_fits(cout, j) else None
    if kind == "down2":
        shape = s2_shape(cout, h, w)
        if not shape or cin % 8:
            return None
        if opt["s2_staging_wave"]:
            return ("s2p",) + {1: (4, 1, 18), 2: (2, 2, 9), 3: (1, 4, 5)}[shape] + (4,)
        return ("s2",) + {1: (8, 1, 18), 2: (4, 2, 10), 3: (2, 4, 5)}[shape]
    if kind == "up2":
        if h != 8 or w != 8 or cin % 8 or cout % 32 or (cin + cout) * 64 * 4 > 160 * 1024:
            return None
        return ("conv1x1_up2", 10)
    if kind == "pool":
        return None if cin > 64 or j > 32 or h % 2 or w % 2 else ("pool_head",)
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------------
# restatements (CPU), in the dtype asked for, from the fp32 inputs
def relu_nan(t):
    return torch.where(t < 0, torch.zeros_like(t), t)


def upcat_ref(a, b, dtype):
    """[bilinear x2 of a | b]; either may be None"""
    parts = []
    if a is not None and a.shape[1]:
        parts.append(F.interpolate(a.to(dtype), scale_factor=2, mode="bilinear", align_corners=False))
    if b is not None and b.shape[1]:
        parts.append(b.to(dtype))
    return torch.cat(parts, dim=1)


def conv3_ref(x, wt, scale, shift, dtype, stride=1, relu=1, res=None, res_pre=0):
    """act(conv3x3(x) * scale + shift [+ res]) [+ res]: the residual before (res_pre) or after the activation"""
    y = F.conv2d(x.to(dtype), wt.to(dtype), stride=stride, padding=1)
    y = y * scale.to(dtype).view(1, -1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1)
    return tail_ref(y, relu, res, res_pre)


def tail_ref(y, relu=1, res=None, res_pre=0):
    """the epilogue behind the affine, in the dtype of ``y``"""
    dtype = y.dtype
    if res is not None and res_pre:
        y = y + res.to(dtype)
    if relu:
        y = relu_nan(y)
    if res is not None and not res_pre:
        y = y + res.to(dtype)
    return y


def head_ref(y, hw, hb, dtype):
    """max_pool2d(2, 2) -> 1x1 convolution (J x C, bias) -> sigmoid"""
    p = F.max_pool2d(y.to(dtype), kernel_size=2, stride=2)
    return torch.sigmoid(torch.einsum("jc,nchw->njhw", hw.to(dtype), p) + hb.to(dtype).view(1, -1, 1, 1))


def up2_ref(x, wt, bias, dtype):
    """the reference's order: bilinear x2, then the 1x1 convolution"""
    up = F.interpolate(x.to(dtype), scale_factor=2, mode="bilinear", align_corners=False)
    y = torch.einsum("oc,nchw->nohw", wt.to(dtype), up)
    return y if bias is None else y + bias.to(dtype).view(1, -1, 1, 1)


def conv_data(g, views, cin, cout, h, w, integers, ho=None, wo=None):
    """input, weights, affine and residual of one case: random, or small integers whose every partial sum is exact in fp32"""
    ho, wo = ho or h, wo or w
    if integers:
        x = torch.randint(-3, 4, (views, cin, h, w), generator=g).float()
        wt = torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).float()
        scale, shift = torch.ones(cout), torch.randint(-5, 6, (cout,), generator=g).float()
        res = torch.randint(-9, 10, (views, cout, ho, wo), generator=g).float()
    else:
        x = torch.randn(views, cin, h, w, generator=g)
        wt = torch.randn(cout, cin, 3, 3, generator=g) * (1.6 / (9 * cin)) ** 0.5
        wt = torch.where(wt == 0, torch.full_like(wt, 0.01), wt)               # the NaN cases rely on non-zero weights
        scale, shift = 1 + 0.2 * (2 * torch.rand(cout, generator=g) - 1), 0.3 * torch.randn(cout, generator=g)
        res = torch.randn(views, cout, ho, wo, generator=g)
    return x, wt, scale, shift, res


def upcat_data(g, views, ca, cb, h, w, integers):
    """a (views, ca, h/2, w/2) and b (views, cb, h, w); integers: a in multiples of 16, so every bilinear tap product
    (weights in sixteenths) stays an integer"""
    if integers:
        a = 16.0 * torch.randint(-3, 4, (views, ca, h // 2, w // 2), generator=g).float()
        b = torch.randint(-3, 4, (views, cb, h, w), generator=g).float()
    else:
        a, b = torch.randn(views, ca, h // 2, w // 2, generator=g), torch.randn(views, cb, h, w, generator=g)
    return a, b


def poison(t, variant, view=1):
    """a copy with one non-finite value: "nan00" NaN at pixel (0, 0) of channel 0, "nan_in" NaN at an interior pixel of the
    last channel, "inf00" +Inf at (0, 0) of channel 0 -- all in view ``view``"""
    t = t.clone()
    n = min(view, t.shape[0] - 1)
    if variant == "nan00":
        t[n, 0, 0, 0] = float("nan")
    elif variant == "nan_in":
        t[n, -1, t.shape[2] // 2, t.shape[3] // 2] = float("nan")
    elif variant == "inf00":
        t[n, 0, 0, 0] = float("inf")
    else:
        raise ValueError(variant)
    return t


POISONS = ("nan00", "nan_in", "inf00")


# ---------------------------------------------------------------------------------------------------------------------
# case tables (the smallest shapes at which each form can go wrong; tests/test_conv_forms.py has the coverage table)
DIRECT_CASES = [  # cin, cout, h, w, stride
    (8, 32, 4, 8, 1), (16, 32, 8, 8, 1), (40, 32, 2, 48, 1),              # CT 1: PT 1 / 2, a tile crossing a row mid-row
    (40, 40, 12, 8, 1), (16, 40, 16, 8, 1), (40, 40, 16, 16, 2),          # CT 2 with an 8-channel tail: three / two pixel groups
    (8, 96, 2, 48, 1), (16, 96, 8, 8, 1), (8, 96, 8, 16, 2),              # CT 3
    (8, 160, 4, 8, 1), (16, 160, 16, 16, 2), (8, 160, 16, 8, 1),          # CT 5
    (8, 224, 8, 16, 2), (16, 200, 8, 32, 2), (8, 200, 12, 8, 1),          # seven channel groups of CT 1; with a tail
    (16, 224, 16, 8, 1),
]

LDS_COUTS = (32, 64, 96, 128, 100, 160, 130)                  # conv3x3_lds_kernel CT 1..5 (100: CT 4 with a tail)
LDS16_COUTS = (16, 9, 1, 48, 40, 33, 80, 65)                  # conv3x3_lds16_kernel CT16 1 / 3 / 5
LDS_WIDTHS = (4, 8, 16, 32, 64)
CINS = (8, 16, 24)


def lds_cases():
    """(cin, cout, h, w): per kernel family every width with H = TR, 2 TR, 3 TR and with Cin 8, 16, 24"""
    out = []
    for couts in (LDS_COUTS, LDS16_COUTS):
        for ci, cout in enumerate(couts):
            for wi, w in enumerate(LDS_WIDTHS):
                out.append((CINS[(ci + 2 * wi) % 3], cout, (1 + (ci + wi) % 3) * (256 // w), w))
    return out


UPCAT_COUTS = (32, 64, 96, 128, 160, 16, 40, 80, 100, 33)
UPCAT_SHAPES = ((4, 64), (8, 64), (12, 64), (8, 32), (16, 32), (24, 32), (64, 4), (32, 8), (16, 16), (32, 16))   # (h, w)
CACB = ((8, 8), (16, 8), (8, 16), (24, 8), (0, 16), (16, 0), (8, 0), (0, 8))


def upcat_cases():
    """(ca, cb, cout, h, w): every cout on every shape, the channel splits dealt over them"""
    return [CACB[(ci + 3 * si) % 8] + (cout, h, w) for ci, cout in enumerate(UPCAT_COUTS) for si, (h, w) in enumerate(UPCAT_SHAPES)]


UPCAT_REFUSED = [(12, 8, 40, 16, 16), (8, 8, 40, 7, 16), (8, 8, 161, 16, 16), (8, 8, 40, 2, 128)]       # Ca % 8, odd H, Cout, W

POOL_HEAD_CASES = [  # ca, cb, cout, j, h, taken
    (8, 8, 33, 1, 4, True), (16, 24, 33, 21, 8, True), (8, 8, 33, 32, 12, True),
    (16, 24, 40, 1, 12, True), (8, 8, 40, 21, 8, True), (16, 24, 40, 31, 4, True), (8, 8, 40, 32, 4, False),
    (8, 8, 48, 1, 8, True), (16, 24, 48, 5, 12, True), (8, 8, 48, 6, 4, False), (16, 24, 48, 21, 8, False),
]

DOWN2_SHAPES = ((80, 64), (160, 32), (320, 16))          # (cout, side)
DOWN2_REFUSED = [(40, 96, 64, 64), (40, 80, 64, 32), (12, 80, 64, 64)]      # cin, cout, h, w

UP2_CASES = [(8, 32, True), (40, 160, True), (8, 192, True), (448, 192, True), (456, 192, False), (40, 48, False)]   # K, C, taken
POOL_CASES = [(1, 1), (40, 21), (64, 32)]                # (C, J), each on 2 x 2 and 6 x 10 maps


def tested_forms():
    """every instantiation tests/test_conv_forms.py runs a case on, as route() names them"""
    forms = set()
    for cin, cout, h, w, stride in DIRECT_CASES:
        forms |= {route("conv3", cin, cout, h, w, stride, ex=e) for e in (False, True)}
    for cin, cout, h, w in lds_cases():
        forms |= {route("conv3", cin, cout, h, w, 1, ex=e) for e in (False, True)}
    for ca, cb, cout, h, w in upcat_cases():
        forms.add(route("upcat", (ca, cb), cout, h, w))
        forms.add(route("upcat", (ca, cb), cout, h, w, row_stager=0, pin32=0))
    for ca, cb, cout, j, h, taken in POOL_HEAD_CASES:
        forms.add(route("pool_head", (ca, cb), cout, h, 64, j=j))
    for cout, side in DOWN2_SHAPES:
        forms |= {route("down2", 8, cout, side, side, s2_staging_wave=s) for s in (0, 1)}
    forms.add(route("up2", 8, 32, 8, 8))
    forms.add(route("pool", 40, 21, 2, 2, j=21))
    forms.discard(None)
    return forms
