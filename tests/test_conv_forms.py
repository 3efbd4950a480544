"""The convolution family of csrc/decode.hip in every form its launchers route to, through the C ABI.

Coverage (form x case; the route mirror of tests/conv_forms_util.py names the instantiation and every case asserts it -- and,
where the entry point can refuse, that the library's taken / POEM_E_UNSUPPORTED answer is the mirror's -- before it runs):

    form                                            cases                                                         test
    conv3x3_kernel<CT,PT,EX>  CT 1/2/3/5 x PT 1/2   Cout 32/40/96/160/224/200, Cin 8/16/40, stride 1 on 4x8 12x8   test_conv3x3_direct
      x EX 0/1                                      8x8 16x8 2x48 (a tile crossing a row), stride 2 on 8x16
                                                    16x16 8x32; one..three pixel groups, idle waves in the last block
    conv3x3_lds_kernel<CT,false,false,EX> CT 1..5   Cout 32/64/96/128/100/160/130 x W 4..64 x H = TR, 2TR, 3TR       test_conv3x3_lds
    conv3x3_lds16_kernel<CT16,false,0,false,EX>     Cout 16/9/1, 48/40/33, 80/65 on the same maps; Cin 8/16/24      test_conv3x3_lds
    conv3x3_lds_kernel<1..4,true>, <5,true,PIN>,    Cout 32..160 and 100 x W 64 (H 4/8/12), 32 (8/16/24), 4, 8, 16;   test_upcat_conv3x3
      <5,true,false> (pin32 0)                      (Ca, Cb) from (8,8) to (0,8) incl. Ca = 0, Cb = 0, one chunk
    conv3x3_lds16_kernel<CT16,true,0|64|32>         Cout 16/40/80/33 on the same maps; row_stager 0/1/2/3            test_upcat_conv3x3
    conv3x3_lds16_kernel<3,true,64,POOL>            Cout 33/40/48 x J 1/21/31/32/5 x H 4/8/12, both sides of the fit  test_pool_head_fused
    conv3x3_s2p_kernel<4,1,18,4> <2,2,9,4> <1,4,5,4> the three shapes x Cin 8/16/24, one view; at 16^2 blocks walking   test_conv3x3_down2,
    conv3x3_s2_kernel<8,1,18> <4,2,10> <2,4,5>      two and three tiles under s2_staging_wave 1/2/3/4 against 0       test_down2_many_tiles
    conv1x1_up2_kernel<10>                          (K, C) (8,32) (40,160) (8,192: 12 jobs, 10 waves) (448,192: LDS)  test_conv1x1_upsample2
    pool_head_kernel                                (C, J) (1,1) (40,21) (64,32) on 2x2 and 6x10                      test_pool_conv1x1_sigmoid
    upcat_pad_kernel<false> / <true> (staged)       the two-launch side of every fused case                          test_upcat_conv3x3
    every family, NaN / +Inf in the input           one case each, both stagers, both pools, both stride-2 kernels    test_non_finite_inputs
    FeatureDecoders (HRNet, resnet34)               a NaN in the finest and in the coarsest level, all routes          test_decoders_keep_a_nan

Bars (the project's own):
  * max|HIP - fp64| <= 4 max|fp32_cpu - fp64| + 1e-6 max|fp64|   (tests/test_backbone_hip.py);
  * on small-integer data (inputs -3..3, weights -2..2, scale 1, integer shift and residual; the interpolated tensor in multiples
    of 16, so every bilinear tap product is an integer) the fp64 result exactly.  Behind a sigmoid the integer logits are exact and
    the bar is 6 * 2^-24: expf 1 ulp, the addition 0.5, the division 2.5, of a result <= 1, with headroom for their product terms;
  * the same bits wherever the code promises them: the fused input against poem_upsample2_concat_pad_staged + poem_conv3x3,
    row_stager 0/1/2/3, pin32 0/1, s2_staging_wave 0..4, pool_fused 0/1 and the fused head against its two launches,
    poem_conv3x3 against poem_conv3x3_ex(res_pre = 0);
  * outputs land in the interior of a sentinel-bordered buffer whose border stays untouched, residuals come from the interior of
    a junk-bordered one, refused calls write nothing.

Non-finite inputs: one NaN at pixel (0, 0) of channel 0 of view 1, one NaN at an interior pixel of the last channel, one +Inf at
(0, 0) of channel 0.  The non-finite mask equals the fp32 CPU restatement's; every output the poisoned pixel does not reach (the
CPU's poisoned and clean results agree there) has the bits of the clean run of the same launch; an output it reaches and leaves
finite -- relu(-Inf) = 0 -- cannot equal the clean run and is held to the CPU's value instead."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import conv_forms_util as cu
import decode_oracle as do
import poem_v2_amd as pk
import resnet_util as ru
from conv_forms_util import route
from poem_v2_amd import hip
from test_backbone_hip import DEV, SENTINEL, _border_is, _buffer, _Conv3, _criterion, _plain

pytestmark = pytest.mark.gpu
VIEWS = 3
OK, REFUSED = 0, hip.POEM_E_UNSUPPORTED


@contextlib.contextmanager
def options(**kw):
    """decode options for the block; the library's defaults afterwards, whatever happens inside"""
    L = hip.lib()
    try:
        for k, v in kw.items():
            hip.check(L.poem_set_decode_option(k.encode(), v), "poem_set_decode_option")
        yield
    finally:
        for k, v in cu.DEFAULTS.items():
            L.poem_set_decode_option(k.encode(), v)


def _bits(t):
    return torch.nan_to_num(t.detach().cpu().contiguous(), nan=1.0).view(torch.int32)


def bits_equal(a, b):
    """the same NaN mask and, elsewhere, the same bits"""
    a, b = a.detach().cpu(), b.detach().cpu()
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(_bits(a), _bits(b))


def _out(views, c, h, w, bordered, g):
    return _buffer(torch.zeros(views, c, h, w), bordered, SENTINEL, g)


def _dev(t):
    return None if t is None or t.numel() == 0 else t.to(DEV).contiguous()


def _check(got, ref64, ref32, integers, what):
    if integers:
        assert torch.equal(got.cpu().double(), ref64), what
    else:
        _criterion(got, ref64, ref32, what)


# ---- poem_conv3x3 / poem_conv3x3_ex: the direct kernel and the two LDS-staged ones -----------------------------------------------
def _conv3_case(cin, cout, h, w, stride, family):
    forms = [route("conv3", cin, cout, h, w, stride, ex=e) for e in (False, True)]
    assert forms[0][0] == forms[1][0] == family and forms[0][-1] is False and forms[1][-1] is True, forms
    print(f"{cin}->{cout} {h}x{w}/{stride}: {forms}")
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + h + 3 * w + stride)
    ho, wo = h // stride, w // stride
    for integers in (False, True):
        x, wt, scale, shift, res = cu.conv_data(g, VIEWS, cin, cout, h, w, integers, ho, wo)
        conv = _Conv3(wt, scale, shift)
        xp = F.pad(x, (1, 1, 1, 1)).to(DEV).contiguous()
        pre64, pre32 = (cu.conv3_ref(x, wt, scale, shift, dt, stride, relu=0) for dt in (torch.float64, torch.float32))
        rd = res.to(DEV).contiguous()
        # poem_conv3x3: ReLU then the lateral add, into a bordered buffer; no ReLU and no residual, plain
        old = {}
        for relu, r, bordered in ((1, rd, True), (0, None, False), (1, None, False), (0, rd, True)):
            obuf, oint, ostr = _out(VIEWS, cout, ho, wo, bordered, g)
            assert conv.old(xp, h, w, stride, r, obuf, ostr, relu) == OK
            rr = None if r is None else res
            _check(oint, cu.tail_ref(pre64, relu, None if rr is None else rr.double()), cu.tail_ref(pre32, relu, rr), integers,
                   f"conv3x3 {forms[0]} relu={relu} res={r is not None}")
            assert not bordered or _border_is(obuf, SENTINEL), "a store outside the interior"
            old[(relu, r is not None)] = oint.clone()
        # poem_conv3x3_ex: the residual from a junk-bordered buffer before the activation; and the old order, the same bits
        rbuf, _, rstr = _buffer(res, True, "rand", g)
        for relu, with_res, pre in ((1, True, 1), (0, True, 1), (1, False, 1), (1, True, 0), (0, False, 0), (1, False, 0), (0, True, 0)):
            obuf, oint, ostr = _out(VIEWS, cout, ho, wo, True, g)
            assert conv.ex(xp, h, w, stride, rbuf if with_res else None, rstr if with_res else (0, 0, 0, 0), pre, obuf, ostr, relu) == OK
            rr = res if with_res else None
            _check(oint, cu.tail_ref(pre64, relu, None if rr is None else rr.double(), pre), cu.tail_ref(pre32, relu, rr, pre), integers,
                   f"conv3x3_ex {forms[1]} relu={relu} res={with_res} pre={pre}")
            assert _border_is(obuf, SENTINEL), "a store outside the interior"
            if not pre:
                assert bits_equal(oint, old[(relu, with_res)]), "poem_conv3x3_ex(res_pre = 0) is poem_conv3x3"


@pytest.mark.parametrize("cin,cout,h,w,stride", cu.DIRECT_CASES)
def test_conv3x3_direct(cin, cout, h, w, stride):
    _conv3_case(cin, cout, h, w, stride, "direct")


def test_direct_cases_reach_all_eight_tilings():
    got = {route("conv3", *c)[1:3] for c in cu.DIRECT_CASES}
    assert got == {(ct, pt) for ct in (1, 2, 3, 5) for pt in (1, 2)}


@pytest.mark.parametrize("cin,cout,h,w", cu.lds_cases())
def test_conv3x3_lds(cin, cout, h, w):
    _conv3_case(cin, cout, h, w, 1, "lds16" if cu.m16(cout) else "lds")


def test_conv3x3_refusals():
    conv = _Conv3(torch.zeros(40, 16, 3, 3), torch.ones(40), torch.zeros(40))
    xp = torch.zeros(1, 16, 18, 18, device=DEV)
    out = torch.full((1, 40, 16, 16), SENTINEL, device=DEV)
    for h, w, stride in ((16, 16, 3), (6, 8, 1), (16, 15, 1), (12, 8, 2)):
        assert route("conv3", 16, 40, h, w, stride) is None
        assert conv.old(xp, h, w, stride, None, out, _plain(40, 16, 16)) == REFUSED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- poem_upcat_conv3x3: the fused [bilinear x2 of a | b] input ---------------------------------------------------------------------
def _upcat(conv, a, ca, b, cb, h, w, out, strides, relu=1, views=VIEWS):
    return hip.lib().poem_upcat_conv3x3(hip.ptr(a), ca, hip.ptr(b), cb, conv.packed.data_ptr(), hip.ptr(conv.scale), hip.ptr(conv.shift),
                                        out.data_ptr(), views, conv.cout, h, w, relu, *strides, hip.stream())


def _two_launch(conv, a, ca, b, cb, h, w, views=VIEWS, relu=1):
    """poem_upsample2_concat_pad_staged + poem_conv3x3"""
    xin = torch.empty(views, ca + cb, h + 2, w + 2, device=DEV)
    hip.check(hip.lib().poem_upsample2_concat_pad_staged(hip.ptr(a), ca, hip.ptr(b), cb, hip.ptr(xin), views, h, w, hip.stream()), "staged")
    out = torch.empty(views, conv.cout, h, w, device=DEV)
    assert conv.old(xin, h, w, 1, None, out, _plain(conv.cout, h, w), relu) == OK
    return out


@pytest.mark.parametrize("ca,cb,cout,h,w", cu.upcat_cases())
def test_upcat_conv3x3(ca, cb, cout, h, w):
    form = route("upcat", (ca, cb), cout, h, w)
    assert form is not None and form[2] is True
    print(f"[{ca}|{cb}]->{cout} {h}x{w}: {form}")
    g = torch.Generator().manual_seed(ca + 7 * cb + 100 * cout + h + 5 * w)
    for integers in (False, True):
        a, b = cu.upcat_data(g, VIEWS, ca, cb, h, w, integers)
        _, wt, scale, shift, _ = cu.conv_data(g, 1, ca + cb, cout, 2, 2, integers)
        conv = _Conv3(wt, scale, shift)
        ad, bd = _dev(a), _dev(b)
        ref64, ref32 = (cu.conv3_ref(cu.upcat_ref(a, b, dt), wt, scale, shift, dt) for dt in (torch.float64, torch.float32))
        one = torch.full((VIEWS, cout, h, w), SENTINEL, device=DEV)
        assert _upcat(conv, ad, ca, bd, cb, h, w, one, _plain(cout, h, w)) == OK
        _check(one, ref64, ref32, integers, f"upcat_conv3x3 {form}")
        obuf, oint, ostr = _out(VIEWS, cout, h, w, True, g)
        assert _upcat(conv, ad, ca, bd, cb, h, w, obuf, ostr) == OK
        assert bits_equal(oint, one) and _border_is(obuf, SENTINEL)
        assert bits_equal(_two_launch(conv, ad, ca, bd, cb, h, w), one), "the fused input is the staged tensor's convolution"
        # the A/B switches: other stagers and schedules, the same bits
        alts = []
        if form[0] == "lds16" and w in (64, 32):
            alts = [dict(row_stager=v) for v in (0, 1, 2)]
        elif form[0] == "lds" and form[1] == 5:
            alts = [dict(pin32=0)]
        for kw in alts:
            with options(**kw):
                alt = route("upcat", (ca, cb), cout, h, w, **kw)
                assert alt is not None and alt[:3] == form[:3]
                other = torch.full((VIEWS, cout, h, w), SENTINEL, device=DEV)
                assert _upcat(conv, ad, ca, bd, cb, h, w, other, _plain(cout, h, w)) == OK
                assert bits_equal(other, one), (form, alt)
        # without the ReLU
        if not integers:
            lin = torch.full((VIEWS, cout, h, w), SENTINEL, device=DEV)
            assert _upcat(conv, ad, ca, bd, cb, h, w, lin, _plain(cout, h, w), relu=0) == OK
            _criterion(lin, *(cu.conv3_ref(cu.upcat_ref(a, b, dt), wt, scale, shift, dt, relu=0) for dt in (torch.float64, torch.float32)),
                       f"upcat_conv3x3 {form} relu=0")


def test_upcat_cases_reach_every_fused_form():
    forms = {route("upcat", (ca, cb), cout, h, w, **kw) for ca, cb, cout, h, w in cu.upcat_cases()
             for kw in ({}, dict(row_stager=0), dict(row_stager=1), dict(row_stager=2), dict(pin32=0))}
    want = {("lds", ct, True, False, False) for ct in (1, 2, 3, 4, 5)} | {("lds", 5, True, True, False)} | \
        {("lds16", ct, True, rw, False, False) for ct in (1, 3, 5) for rw in (0, 64, 32)}
    assert forms == want


@pytest.mark.parametrize("ca,cb,cout,h,w", cu.UPCAT_REFUSED)
def test_upcat_conv3x3_refusals(ca, cb, cout, h, w):
    assert route("upcat", (ca, cb), cout, h, w) is None
    conv = _Conv3(torch.zeros(cout, 16, 3, 3), torch.ones(cout), torch.zeros(cout))
    a, b = torch.zeros(1, 16, 16, 64, device=DEV), torch.zeros(1, 16, 32, 128, device=DEV)
    out = torch.full((1, cout, 32, 128), SENTINEL, device=DEV)
    assert _upcat(conv, a, ca, b, cb, h, w, out, _plain(cout, h, w), views=1) == REFUSED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- poem_upcat_conv3x3_pool_head and poem_pool_conv1x1_sigmoid ---------------------------------------------------------------------
def _pool_head(conv, a, ca, b, cb, hw, hb, hmap, j, h, w, views=VIEWS, relu=1):
    return hip.lib().poem_upcat_conv3x3_pool_head(hip.ptr(a), ca, hip.ptr(b), cb, conv.packed.data_ptr(), hip.ptr(conv.scale),
                                                  hip.ptr(conv.shift), hip.ptr(hw), hip.ptr(hb), hmap.data_ptr(), views, conv.cout, j, h, w,
                                                  relu, hip.stream())


def _pool(y, hw, hb, hmap, c, j, h, w, views=VIEWS):
    return hip.lib().poem_pool_conv1x1_sigmoid(hip.ptr(y), hip.ptr(hw), hip.ptr(hb), hmap.data_ptr(), views, c, j, h, w, hip.stream())


def _head_data(g, j, c, integers):
    if integers:           # powers of two keep every product and partial sum exact
        return torch.randint(-1, 2, (j, c), generator=g).float() / 4096, torch.randint(-8, 9, (j,), generator=g).float() / 8
    hw = 0.3 * torch.randn(j, c, generator=g)
    return torch.where(hw == 0, torch.full_like(hw, 0.01), hw), 0.1 * torch.randn(j, generator=g)


SIGMOID_BAR = 6 * 2.0 ** -24


@pytest.mark.parametrize("ca,cb,cout,j,h,taken", cu.POOL_HEAD_CASES)
def test_pool_head_fused(ca, cb, cout, j, h, taken):
    w = 64
    form = route("pool_head", (ca, cb), cout, h, w, j=j)
    assert (form is not None) == taken and (not taken or form == ("lds16", 3, True, 64, True, False))
    g = torch.Generator().manual_seed(ca + 3 * cb + 50 * cout + j + h)
    for integers in (False, True):
        a, b = cu.upcat_data(g, VIEWS, ca, cb, h, w, integers)
        _, wt, scale, shift, _ = cu.conv_data(g, 1, ca + cb, cout, 2, 2, integers)
        hw, hb = _head_data(g, j, cout, integers)
        conv = _Conv3(wt, scale, shift)
        ad, bd, hwd, hbd = _dev(a), _dev(b), _dev(hw), _dev(hb)
        one = torch.full((VIEWS, j, h // 2, w // 2), SENTINEL, device=DEV)
        rc = _pool_head(conv, ad, ca, bd, cb, hwd, hbd, one, j, h, w)
        assert rc == (OK if taken else REFUSED)
        if not taken:
            torch.cuda.synchronize()
            assert bool((one == SENTINEL).all()), "a refused call wrote"
            return
        y = torch.empty(VIEWS, cout, h, w, device=DEV)
        assert _upcat(conv, ad, ca, bd, cb, h, w, y, _plain(cout, h, w)) == OK
        two = torch.full((VIEWS, j, h // 2, w // 2), SENTINEL, device=DEV)
        assert _pool(y, hwd, hbd, two, cout, j, h, w) == OK
        assert bits_equal(one, two), "the fused head is its two launches"
        y64, y32 = (cu.conv3_ref(cu.upcat_ref(a, b, dt), wt, scale, shift, dt) for dt in (torch.float64, torch.float32))
        ref64 = cu.head_ref(y64, hw, hb, torch.float64)
        if integers:
            assert torch.equal(y.cpu().double(), y64)
            err = float((one.cpu().double() - ref64).abs().max())
            print(f"pool head {cout}x{j} integers: max err {err:.3e}")
            assert err <= SIGMOID_BAR
        else:
            _criterion(one, ref64, cu.head_ref(y32, hw, hb, torch.float32), f"pool head {cout} x {j} at {h} x 64")
        for kw in (dict(pool_fused=0), dict(row_stager=2), dict(row_stager=0)):
            with options(**kw):
                assert route("pool_head", (ca, cb), cout, h, w, j=j, **kw) is None
                other = torch.full((VIEWS, j, h // 2, w // 2), SENTINEL, device=DEV)
                assert _pool_head(conv, ad, ca, bd, cb, hwd, hbd, other, j, h, w) == REFUSED
                torch.cuda.synchronize()
                assert bool((other == SENTINEL).all()), "a refused call wrote"


@pytest.mark.parametrize("cout,j,h,w", [(40, 21, 8, 32), (32, 21, 8, 64), (49, 5, 8, 64), (64, 5, 8, 64), (40, 33, 8, 64), (40, 21, 6, 64)])
def test_pool_head_fused_refusals(cout, j, h, w):
    assert route("pool_head", (8, 8), cout, h, w, j=j) is None
    conv = _Conv3(torch.zeros(cout, 16, 3, 3), torch.ones(cout), torch.zeros(cout))
    a, b = torch.zeros(1, 8, 4, 32, device=DEV), torch.zeros(1, 8, 8, 64, device=DEV)
    hw, hb = torch.zeros(j, cout, device=DEV), torch.zeros(j, device=DEV)
    out = torch.full((1, j, 4, 32), SENTINEL, device=DEV)
    assert _pool_head(conv, a, 8, b, 8, hw, hb, out, j, h, w, views=1) == REFUSED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("h,w", [(2, 2), (6, 10)])
@pytest.mark.parametrize("c,j", cu.POOL_CASES)
def test_pool_conv1x1_sigmoid(c, j, h, w):
    assert route("pool", c, 0, h, w, j=j) == ("pool_head",)
    g = torch.Generator().manual_seed(c + 5 * j + h)
    for integers in (False, True):
        y = torch.randint(-3, 4, (VIEWS, c, h, w), generator=g).float() if integers else torch.randn(VIEWS, c, h, w, generator=g)
        hw, hb = _head_data(g, j, c, integers)
        yd, hwd, hbd = _dev(y), _dev(hw), _dev(hb)
        out = torch.full((VIEWS, j, h // 2, w // 2), SENTINEL, device=DEV)
        assert _pool(yd, hwd, hbd, out, c, j, h, w) == OK
        ref64 = cu.head_ref(y, hw, hb, torch.float64)
        if integers:
            assert float((out.cpu().double() - ref64).abs().max()) <= SIGMOID_BAR
        else:
            _criterion(out, ref64, cu.head_ref(y, hw, hb, torch.float32), f"pool_conv1x1_sigmoid {c} x {j} at {h} x {w}")
    assert route("pool", 65, 0, 2, 2, j=1) is None and route("pool", 8, 0, 2, 2, j=33) is None and route("pool", 8, 0, 3, 2, j=1) is None
    for cc, jj, hh in ((65, 1, 2), (8, 33, 2), (8, 1, 3)):
        assert _pool(yd, hwd, hbd, out, cc, jj, hh, 2) == REFUSED


# ---- poem_conv3x3_down2 -----------------------------------------------------------------------------------------------------------
def _down2(conv, x, res, out, strides, side, relu, views):
    return hip.lib().poem_conv3x3_down2(hip.ptr(x), conv.packed.data_ptr(), hip.ptr(conv.scale), hip.ptr(conv.shift), hip.ptr(res),
                                        out.data_ptr(), views, conv.cin, conv.cout, side, side, relu, *strides, hip.stream())


S2_OPTIONS = (1, 0, 2, 3, 4)      # poem_set_decode_option("s2_staging_wave", v): 0 the every-wave-stages kernel; 2..4 forced blocks per CU


def _s2_option(v):
    """a forced block count keeps the kernel choice: select the staging-wave kernel first"""
    L = hip.lib()
    hip.check(L.poem_set_decode_option(b"s2_staging_wave", 1 if v else 0), "poem_set_decode_option")
    if v >= 2:
        hip.check(L.poem_set_decode_option(b"s2_staging_wave", v), "poem_set_decode_option")


@pytest.mark.parametrize("cin", cu.CINS)
@pytest.mark.parametrize("cout,side", cu.DOWN2_SHAPES)
def test_conv3x3_down2(cout, side, cin):
    views, ro = 1, side // 2
    assert route("down2", cin, cout, side, side)[0] == "s2p" and route("down2", cin, cout, side, side, s2_staging_wave=0)[0] == "s2"
    g = torch.Generator().manual_seed(cin + cout + side)
    for integers in (False, True):
        x, wt, scale, shift, res = cu.conv_data(g, views, cin, cout, side, side, integers, ro, ro)
        conv = _Conv3(wt, scale, shift)
        xd, rd = _dev(x), _dev(res)
        pre64, pre32 = (cu.conv3_ref(x, wt, scale, shift, dt, 2, relu=0) for dt in (torch.float64, torch.float32))
        for relu, r, bordered in ((1, rd, False), (0, None, True), (1, None, True), (0, rd, False)):
            rr = None if r is None else res
            ref64, ref32 = cu.tail_ref(pre64, relu, None if rr is None else rr.double()), cu.tail_ref(pre32, relu, rr)
            first = None
            try:
                for v in S2_OPTIONS:
                    _s2_option(v)
                    obuf, oint, ostr = _out(views, cout, ro, ro, bordered, g)
                    assert _down2(conv, xd, r, obuf, ostr, side, relu, views) == OK
                    assert not bordered or _border_is(obuf, SENTINEL), "a store outside the interior"
                    if first is None:
                        first = oint.clone()
                        _check(first, ref64, ref32, integers, f"conv3x3_down2 {cin}->{cout} at {side} relu={relu} res={r is not None}")
                    else:
                        assert bits_equal(oint, first), f"s2_staging_wave {v}"
            finally:
                hip.lib().poem_set_decode_option(b"s2_staging_wave", 1)


@pytest.mark.parametrize("option", (1, 2, 3, 4))
def test_down2_many_tiles(option):
    """8 -> 320 at 16 x 16 with so many views that the persistent blocks walk two and three tiles, the last ones one fewer,
    against the every-wave-stages kernel: the same bits; a few views against fp64"""
    cin, cout, side, ro = 8, 320, 16, 8
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    forced = option if option >= 2 else 0
    views = None
    for f in ((forced,) if forced else (3, 2)):
        v = (5 * f * cus) // 4
        if cu.s2_blocks_per_cu(2 * v, cus, forced) == f:
            views = v
            break
    assert views is not None
    tiles, blocks = cu.s2p_grid(views, side, cus, forced)
    assert 2 * blocks < tiles < 3 * blocks, (tiles, blocks)
    g = torch.Generator().manual_seed(option)
    x, wt, scale, shift, res = cu.conv_data(g, views, cin, cout, side, side, False, ro, ro)
    conv = _Conv3(wt, scale, shift)
    xd, rd = _dev(x), _dev(res)
    outs = []
    try:
        for v in (option, 0):
            _s2_option(v)
            out = torch.full((views, cout, ro, ro), SENTINEL, device=DEV)
            assert _down2(conv, xd, rd, out, _plain(cout, ro, ro), side, 1, views) == OK
            outs.append(out)
    finally:
        hip.lib().poem_set_decode_option(b"s2_staging_wave", 1)
    assert bits_equal(outs[0], outs[1])
    pick = torch.tensor([0, 1, views // 2, views - 2, views - 1])
    ref64, ref32 = (cu.conv3_ref(x[pick], wt, scale, shift, dt, 2, res=res[pick]) for dt in (torch.float64, torch.float32))
    _criterion(outs[0].cpu()[pick], ref64, ref32, f"conv3x3_down2 at {views} views, {tiles} tiles on {blocks} blocks")


@pytest.mark.parametrize("cin,cout,h,w", cu.DOWN2_REFUSED)
def test_conv3x3_down2_refusals(cin, cout, h, w):
    conv = _Conv3(torch.zeros(cout, 16, 3, 3), torch.ones(cout), torch.zeros(cout))
    x = torch.zeros(1, 40, 64, 64, device=DEV)
    out = torch.full((1, cout, 32, 32), SENTINEL, device=DEV)
    for s in (1, 0):
        with options(s2_staging_wave=s):
            assert route("down2", cin, cout, h, w, s2_staging_wave=s) is None
            rc = hip.lib().poem_conv3x3_down2(hip.ptr(x), conv.packed.data_ptr(), hip.ptr(conv.scale), hip.ptr(conv.shift), None, out.data_ptr(),
                                              1, cin, cout, h, w, 1, *_plain(cout, h // 2, w // 2), hip.stream())
            assert rc == REFUSED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- poem_conv1x1_upsample2 -------------------------------------------------------------------------------------------------------
def _up2(x, wp, bias, out, k, c, views=VIEWS):
    return hip.lib().poem_conv1x1_upsample2(hip.ptr(x), wp.data_ptr(), hip.ptr(bias), out.data_ptr(), views, k, c, 8, 8, hip.stream())


@pytest.mark.parametrize("k,c,taken", cu.UP2_CASES)
def test_conv1x1_upsample2(k, c, taken):
    assert (route("up2", k, c, 8, 8) is not None) == taken
    g = torch.Generator().manual_seed(k + c)
    for integers in (False, True):
        if integers:         # the input in multiples of 16: the interpolation of the exact 1x1 result stays exact
            x = 16.0 * torch.randint(-3, 4, (VIEWS, k, 8, 8), generator=g).float()
            wt, bias = torch.randint(-2, 3, (c, k), generator=g).float(), 16.0 * torch.randint(-5, 6, (c,), generator=g).float()
        else:
            x, wt, bias = torch.randn(VIEWS, k, 8, 8, generator=g), torch.randn(c, k, generator=g) / k ** 0.5, 0.1 * torch.randn(c, generator=g)
        xd, wd, bd = _dev(x), _dev(wt), _dev(bias)
        wp = hip.pack_linear(wd)
        for b_host, b_dev in ((bias, bd), (None, None)):
            out = torch.full((VIEWS, c, 16, 16), SENTINEL, device=DEV)
            rc = _up2(xd, wp, b_dev, out, k, c)
            assert rc == (OK if taken else REFUSED)
            if not taken:
                torch.cuda.synchronize()
                assert bool((out == SENTINEL).all()), "a refused call wrote"
                continue
            _check(out, cu.up2_ref(x, wt, b_host, torch.float64), cu.up2_ref(x, wt, b_host, torch.float32), integers,
                   f"conv1x1_upsample2 {k}->{c} bias={b_host is not None}")
    assert route("up2", 40, 160, 16, 16) is None
    assert hip.lib().poem_conv1x1_upsample2(hip.ptr(xd), wp.data_ptr(), None, out.data_ptr(), 1, k, c, 16, 16, hip.stream()) == REFUSED


# ---- NaN and Inf in the input -------------------------------------------------------------------------------------------------------
def _check_poison(run, cpu32, clean_in, variant, what):
    """``run(t)`` -> list of device outputs that must agree in bits (the first is the form under test), ``cpu32(t)`` -> the fp32
    restatement.  See the module docstring for the rule."""
    clean, bad_in = run(clean_in), cu.poison(clean_in, variant)
    bad, ref_clean, ref_bad = run(bad_in), cpu32(clean_in), cpu32(bad_in)
    got = bad[0].cpu()
    reached = ~(ref_bad == ref_clean)
    print(f"{what} {variant}: {int((~torch.isfinite(ref_bad)).sum())} non-finite, {int(reached.sum())} reached of {reached.numel()}")
    assert bool(reached.any()) and not bool(reached.all()) and bool(torch.isfinite(ref_clean).all())
    assert torch.equal(~torch.isfinite(got), ~torch.isfinite(ref_bad)), f"{what} {variant}: non-finite mask"
    assert torch.equal(got.isnan(), ref_bad.isnan()), f"{what} {variant}: NaN mask"
    assert torch.equal(_bits(got)[~reached], _bits(clean[0])[~reached]), f"{what} {variant}: an output the pixel does not reach changed"
    left = reached & torch.isfinite(ref_bad)
    assert torch.allclose(got[left], ref_bad[left], rtol=1e-4, atol=1e-5)
    for k, (o, c) in enumerate(zip(bad[1:], clean[1:])):
        assert bits_equal(o, bad[0]) and bits_equal(c, clean[0]), f"{what} {variant}: form {k + 1} differs in bits"


def _nf_conv3(cin, cout, h, w, stride, res_pre):
    g = torch.Generator().manual_seed(cin + cout + h + w)
    ho, wo = h // stride, w // stride
    x, wt, scale, shift, res = cu.conv_data(g, VIEWS, cin, cout, h, w, False, ho, wo)
    conv, rd = _Conv3(wt, scale, shift), res.to(DEV)

    def run(t):
        xp = F.pad(t, (1, 1, 1, 1)).to(DEV).contiguous()
        outs = [torch.empty(VIEWS, cout, ho, wo, device=DEV) for _ in range(2)]
        assert conv.ex(xp, h, w, stride, rd, _plain(cout, ho, wo), res_pre, outs[0], _plain(cout, ho, wo)) == OK
        if res_pre:
            return outs[:1]
        assert conv.old(xp, h, w, stride, rd, outs[1], _plain(cout, ho, wo)) == OK
        return outs
    return run, (lambda t: cu.conv3_ref(t, wt, scale, shift, torch.float32, stride, 1, res, res_pre)), x


def _nf_upcat(ca, cb, cout, h, w, alts):
    g = torch.Generator().manual_seed(ca + cb + cout + h + w)
    a, b = cu.upcat_data(g, VIEWS, ca, cb, h, w, False)
    _, wt, scale, shift, _ = cu.conv_data(g, 1, ca + cb, cout, 2, 2, False)
    conv, bd = _Conv3(wt, scale, shift), _dev(b)

    def run(t):
        td, outs = _dev(t), []
        for kw in [{}] + alts:
            with options(**kw):
                out = torch.empty(VIEWS, cout, h, w, device=DEV)
                assert _upcat(conv, td, ca, bd, cb, h, w, out, _plain(cout, h, w)) == OK
                outs.append(out)
        return outs + [_two_launch(conv, td, ca, bd, cb, h, w)]
    return run, (lambda t: cu.conv3_ref(cu.upcat_ref(t, b, torch.float32), wt, scale, shift, torch.float32)), a


def _nf_pool_head(ca, cb, cout, j, h):
    w = 64
    g = torch.Generator().manual_seed(ca + cb + cout + j + h)
    a, b = cu.upcat_data(g, VIEWS, ca, cb, h, w, False)
    _, wt, scale, shift, _ = cu.conv_data(g, 1, ca + cb, cout, 2, 2, False)
    hw, hb = _head_data(g, j, cout, False)
    conv, bd, hwd, hbd = _Conv3(wt, scale, shift), _dev(b), _dev(hw), _dev(hb)

    def run(t):
        td = _dev(t)
        one, two = (torch.empty(VIEWS, j, h // 2, w // 2, device=DEV) for _ in range(2))
        assert _pool_head(conv, td, ca, bd, cb, hwd, hbd, one, j, h, w) == OK
        y = torch.empty(VIEWS, cout, h, w, device=DEV)
        assert _upcat(conv, td, ca, bd, cb, h, w, y, _plain(cout, h, w)) == OK
        assert _pool(y, hwd, hbd, two, cout, j, h, w) == OK
        return [one, two]

    def cpu32(t):
        return cu.head_ref(cu.conv3_ref(cu.upcat_ref(t, b, torch.float32), wt, scale, shift, torch.float32), hw, hb, torch.float32)
    return run, cpu32, a


def _nf_pool(c, j, h, w):
    g = torch.Generator().manual_seed(c + j + h + w)
    y = torch.randn(VIEWS, c, h, w, generator=g)
    hw, hb = _head_data(g, j, c, False)
    hwd, hbd = _dev(hw), _dev(hb)

    def run(t):
        td, out = _dev(t), torch.empty(VIEWS, j, h // 2, w // 2, device=DEV)
        assert _pool(td, hwd, hbd, out, c, j, h, w) == OK
        return [out]
    return run, (lambda t: cu.head_ref(t, hw, hb, torch.float32)), y


def _nf_down2(cin, cout, side):
    g = torch.Generator().manual_seed(cin + cout + side)
    ro = side // 2
    x, wt, scale, shift, res = cu.conv_data(g, VIEWS, cin, cout, side, side, False, ro, ro)
    conv, rd = _Conv3(wt, scale, shift), _dev(res)

    def run(t):
        td, outs = _dev(t), []
        try:
            for v in (1, 0):
                _s2_option(v)
                out = torch.empty(VIEWS, cout, ro, ro, device=DEV)
                assert _down2(conv, td, rd, out, _plain(cout, ro, ro), side, 1, VIEWS) == OK
                outs.append(out)
        finally:
            hip.lib().poem_set_decode_option(b"s2_staging_wave", 1)
        return outs
    return run, (lambda t: cu.conv3_ref(t, wt, scale, shift, torch.float32, 2, 1, res)), x


def _nf_up2(k, c):
    g = torch.Generator().manual_seed(k + c)
    x, wt, bias = torch.randn(VIEWS, k, 8, 8, generator=g), torch.randn(c, k, generator=g) / k ** 0.5, 0.1 * torch.randn(c, generator=g)
    wt = torch.where(wt == 0, torch.full_like(wt, 0.01), wt)
    wd, bd = _dev(wt), _dev(bias)
    wp = hip.pack_linear(wd)

    def run(t):
        td, out = _dev(t), torch.empty(VIEWS, c, 16, 16, device=DEV)
        assert _up2(td, wp, bd, out, k, c) == OK
        return [out]
    return run, (lambda t: cu.up2_ref(t, wt, bias, torch.float32)), x


NON_FINITE_FAMILIES = {  # name: (route arguments, the form they must name, the case)
    "direct": (("conv3", 16, 40, 16, 8, 1, True), ("direct", 2, 2, True), lambda: _nf_conv3(16, 40, 16, 8, 1, 0)),     # and its plain twin
    "direct-ex-res-pre": (("conv3", 16, 40, 12, 8, 1, True), ("direct", 2, 1, True), lambda: _nf_conv3(16, 40, 12, 8, 1, 1)),
    "direct-stride2": (("conv3", 16, 40, 16, 16, 2, True), ("direct", 2, 2, True), lambda: _nf_conv3(16, 40, 16, 16, 2, 0)),
    "lds": (("conv3", 16, 64, 32, 16, 1, True), ("lds", 2, False, False, True), lambda: _nf_conv3(16, 64, 32, 16, 1, 0)),
    "lds16": (("conv3", 16, 40, 32, 16, 1, True), ("lds16", 3, False, 0, False, True), lambda: _nf_conv3(16, 40, 32, 16, 1, 0)),
    # Conv3Stager<true> in the compiler-scheduled, the pinned and the 16-row kernel; the two row stagers against it
    "upcat-lds-stager": (("upcat", (16, 8), 64, 32, 16), ("lds", 2, True, False, False), lambda: _nf_upcat(16, 8, 64, 32, 16, [])),
    "upcat-lds-pin": (("upcat", (16, 8), 160, 32, 16), ("lds", 5, True, True, False), lambda: _nf_upcat(16, 8, 160, 32, 16, [dict(pin32=0)])),
    "upcat-lds16-stager": (("upcat", (16, 8), 40, 32, 16), ("lds16", 3, True, 0, False, False), lambda: _nf_upcat(16, 8, 40, 32, 16, [])),
    "upcat-rows64": (("upcat", (16, 8), 40, 12, 64), ("lds16", 3, True, 64, False, False),
                     lambda: _nf_upcat(16, 8, 40, 12, 64, [dict(row_stager=0)])),
    "upcat-rows32": (("upcat", (16, 8), 80, 24, 32), ("lds16", 5, True, 32, False, False),
                     lambda: _nf_upcat(16, 8, 80, 24, 32, [dict(row_stager=0)])),
    "pool-head-fused": (("pool_head", (16, 8), 40, 12, 64, 1, False, 21), ("lds16", 3, True, 64, True, False),
                        lambda: _nf_pool_head(16, 8, 40, 21, 12)),
    "pool-head": (("pool", 40, 0, 6, 10, 1, False, 21), ("pool_head",), lambda: _nf_pool(40, 21, 6, 10)),
    "down2-64": (("down2", 16, 80, 64, 64), ("s2p", 4, 1, 18, 4), lambda: _nf_down2(16, 80, 64)),                        # and conv3x3_s2_kernel
    "down2-16": (("down2", 16, 320, 16, 16), ("s2p", 1, 4, 5, 4), lambda: _nf_down2(16, 320, 16)),
    "conv1x1-up2": (("up2", 40, 160, 8, 8), ("conv1x1_up2", 10), lambda: _nf_up2(40, 160)),
}


@pytest.mark.parametrize("variant", cu.POISONS)
@pytest.mark.parametrize("family", sorted(NON_FINITE_FAMILIES))
def test_non_finite_inputs(family, variant):
    args, form, case = NON_FINITE_FAMILIES[family]
    assert route(*args) == form
    run, cpu32, clean_in = case()
    _check_poison(run, cpu32, clean_in, variant, family)


# ---- the decoders ---------------------------------------------------------------------------------------------------------------------
def _poisoned_pyramid(feats):
    """one NaN pixel in the finest and one in the coarsest level, both in view 0"""
    feats = [f.clone() for f in feats]
    f0, f3 = feats[0], feats[3]
    f0[0, 3, f0.shape[2] // 3, f0.shape[3] // 2] = float("nan")
    f3[0, 5, 1, f3.shape[3] - 2] = float("nan")
    return feats


def _routes(dec):
    for fused in (True, False):
        dec.fuse_upcat, dec.fuse_pool_head, dec.fuse_feat_in = [fused] * 3, fused, fused
        yield fused
    dec.fuse_upcat, dec.fuse_pool_head, dec.fuse_feat_in = [True] * 3, True, True


@pytest.mark.parametrize("name", ["HRNet", "resnet34"])
def test_decoders_keep_a_nan(name):
    if name == "HRNet":
        sd, feats = do.seeded_decoder_state(3), do.synthetic_mlvl_feats(2, 3)
        feat_ref, uv_ref = do.feat_decode, do.uv_decode
    else:
        sd, feats = pk.weights.seeded_decoder_state_dict(2, backbone=name), ru.synthetic_levels(name, 2, 128, 256, 3)
        feat_ref, uv_ref = ru.feat_decode, ru.uv_decode
    feats = _poisoned_pyramid(feats)
    with torch.no_grad():
        masks = [feat_ref(feats, sd).isnan(), uv_ref(feats, sd).isnan()]
    for m in masks:                                                   # the oracle first: a mask that says something
        assert 0 < int(m.sum()) < m.numel() and not bool(m[1].any()), (int(m.sum()), m.numel())
    dec = pk.decode.FeatureDecoders(sd, DEV, name)
    fd = [f.to(DEV) for f in feats]
    for fused in _routes(dec):
        got = [dec.feat_decode(fd, name).cpu(), dec.uv_decode(fd).cpu()]
        for what, o, m in zip(("feat_decode", "uv_decode"), got, masks):
            assert torch.equal(o.isnan(), m), f"{name} {what} fused={fused}: {int(o.isnan().sum())} NaNs, the oracle has {int(m.sum())}"
            assert bool(torch.isfinite(o[~m]).all())
