"""The MANO fit (include/poem_hip.h ``poem_mano_fit``) without a device: the fp64 restatement of tests/mano_fit_util.py is checked
against autograd and against the bars tests/test_mano_fit.py puts on the seeded cases (the condition on the INPUTS: a case the
restatement cannot fit would ask the kernels for something the definition does not deliver), and the new surface -- the module,
its argument validation, the two ABI entries -- is there.

Measured here (CPU, fp64): restatement's Jacobian against ``torch.autograd`` through the oracle 6.9e-13 (random pose) and 3.1e-13
(all-zero pose) of max|J|; recovery from the default start in 8 iterations: final cost 3.8e-14 .. 9.9e-14 m^2 (the fp32 rounding
of the targets), fitted mesh within 2.1e-8 m of the target; 2 mm noise: fitted mesh 0.48 .. 0.57 mm (mean per vertex) from the
clean mesh against 3.19 .. 3.24 mm for the noisy target."""
import os
import re

import pytest
import torch

import mano_fit_util as u


def _autograd_jacobian(x):
    f = lambda z: u.model(u.assets(), z[None])[0][0].reshape(-1)          # noqa: E731
    return torch.autograd.functional.jacobian(f, x.double().clone().requires_grad_(True), vectorize=True)


@pytest.mark.parametrize("name", ["random", "all_zero"])
def test_restatement_jacobian_agrees_with_autograd(name):
    x = u.eval_poses()["random"] if name == "random" else torch.zeros(u.NX)
    J, Ja = u.jacobian(u.assets(), x), _autograd_jacobian(x)
    rel = float((J - Ja).abs().max() / Ja.abs().max())
    print(f"{name}: |J_restated - J_autograd| / max|J| = {rel:.3e}")
    assert rel < 1e-7, rel
    if name == "all_zero":            # a joint at exactly zero has the three generators as its derivative: nothing vanishes, nothing is NaN
        assert bool(torch.isfinite(Ja).all()) and float(Ja[:, 3:48].abs().amax(0).min()) > 1e-4


def test_restatement_keeps_the_composed_regression_of_the_table():
    assert u.composed_error() < 1e-16


def test_restatement_meets_the_recovery_bars():
    """tests/test_mano_fit.py: the fitted mesh lies within restatement residual + fp32 rounding of the target; the restatement itself
    has to get down to that rounding, or the case would not test recovery."""
    case, ref = u.recovery_case(), u.recovery_reference()
    for i, r in enumerate(ref):
        resid = float((r["verts"] - case["target"][i].double()).abs().max())
        rounding = float(case["target"][i].abs().max()) * 2.0 ** -24
        print(f"sample {i}: cost {r['cost']:.3e}  accepted {sum(r['accepted'])}  max residual {resid:.3e} m  fp32 rounding {rounding:.3e} m")
        assert resid <= 2 * rounding, (i, resid, rounding)           # (|fp32(t) - t| <= rounding per coordinate)
        assert float(case["x_true"][i, :3].norm()) <= 2.8 + 1e-6
    assert abs(float(case["x_true"][0, :3].norm()) - 2.8) < 1e-5


def test_restatement_meets_the_noise_bars():
    case, ref = u.recovery_case(noise_mm=2.0), u.recovery_reference(noise_mm=2.0)
    for i, r in enumerate(ref):
        fitted = float((r["verts"] - case["clean"][i]).norm(dim=-1).mean())
        noisy = float((case["target"][i].double() - case["clean"][i]).norm(dim=-1).mean())
        print(f"sample {i}: fitted {fitted * 1e3:.3f} mm, noisy target {noisy * 1e3:.3f} mm from the clean mesh")
        assert fitted < 0.25 * noisy, (i, fitted, noisy)


def test_restatement_meets_the_step_and_evaluation_conditions():
    """What the device tests take for granted about their inputs: the accept / reject sequences of ``lm_cases`` (with and without
    the regularisers of the two-step run) and measured evaluation bars below 1e-9 at every point those tests evaluate at."""
    a = u.assets()
    for name, (x0, target) in u.lm_cases().items():
        for reg in ({}, u.REG) if name == "far" else ({},):
            ref = u.lm(a, target, x0=x0, iters=2, **reg)
            assert ref["accepted"] == u.LM_EXPECT[name], (name, reg, ref["accepted"], ref["costs"])
            if not ref["accepted"][1]:            # a rejection must be decisive, not a matter of round-off
                cn = float(u.evaluate(a, ref["xs"][1] + ref["dx"][1], target, **reg)[0])
                assert cn > 1.01 * ref["costs"][1], (cn, ref["costs"])
            for x in (x0.double(), ref["xs"][1]):
                _, bars = u.eval_bars(x, target, **reg)        # (asserts < 1e-9 itself)
                print(name, reg, {k: f"{v:.2e}" for k, v in bars.items()})
    for name, x in u.eval_poses().items():
        for reg in ({}, u.REG) if name == "random" else ({},):
            u.eval_bars(x, u.eval_target(), **reg)
    r = u.lm(a, u.recovery_case()["target"][1], iters=8, shape_reg=1e6)      # the regularised full fit has settled by iteration 6
    print("shape_reg 1e6 costs", r["costs"][5:])
    assert abs(r["costs"][6] - r["costs"][8]) / r["cost"] < 1e-9


def test_restatement_regularisers():
    """a very large shape_reg returns betas near 0; the regularised cost, gradient and matrix carry the stated terms"""
    case = u.recovery_case()
    r = u.lm(u.assets(), case["target"][1], iters=8, shape_reg=1e6)
    assert float(r["x"][48:58].abs().max()) < 1e-3, r["x"][48:58]
    x = u.eval_poses()["random"]
    J = u.jacobian(u.assets(), x)
    c0, g0, H0 = u.evaluate(u.assets(), x, u.eval_target(), jac=J)
    c1, g1, H1 = u.evaluate(u.assets(), x, u.eval_target(), shape_reg=0.5, pose_reg=0.25, jac=J)
    xd = x.double()
    assert abs(float(c1 - c0) - float(0.5 * (xd[48:58] ** 2).sum() + 0.25 * (xd[3:48] ** 2).sum())) < 1e-12
    assert torch.allclose(g1 - g0, u.reg_vector(0.5, 0.25) * xd, atol=1e-12) and torch.allclose(H1 - H0, torch.diag(u.reg_vector(0.5, 0.25)))


# ---- the new surface ----------------------------------------------------------------------------------------------------------------
def test_fit_module_imports_without_a_device():
    import poem_v2_amd as pk
    from poem_v2_amd import fit
    assert pk.fit_mano is fit.fit_mano and pk.ManoFit is fit.ManoFit
    assert fit.ManoFit._fields == ("pose_aa", "betas", "tsl", "verts", "joints", "cost", "accepted", "status")


class _Layer:
    """what fit_mano reads of a ManoLayer"""
    def __init__(self):
        self.th_table = torch.zeros(4)


def test_argument_validation_raises_before_any_launch(monkeypatch):
    import poem_v2_amd as pk
    from poem_v2_amd import fit

    def no_lib():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(pk.hip, "lib", no_lib)
    layer, v = _Layer(), torch.zeros(2, 778, 3)
    bad = [
        (dict(layer=object(), verts=v), TypeError),
        (dict(layer=layer, verts=torch.zeros(2, 777, 3)), ValueError),
        (dict(layer=layer, verts=torch.zeros(778, 3)), ValueError),
        (dict(layer=layer, verts=v.double()), TypeError),
        (dict(layer=layer, verts=v.to("meta")), ValueError),                    # another device than the layer's
        (dict(layer=layer, verts=v, iters=-1), ValueError),
        (dict(layer=layer, verts=v, iters=65), ValueError),
        (dict(layer=layer, verts=v, iters=2.0), ValueError),
        (dict(layer=layer, verts=v, shape_reg=-1.0), ValueError),
        (dict(layer=layer, verts=v, pose_reg=float("nan")), ValueError),
        (dict(layer=layer, verts=v, pose_reg=float("inf")), ValueError),
        (dict(layer=layer, verts=v, init=torch.zeros(2, 60)), ValueError),
        (dict(layer=layer, verts=v, init=torch.zeros(3, 61)), ValueError),
        (dict(layer=layer, verts=v, init=torch.zeros(2, 61, dtype=torch.float64)), TypeError),
    ]
    for kw, exc in bad:
        kw = dict(kw)
        with pytest.raises(exc):
            fit.fit_mano(kw.pop("layer"), kw.pop("verts"), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):              # everything valid, but host tensors
        fit.fit_mano(layer, v)


def test_abi_entries_are_declared_and_bound(repo_root):
    import poem_v2_amd as pk
    header = open(os.path.join(repo_root, "include", "poem_hip.h")).read()
    for name, nargs in (("poem_mano_fit_workspace_bytes", 1), ("poem_mano_fit", 18)):
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/poem_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in pk.hip.SIGNATURES and len(pk.hip.SIGNATURES[name][1]) == nargs
    assert pk.hip.ABI_VERSION == 3                                           # additive: the ABI version stays
