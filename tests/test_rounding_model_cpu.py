"""CPU proof that the error budget of tests/test_gpu_error_budget.py sees what the absolute
1e-2 / 2e-2 rule does not.

1. With rounding disabled the model of tests/rounding_model.py is the closed form of
   tests/causal_ref.py (masked and unmasked) to 1e-12, so `model - exact` is rounding only.
2. The defect table: each deliberate defect is applied to the exact float64 closed form (not
   to any kernel) at the shapes and inputs of the GPU budget cases, and the budget check --
   rounding_model.violations with rounding_model.M_RMS / M_MAX, the very function and
   constants the GPU test asserts with -- must reject it on at least one tensor.  A margin
   widened on the GPU side until a defect slips through fails here.
3. Every case's id ends in `old_accepts` or `old_rejects`: whether the previous rule (max-abs
   below 1e-3 / 1e-2 / 2e-2 for fp32 / fp16 / bf16 tiles on O and LSE, gradients against
   that x max(1, max|ref|)) accepted the same defect; the test asserts the record.

Where a defect is listed (`applies`):
  * swapped V rows need keys 40 and 41 (S >= 42); the excluded diagonal needs the mask.
  * dK's zeroed last row is listed without the mask only: under it the last key is seen by
    the last query alone, with weight ~1/S, so that row of dK is itself of the size of the
    rounding error of the other rows and no tolerance can tell it from zero.
  * Δ from a 16-bit-rounded O is one more rounding of the size of those the fp16 / bf16
    model already holds (O feeds Δ, which is subtracted from a dP that was itself computed
    from 16-bit dO and V): inside that budget by construction.  It is a defect of the
    exact-fp32 path, whose budget it exceeds, and is listed there.
  * On U[0,1) inputs P is nearly uniform, so swapping two V rows moves O and dV only by
    (P_i40 - P_i41)(v41 - v40), second order in the spread of the scores: with bf16 tiles
    and no mask that is at the model's own error from S = 257 on, and so it is for the
    hand-scheduled forward's models ("fp16_hs", "bf16_hs": listed without the mask at the
    whole-tile shapes that forward serves, for the defects a forward can have).  Those
    cases are left to the N(0,1) inputs of the same shape, which reject every defect.
"""
import numpy as np
import pytest

import causal_ref
import rounding_model as rm

OLD_TOL = {"fp32": 1e-3, "fp16": 1e-2, "bf16": 2e-2}
HS_SHAPES = [s for s in rm.SHAPES if s[2] in (576, 640, 1024)]
sid = lambda s: "x".join(map(str, s))  # noqa: E731


def applies(defect, shape, kind, causal, tiles):
    S = shape[2]
    if tiles == "fp32" and causal:
        return False  # the exact-fp32 path has no mask
    if tiles.endswith("_hs"):  # the hand-scheduled forward: whole 64-key tiles, no mask; its budget cases
        if causal or shape not in HS_SHAPES or defect in ("dq_zero", "dk_last_row_zero", "delta_rounded_o"):
            return False
        if defect == "swap_v" and kind == "uniform":
            return False  # as below; the packed fp16 row sum makes O's own error 4x larger still
        tiles = tiles[:4]
    if defect == "swap_v":
        return S >= 42 and not (kind == "uniform" and tiles == "bf16" and not causal and S >= 257)
    if defect == "diag_excluded":
        return causal
    if defect == "dk_last_row_zero":
        return not causal
    if defect == "delta_rounded_o":
        return tiles == "fp32"
    return True


# {(defect, kind, causal, tiles): the S of the shapes at which the old absolute rule accepted it}
_OLD = {
    ('delta_rounded_o', 'gaussian', False, 'fp32'): (33, 65, 257, 300, 576, 777, 640, 1000, 1024),
    ('delta_rounded_o', 'uniform', False, 'fp32'): (33, 65, 257, 300, 576, 777, 640, 1000, 1024),
    ('dk_last_row_zero', 'uniform', False, 'bf16'): (576, 777, 640, 1000, 1024),
    ('dk_last_row_zero', 'uniform', False, 'fp16'): (576, 640),
    ('dq_zero', 'uniform', False, 'bf16'): (576, 777, 640, 1000, 1024),
    ('drop_key', 'uniform', True, 'bf16'): (777, 1000, 1024),
    ('scale', 'gaussian', False, 'bf16'): (33, 65, 257, 576, 777, 640, 1000, 1024),
    ('scale', 'gaussian', False, 'bf16_hs'): (576, 640, 1024),
    ('scale', 'gaussian', True, 'bf16'): (33, 576, 777, 640, 1000),
    ('scale', 'uniform', False, 'bf16'): (33, 65, 300, 576, 777, 1000, 1024),
    ('scale', 'uniform', False, 'bf16_hs'): (576, 1024),
    ('scale', 'uniform', True, 'bf16'): (33, 65, 300, 576, 777, 1000, 1024),
    ('swap_v', 'uniform', False, 'bf16'): (65,),
    ('swap_v', 'uniform', False, 'fp16'): (65, 257, 300, 576, 777, 640, 1000, 1024),
    ('swap_v', 'uniform', False, 'fp32'): (576, 777, 640, 1000, 1024),
}
OLD_RULE_ACCEPTED = {(d, s, kind, c, t) for (d, kind, c, t), ss in _OLD.items() for s in rm.SHAPES if s[2] in ss}


def _cases():
    out = []
    for defect in rm.DEFECTS:
        for shape in rm.SHAPES:
            for kind in rm.KINDS:
                for causal in (False, True):
                    for tiles in rm.TILES:
                        if applies(defect, shape, kind, causal, tiles):
                            old = (defect, shape, kind, causal, tiles) in OLD_RULE_ACCEPTED
                            out.append(pytest.param(defect, shape, kind, causal, tiles, old, id="%s-%s-%s-%s-%s-%s" % (
                                defect, sid(shape), kind, "causal" if causal else "full", tiles,
                                "old_accepts" if old else "old_rejects")))
    return out


_CACHE = {}


def exact_and_model(shape, kind, causal, tiles):
    """(inputs, exact, model errors), each computed once"""
    if (shape, kind) not in _CACHE:
        _CACHE[(shape, kind)] = rm.inputs(shape, kind)
    x = _CACHE[(shape, kind)]
    if (shape, kind, causal) not in _CACHE:
        _CACHE[(shape, kind, causal)] = rm.attention(*x, causal=causal)
    exact = _CACHE[(shape, kind, causal)]
    if (shape, kind, causal, tiles) not in _CACHE:
        _CACHE[(shape, kind, causal, tiles)] = rm.errors(rm.attention(*x, causal=causal, tiles=tiles), exact)
    return x, exact, _CACHE[(shape, kind, causal, tiles)]


def old_rule_accepts(got, exact, tiles):
    for n in rm.TENSORS:
        scale = 1.0 if n in ("o", "lse") else max(1.0, float(np.abs(exact[n]).max()))
        if not float(np.abs(got[n] - exact[n]).max()) < OLD_TOL[tiles[:4]] * scale:
            return False
    return True


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("kind", rm.KINDS)
@pytest.mark.parametrize("shape", [(1, 1, 1, 64), (2, 3, 65, 32), (1, 2, 257, 128), (2, 2, 300, 64)], ids=sid)
def test_unrounded_model_is_the_closed_form(shape, kind, causal):
    q, k, v, do = rm.inputs(shape, kind)
    got = rm.attention(q, k, v, do, causal=causal)
    o, lse = causal_ref.forward(q, k, v, causal=causal)
    dq, dk, dv, delta = causal_ref.backward(q, k, v, do, causal=causal)
    for n, e in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv), ("delta", delta)):
        assert float(np.abs(got[n] - e).max()) <= 1e-12, n


def test_rounding_functions():
    """fp16 / bf16 images: exact values stay, ties go to even, the unit roundoffs are 2^-11 / 2^-8"""
    x = np.array([1.0, -0.5, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])
    assert rm.round_bf16(x).tolist() == [1.0, -0.5, 1.0, 1.0 + 2.0 ** -6, 1.0, 1.0]
    assert rm.round_fp16(x).tolist() == [1.0, -0.5, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0, 1.0 + 2.0 ** -9]
    r = np.random.RandomState(0).randn(4096)
    assert 2.0 ** -10 < np.abs(rm.round_bf16(r) / r - 1).max() <= 2.0 ** -8
    assert 2.0 ** -13 < np.abs(rm.round_fp16(r) / r - 1).max() <= 2.0 ** -11


def test_errors_statistics():
    exact = {"o": np.array([[[[3.0, -4.0], [0.0, 0.0]]]]), "lse": np.array([[[2.0, 4.0]]])}
    got = {"o": exact["o"] + np.array([[[[0.0, 0.4], [0.0, 0.0]]]]), "lse": exact["lse"] + np.array([[[0.0, -0.5]]])}
    e = rm.errors(got, exact)
    assert e["o"]["relmax"].shape == (1, 1) and np.isclose(e["o"]["relmax"][0, 0], 0.1)
    assert np.isclose(e["o"]["relrms"][0, 0], 0.2 / 2.5)
    assert np.isclose(e["lse"]["relmax"][0, 0], 0.5) and np.isclose(e["lse"]["relrms"][0, 0], 0.5 / np.sqrt(2.0))
    # a NaN is a violation, never a pass
    got["o"][0, 0, 0, 0] = np.nan
    assert rm.violations(rm.errors(got, exact), {n: {s: v + 1.0 for s, v in d.items()} for n, d in e.items()}, "fp16")


@pytest.mark.parametrize("tiles", rm.TILES)
def test_the_model_passes_its_own_budget(tiles):
    """margins >= 1: a kernel that is exactly the model passes"""
    assert rm.M_RMS[tiles[:4]] >= 1.0 and rm.M_MAX[tiles[:4]] >= 1.0
    _, _, merr = exact_and_model((1, 2, 576, 64), "gaussian", False, tiles)
    assert rm.violations(merr, merr, tiles) == []


@pytest.mark.parametrize("defect,shape,kind,causal,tiles,old_accepted", _cases())
def test_budget_rejects_defect(defect, shape, kind, causal, tiles, old_accepted):
    x, exact, merr = exact_and_model(shape, kind, causal, tiles)
    got = rm.attention(*x, causal=causal, defect=defect)
    bad = rm.violations(rm.errors(got, exact), merr, tiles)
    assert bad, "the budget accepts this defect"
    assert old_rule_accepts(got, exact, tiles) == old_accepted


@pytest.mark.parametrize("defect", rm.DEFECTS)
def test_every_defect_has_gaussian_cases_at_every_shape_it_can_touch(defect):
    """every defect is rejected by the N(0,1) case of each shape (swapped V rows: S >= 42)"""
    listed = {p.values[1] for p in _cases() if p.values[0] == defect and p.values[2] == "gaussian"}
    assert listed == {s for s in rm.SHAPES if defect != "swap_v" or s[2] >= 42}
