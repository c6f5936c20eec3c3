"""GPU tests of the causal mask (fa2_forward_masked / fa2_backward_masked, fp16 and bf16
tiles) against the float64 closed form of tests/causal_ref.py.

Tolerances are test_gpu_parity.py's: max-abs 1e-2 (fp16 tiles) and 2e-2 (bf16 tiles) on O
and LSE; dQ, dK, dV against that tolerance x max(1, max|ref|).  The shapes cross every
boundary the tile-skipping logic has: a wave (32 rows), a key tile (64), a workgroup (128
rows at D = 128, 256 otherwise), ragged tails, and several workgroups with full tiles below
the diagonal.  The leak tests are bitwise: a masked score is -inf before the exponential,
so what lies across the diagonal cannot move a protected row by even one ulp.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import causal_ref  # noqa: E402
import fa2amd  # noqa: E402
from oracle import fa2_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {"fp16": 1e-2, "bf16": 2e-2}
SHAPES = [(1, 1, 1, 64), (1, 2, 33, 64), (2, 3, 65, 32), (1, 2, 256, 64), (1, 2, 257, 128), (2, 2, 300, 64),
          (1, 1, 640, 128), (1, 2, 777, 32), (1, 1, 1000, 64)]
sid = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fa2amd.lib()


@pytest.fixture(autouse=True)
def _no_overrides():
    """every test starts and ends with the shipped launch plans (fa2_tune_set cleared)"""
    fa2amd.tune_set(None)
    yield
    fa2amd.tune_set(None)


def cuda(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def maxerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def inputs(shape, gaussian=False):
    q, k, v = fo.cli_inputs(*shape, seed=7) if gaussian else fo.harness_inputs(*shape)
    do = np.random.RandomState(43).randn(*shape).astype(np.float32)
    return q, k, v, do


_REF = {}


def reference(shape, gaussian=False):
    """(inputs, O, LSE, dQ, dK, dV) of the float64 reference, computed once per shape"""
    if (shape, gaussian) not in _REF:
        q, k, v, do = inputs(shape, gaussian)
        o, lse = causal_ref.forward(q, k, v, causal=True)
        dq, dk, dv, _ = causal_ref.backward(q, k, v, do, causal=True)
        _REF[(shape, gaussian)] = ((q, k, v, do), o, lse, dq, dk, dv)
    return _REF[(shape, gaussian)]


def run(tq, tk, tv, tdo, precision):
    o, lse = fa2amd.forward(tq, tk, tv, precision, causal=True)
    dq, dk, dv = fa2amd.backward(tq, tk, tv, o, tdo, lse, precision, causal=True)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def check_parity(got, exp, tol, where=""):
    names = ("o", "lse", "dq", "dk", "dv")
    errs = {}
    for n, a, e in zip(names, got, exp):
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        assert np.isfinite(a).all(), (n, where)
        scale = 1.0 if n in ("o", "lse") else max(1.0, float(np.abs(e).max()))
        errs[n] = (maxerr(a, e), tol * scale)
    print(where, {n: "%.2e / %.2e" % v for n, v in errs.items()})
    for n, (err, bound) in errs.items():
        assert err < bound, (n, err, bound, where)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_parity_against_reference(shape, precision):
    (q, k, v, do), *exp = reference(shape)
    got = run(*cuda(q, k, v, do), precision)
    check_parity(got, exp, TOL[precision], f"{sid(shape)} {precision}")


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_parity_against_reference_gaussian(shape, precision):
    """the same shapes and tolerances on N(0,1) Q, K, V (fo.cli_inputs): U[0,1) inputs make P
    nearly uniform, so the mask is otherwise only ever seen through O ~ mean(V)"""
    (q, k, v, do), *exp = reference(shape, gaussian=True)
    got = run(*cuda(q, k, v, do), precision)
    check_parity(got, exp, TOL[precision], f"{sid(shape)} {precision} gaussian")


LEAK_SHAPE = (1, 2, 777, 64)
LEAK_J0 = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 776]


@pytest.fixture(scope="module")
def leak_base():
    out = {}
    for precision in ("fp16", "bf16"):
        t = cuda(*inputs(LEAK_SHAPE))
        out[precision] = (t, run(*t, precision))
    return out


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("j0", LEAK_J0)
def test_no_leak_across_the_diagonal(leak_base, j0, precision):
    """Keys and values from j0 on must not reach rows < j0 of O, LSE and dQ; queries, dO, O
    and LSE before j0 must not reach rows >= j0 of dK and dV: bitwise.  The perturbations
    are finite and modest (|x| <= 8; K scaled by -3 lowers the perturbed scores, so no
    protected row's wave takes another path through the kernel)."""
    (tq, tk, tv, tdo), (o, lse, dq, dk, dv) = leak_base[precision]
    k2, v2 = tk.clone(), tv.clone()
    k2[:, :, j0:] *= -3.0
    v2[:, :, j0:] = 7.0 * v2[:, :, j0:] + 1.0
    o2, lse2, dq2, _, _ = run(tq, k2, v2, tdo, precision)
    assert not torch.equal(o2, o)  # the perturbation does reach the rows from j0 on
    assert torch.equal(o2[:, :, :j0], o[:, :, :j0])
    assert torch.equal(lse2[:, :, :j0], lse[:, :, :j0])
    assert torch.equal(dq2[:, :, :j0], dq[:, :, :j0])
    q3, do3, o3, lse3 = tq.clone(), tdo.clone(), o.clone(), lse.clone()
    q3[:, :, :j0] = 1.0 - q3[:, :, :j0]
    do3[:, :, :j0] *= -2.0
    o3[:, :, :j0] += 1.0
    lse3[:, :, :j0] += 0.5
    dq3, dk3, dv3 = fa2amd.backward(q3, tk, tv, o3, do3, lse3, precision, causal=True)
    torch.cuda.synchronize()
    assert not torch.equal(dk3, dk)
    assert torch.equal(dk3[:, :, j0:], dk[:, :, j0:])
    assert torch.equal(dv3[:, :, j0:], dv[:, :, j0:])


# value of the spiking key's elements (test_gpu_parity.py SPIKE; D = 64 takes 4.0 so that
# EVERY later row clears 13 log2 units, which the test asserts)
SPIKE = {64: 4.0, 128: 3.0}
# unit roundoff of the tile formats (11 and 8 significand bits)
UNIT = {"fp16": 2.0**-11, "bf16": 2.0**-8}


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_restart_under_the_mask(D, precision):
    """One late key (600 of 768) whose score exceeds tile 0's row max by more than 13 log2
    units for the rows after it: their waves restart the block with the rescaling loop,
    which must skip and mask as the common path does; the rows before it never see it.

    O and LSE -- what the restart computes -- are held to the project's tolerance.  The
    gradients are checked on the same inputs, with the bound the tile format gives at
    scores this large: a score of smax log2 units built from two rounded factors is off by
    up to smax * 2u, so P = exp2(s - lse) by the factor 2^(smax * 2u) (about 27 * 2^-10 ->
    1.9 % in fp16, 27 * 2^-7 -> 16 % in bf16; the spiking key's equal elements make the
    rounding systematic over d, so it does not average out).  The project's tolerance
    applies where it is the larger."""
    shape = (1, 1, 768, D)
    q, k, v, do = inputs(shape)
    k = k.copy()
    k[:, :, 600, :] = SPIKE[D]
    s = (q[0, 0].astype(np.float64) @ k[0, 0].astype(np.float64).T) / np.sqrt(D) * np.log2(np.e)
    assert (s[600:, 600] - s[600:, :64].max(-1)).min() > 13.0  # the construction does what it says
    o, lse = causal_ref.forward(q, k, v, causal=True)
    dq, dk, dv, _ = causal_ref.backward(q, k, v, do, causal=True)
    got = run(*cuda(q, k, v, do), precision)
    check_parity(got[:2], (o, lse), TOL[precision], f"restart D={D} {precision}")
    gtol = max(TOL[precision], 2.0 ** (float(np.tril(s).max()) * 2 * UNIT[precision]) - 1.0)
    check_parity(got, (o, lse, dq, dk, dv), gtol, f"restart D={D} {precision} gradients")


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(2, 2, 300, 64), (1, 2, 777, 32)], ids=sid)
def test_deterministic(shape, precision):
    t = cuda(*inputs(shape))
    a, b = run(*t, precision), run(*t, precision)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_full_grid_sampled_heads():
    """B4_H16_S2048_D64: many workgroups per head, the XCD remap and the launch order."""
    shape = (4, 16, 2048, 64)
    q, k, v, do = inputs(shape)
    got = run(*cuda(q, k, v, do), "fp16")
    for b, h in ((0, 0), (2, 8), (3, 15)):
        sl = (slice(b, b + 1), slice(h, h + 1))
        o, lse = causal_ref.forward(q[sl], k[sl], v[sl], causal=True)
        dq, dk, dv, _ = causal_ref.backward(q[sl], k[sl], v[sl], do[sl], causal=True)
        check_parity([x[sl] for x in got], (o, lse, dq, dk, dv), TOL["fp16"], f"head {b},{h}")


FWD_OVERRIDES = [{"FWD_HS": 1}, {"FWD_SPLIT": 2}, {"FWD_KS": 2}, {"FWD_WAVES": 4}, {"FWD_NKB": 1}]
BWD_OVERRIDES = [{"DQ_HS": 1}, {"DKDV_HS": 1}, {"DQ_KS": 2}, {"DQ_WAVES": 4}, {"DKDV_QS": 2}, {"DKDV_WAVES": 4},
                 {"BWD_FUSED": 1}, {"BWD_SPLIT": 2}]
kid = lambda kn: "_".join(f"{a}{b}" for a, b in kn.items())  # noqa: E731


@pytest.mark.parametrize("knobs", FWD_OVERRIDES + BWD_OVERRIDES, ids=kid)
def test_override_the_causal_plan_cannot_honour_is_an_error(knobs):
    shape = (1, 2, 512, 64)
    tq, tk, tv, tdo = cuda(*inputs(shape))
    o, lse = fa2amd.forward(tq, tk, tv, "fp16", causal=True)
    with fa2amd.tuned(**knobs):
        with pytest.raises(fa2amd.FA2Error, match=next(iter(knobs))):
            if knobs in FWD_OVERRIDES:
                fa2amd.forward(tq, tk, tv, "fp16", causal=True)
            else:
                fa2amd.backward(tq, tk, tv, o, tdo, lse, "fp16", causal=True)
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_no_mask_is_the_unmasked_call(precision):
    """causal=False, and FA2_MASK_NONE through the masked entry points, are the calls
    without the argument: same plans, same bits."""
    shape = (2, 2, 300, 64)
    tq, tk, tv, tdo = cuda(*inputs(shape))
    o, lse = fa2amd.forward(tq, tk, tv, precision)
    dq, dk, dv = fa2amd.backward(tq, tk, tv, o, tdo, lse, precision)
    o2, lse2 = fa2amd.forward(tq, tk, tv, precision, causal=False)
    g2 = fa2amd.backward(tq, tk, tv, o, tdo, lse, precision, causal=False)
    B, H, S, D = shape
    L, P = fa2amd.lib(), fa2amd._PRECISION[precision]
    o3, lse3, dl3 = torch.empty_like(o), torch.empty_like(lse), torch.empty_like(lse)
    g3 = [torch.empty_like(tq) for _ in range(3)]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda *ts: [t.data_ptr() for t in ts]  # noqa: E731
    assert L.fa2_forward_masked(*p(tq, tk, tv, o3, lse3), B, H, S, D, P, fa2amd.FA2_MASK_NONE, st) == 0
    assert L.fa2_backward_masked(*p(tq, tk, tv, o, tdo, lse, dl3, *g3), B, H, S, D, P, fa2amd.FA2_MASK_NONE, st) == 0
    torch.cuda.synchronize()
    for a, b in zip((o, lse, dq, dk, dv) * 2, (o2, lse2, *g2, o3, lse3, *g3)):
        assert torch.equal(a, b)
    if precision == "fp32":
        with pytest.raises(fa2amd.FA2Error, match="fp16"):
            fa2amd.forward(tq, tk, tv, precision, causal=True)


@pytest.mark.parametrize("shape,precision", [((2, 4, 512, 64), "fp16"), ((1, 2, 300, 128), "bf16")])
def test_graph_capture_replay(shape, precision):
    """causal fwd + bwd captured into a torch.cuda.CUDAGraph replay to the eager bits (the
    causal plans take no scratch, so the capture needs nothing from an earlier call)"""
    B, H, S, D = shape
    tq, tk, tv, tdo = cuda(*inputs(shape))
    o, lse = torch.empty_like(tq), torch.empty(B, H, S, device=tq.device)
    dq, dk, dv = torch.empty_like(tq), torch.empty_like(tq), torch.empty_like(tq)
    dl = torch.empty(B, H, S, device=tq.device)

    def step():
        fa2amd.forward(tq, tk, tv, precision, out=o, lse=lse, causal=True)
        fa2amd.backward(tq, tk, tv, o, tdo, lse, precision, dq=dq, dk=dk, dv=dv, delta_buf=dl, causal=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # eager, on the stream the graph is captured on
        torch.cuda.synchronize()
        eager = [t.clone() for t in (o, lse, dq, dk, dv)]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t in (o, lse, dq, dk, dv):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), eager, (o, lse, dq, dk, dv)):
            assert torch.equal(a, b), name
