"""GPU checks of the 512-row hand-scheduled forward (fa2_fwd_hs_wide_kernel, D = 64).

Four waves of four 32-row chains: a workgroup covers 512 query rows per staged K/V tile
instead of 256 (gen/gen_fwd_hs.py, body4).  FWD_ROWS = 512 forces it onto the small
grids used here.  Shapes, the smallest that reach every edge of the 512-row block:
  (1, 1, 128)   one wave live, three waves entirely past S
  (1, 2, 192)   a wave half past S
  (1, 1, 512)   exactly one block
  (1, 2, 576)   a full block plus a 64-row remainder
  (2, 1, 1088)  two full blocks plus a 64-row remainder
Checked: parity with the oracle at the tolerances of test_gpu_fwd_hs.py (1e-2 fp16, 2e-2
bf16) on U[0,1) and N(0,1) inputs; O and LSE bit for bit those of the 256-row kernel
(per row both loops run the same arithmetic in the same order; no restart fires on
U[0,1) inputs); the per-wave restart; the forced-knob errors; a graph capture.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fa2amd  # noqa: E402
from oracle import fa2_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = {"fp16": 1e-2, "bf16": 2e-2}
SHAPES = [(1, 1, 128, 64), (1, 2, 192, 64), (1, 1, 512, 64), (1, 2, 576, 64), (2, 1, 1088, 64)]
IDS = ["B%d_H%d_S%d_D%d" % s for s in SHAPES]
LOG2E = 1.4426950408889634


def cuda(*xs):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in xs]


def maxerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    fa2amd.lib()


@pytest.fixture(autouse=True)
def _no_overrides():
    fa2amd.tune_set(None)
    yield
    fa2amd.tune_set(None)


def run(q, k, v, precision, rows=512):
    fa2amd.tune_set(None)
    fa2amd.tune_set("FWD_HS", 1)
    fa2amd.tune_set("FWD_ROWS", rows)
    tq, tk, tv = cuda(q, k, v)
    o, lse = fa2amd.forward(tq, tk, tv, precision)
    torch.cuda.synchronize()
    return o.cpu().numpy(), lse.cpu().numpy()


_cache = {}


def case(shape, kind):
    """inputs and the oracle's O, LSE of one shape, computed once"""
    if (shape, kind) not in _cache:
        q, k, v = fo.harness_inputs(*shape) if kind == "uniform" else fo.cli_inputs(*shape, seed=11)
        _cache[(shape, kind)] = (q, k, v) + tuple(fo.attention_forward(q, k, v))
    return _cache[(shape, kind)]


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("kind", ["uniform", "gaussian"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_wide_forward_vs_oracle(shape, kind, precision):
    q, k, v, eo, el = case(shape, kind)
    o, lse = run(q, k, v, precision)
    assert np.isfinite(o).all() and np.isfinite(lse).all()
    assert maxerr(o, eo) < TOL[precision]
    assert maxerr(lse, el) < TOL[precision]


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_wide_forward_is_bitwise_the_256_row_forward(shape, precision):
    q, k, v, _, _ = case(shape, "uniform")
    o5, l5 = run(q, k, v, precision, rows=512)
    o2, l2 = run(q, k, v, precision, rows=256)
    assert np.array_equal(o5.view(np.uint32), o2.view(np.uint32))
    assert np.array_equal(l5.view(np.uint32), l2.view(np.uint32))


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_wide_forward_restart_one_chain(precision):
    """A key late in the head that only rows 160..191 (chain 1 of wave 1) score high on: 9.6
    nats or more over their first tile's row max, past the 2^13 tile-sum guard.  That wave recomputes
    its four chains on the robust path in two passes while the other waves keep their loop
    results; every row holds the tolerance.  The spiked rows' Q component is chosen so that
    its scaled 16-bit image (q log2(e) / 8 = 185/128) is exact: at such scores one bf16
    rounding of it would alone be worth 0.02 in LSE, which says nothing about the kernel."""
    shape = (1, 1, 512, 64)
    q, k, v, _, _ = case(shape, "uniform")
    q, k = q.copy(), k.copy()
    q[:, :, 160:192, 0] = np.float32(185.0 / 128.0) / np.float32(LOG2E / 8.0)
    k[:, :, 450, 0] = 11.0
    eo, el = fo.attention_forward(q, k, v)
    o, lse = run(q, k, v, precision)
    assert np.isfinite(o).all() and np.isfinite(lse).all()
    assert maxerr(o, eo) < TOL[precision]
    assert maxerr(lse, el) < TOL[precision]
    # the spike does leave the loop's range: more than 13 ln 2 above those rows' first-tile max
    s = q[0, 0, 160:192].astype(np.float64) @ k[0, 0].astype(np.float64).T / 8.0
    assert (s[:, 450] - s[:, :64].max(1)).min() > 13 * np.log(2.0) + 0.5


@pytest.mark.parametrize("setup", [dict(shape=(1, 1, 256, 128)), dict(shape=(1, 1, 100, 64)),
                                   dict(shape=(1, 1, 512, 64), knob=("FWD_HS", 0)),
                                   dict(shape=(1, 1, 512, 64), causal=True)],
                         ids=["D128", "S100", "FWD_HS0", "causal"])
def test_wide_forced_where_it_cannot_serve_is_an_error(setup):
    """FWD_ROWS = 512 on a shape or plan that cannot take it is an error at the launch, never
    a silent launch of another plan"""
    fa2amd.tune_set("FWD_ROWS", 512)
    if "knob" in setup:
        fa2amd.tune_set(*setup["knob"])
    q, k, v = cuda(*fo.harness_inputs(*setup["shape"]))
    with pytest.raises(fa2amd.FA2Error):
        fa2amd.forward(q, k, v, "fp16", causal=True) if setup.get("causal") else fa2amd.forward(q, k, v, "fp16")


def test_wide_forward_graph_capture():
    """one forced 512-row forward captured and replayed gives the eager result (no scratch)"""
    q, k, v, _, _ = case((1, 2, 576, 64), "uniform")
    tq, tk, tv = cuda(q, k, v)
    fa2amd.tune_set("FWD_ROWS", 512)
    o, lse = torch.empty_like(tq), torch.empty(1, 2, 576, device=tq.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fa2amd.forward(tq, tk, tv, "fp16", out=o, lse=lse)
        torch.cuda.synchronize()
        ref = (o.clone(), lse.clone())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            fa2amd.forward(tq, tk, tv, "fp16", out=o, lse=lse)
    torch.cuda.current_stream().wait_stream(side)
    o.fill_(float("nan"))
    lse.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o, ref[0]) and torch.equal(lse, ref[1])
