"""CPU-only checks of the causal mask: the float64 reference of the GPU tests
(tests/causal_ref.py) is tied to the pinned oracle, behaves as a causal mask must, and
the two masked entry points of the C ABI exist and validate their arguments before any
HIP call.  No compute call touches a device here."""
import ctypes
import os
import re

import numpy as np
import pytest

import causal_ref
import fa2amd
from oracle import fa2_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fa2_amd.h")
SHAPES = [(1, 2, 33, 64), (2, 2, 300, 64), (1, 1, 777, 32)]


def _inputs(shape):
    q, k, v = fo.harness_inputs(*shape)
    do = np.random.RandomState(43).randn(*shape).astype(np.float32)
    return q, k, v, do


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_without_mask_is_the_oracle(shape):
    q, k, v, do = _inputs(shape)
    eo, el = fo.attention_forward(q, k, v)
    edq, edk, edv, edl = fo.attention_backward(q, k, v, do)
    o, lse = causal_ref.forward(q, k, v, causal=False)
    dq, dk, dv, dl = causal_ref.backward(q, k, v, do, causal=False)
    for got, exp in ((o, eo), (lse, el), (dq, edq), (dk, edk), (dv, edv), (dl, edl)):
        assert got.shape == exp.shape
        assert np.abs(got - exp.astype(np.float64)).max() < 1e-6


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_causal_properties(shape):
    q, k, v, do = _inputs(shape)
    D = shape[-1]
    o, lse = causal_ref.forward(q, k, v, causal=True)
    # row 0 attends key 0 alone
    assert np.abs(o[:, :, 0] - v[:, :, 0]).max() < 1e-12
    assert np.abs(lse[:, :, 0] - (q[:, :, 0].astype(np.float64) * k[:, :, 0]).sum(-1) / np.sqrt(D)).max() < 1e-12
    # the last row attends every key: it is the unmasked last row
    fo_, fl = causal_ref.forward(q, k, v, causal=False)
    assert np.abs(o[:, :, -1] - fo_[:, :, -1]).max() < 1e-12 and np.abs(lse[:, :, -1] - fl[:, :, -1]).max() < 1e-12
    # nothing leaks across the diagonal: keys and values from j0 on do not reach rows < j0,
    # queries and dO before j0 do not reach dK / dV rows >= j0
    j0 = shape[2] // 2
    k2, v2 = k.copy(), v.copy()
    k2[:, :, j0:] *= -3.0
    v2[:, :, j0:] = 7.0 * v2[:, :, j0:] + 1.0
    o2, lse2 = causal_ref.forward(q, k2, v2, causal=True)
    assert np.array_equal(o2[:, :, :j0], o[:, :, :j0]) and np.array_equal(lse2[:, :, :j0], lse[:, :, :j0])
    dq, dk, dv, _ = causal_ref.backward(q, k, v, do, causal=True)
    dq2 = causal_ref.backward(q, k2, v2, do, causal=True)[0]
    assert np.array_equal(dq2[:, :, :j0], dq[:, :, :j0])
    q3, do3 = q.copy(), do.copy()
    q3[:, :, :j0] = 1.0 - q3[:, :, :j0]
    do3[:, :, :j0] *= -2.0
    _, dk3, dv3, _ = causal_ref.backward(q3, k, v, do3, causal=True)
    assert np.array_equal(dk3[:, :, j0:], dk[:, :, j0:]) and np.array_equal(dv3[:, :, j0:], dv[:, :, j0:])
    # without the mask the same perturbation does move the protected rows
    assert np.abs(causal_ref.forward(q, k2, v2)[0][:, :, :j0] - fo_[:, :, :j0]).max() > 1e-2


def test_header_declares_and_library_exports_masked_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = fa2amd.lib()
    for name in ("fa2_forward_masked", "fa2_backward_masked"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert name in fa2amd.C_SYMBOLS
    assert re.search(r"FA2_MASK_NONE\s*=\s*0\b", text) and re.search(r"FA2_MASK_CAUSAL\s*=\s*1\b", text)
    assert (fa2amd.FA2_MASK_NONE, fa2amd.FA2_MASK_CAUSAL) == (0, 1)


def test_masked_entry_points_validate_without_device():
    L = fa2amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    fwd = lambda prec, mask, o=one: L.fa2_forward_masked(one, one, one, o, one, 1, 1, 8, 64, prec, mask, null)
    bwd = lambda prec, mask, dk=one: L.fa2_backward_masked(one, one, one, one, one, one, one, one, dk, one, 1, 1, 8, 64,
                                                         prec, mask, null)
    for call in (fwd, bwd):
        # a mask value outside the enum
        assert call(fa2amd.FA2_FP16, 2) == -1 and b"mask" in L.fa2_last_error()
        assert call(fa2amd.FA2_BF16, -1) == -1 and b"mask" in L.fa2_last_error()
        # exact-fp32 tiles have no causal kernels: the message names the two that do
        assert call(fa2amd.FA2_FP32, fa2amd.FA2_MASK_CAUSAL) == -1
        msg = L.fa2_last_error()
        assert b"fp16" in msg and b"bf16" in msg
        # null pointers, with and without a mask
        assert call(fa2amd.FA2_FP16, fa2amd.FA2_MASK_CAUSAL, null) == -1 and b"null" in L.fa2_last_error()
        assert call(fa2amd.FA2_FP16, fa2amd.FA2_MASK_NONE, null) == -1 and b"null" in L.fa2_last_error()
        # a bad precision is still reported as such
        assert call(7, fa2amd.FA2_MASK_CAUSAL) == -1 and b"precision" in L.fa2_last_error()
    rc = L.fa2_forward_masked(one, one, one, one, one, 1, 1, 8, 48, fa2amd.FA2_FP16, fa2amd.FA2_MASK_CAUSAL, null)
    assert rc == -1 and b"head_dim" in L.fa2_last_error()


def test_python_causal_argument_refuses_cpu_tensors():
    import torch
    q = torch.zeros(1, 1, 8, 64)
    with pytest.raises(fa2amd.FA2Error):
        fa2amd.forward(q, q, q, causal=True)
