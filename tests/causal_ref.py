"""Float64 closed form of attention forward and backward with an optional causal
(lower-triangular) mask: the reference of tests/test_causal_cpu.py and
tests/test_gpu_causal.py.

    S = Q Kᵀ / √D   (masked entries -inf: key j > query i)
    LSE = ln Σ_j exp(S),  P = exp(S - LSE),  O = P V
    Δ = rowsum(dO ∘ O),  dV = Pᵀ dO,  dS = P ∘ (dO Vᵀ - Δ) / √D,  dQ = dS K,  dK = dSᵀ Q

With ``causal=False`` it is what ``oracle.fa2_oracle`` computes (tied to it within 1e-6 by
test_causal_cpu.py).  Everything is returned in float64.
"""
import numpy as np


def _probs(q, k, causal):
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    S, D = q.shape[-2], q.shape[-1]
    s = np.matmul(q, np.swapaxes(k, -1, -2)) / np.sqrt(D)
    if causal:
        s = np.where(np.tril(np.ones((S, S), bool)), s, -np.inf)
    m = s.max(-1, keepdims=True)  # finite: key 0 is never masked
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    return e / l, (m + np.log(l))[..., 0]


def forward(q, k, v, causal=False):
    """(O, LSE) in float64; LSE is the natural log of the sum over the allowed keys."""
    p, lse = _probs(q, k, causal)
    return np.matmul(p, np.asarray(v, np.float64)), lse


def backward(q, k, v, do, causal=False):
    """(dQ, dK, dV, Δ) in float64."""
    q64, k64, v64, do64 = (np.asarray(x, np.float64) for x in (q, k, v, do))
    D = q64.shape[-1]
    p, _ = _probs(q, k, causal)
    o = np.matmul(p, v64)
    delta = (do64 * o).sum(-1)
    dv = np.matmul(np.swapaxes(p, -1, -2), do64)
    ds = p * (np.matmul(do64, np.swapaxes(v64, -1, -2)) - delta[..., None]) / np.sqrt(D)
    return np.matmul(ds, k64), np.matmul(np.swapaxes(ds, -1, -2), q64), dv, delta
