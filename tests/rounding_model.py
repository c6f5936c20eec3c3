"""Rounding model of the attention kernels: the yardstick of tests/test_gpu_error_budget.py
and tests/test_rounding_model_cpu.py.  numpy only.

`attention(q, k, v, do, causal, tiles)` is the closed form of tests/causal_ref.py

    S = Q Kᵀ / √D   (masked entries -inf: key j > query i)
    LSE = ln Σ_j exp(S),  P = exp(S - LSE),  O = P V
    Δ = rowsum(dO ∘ O),  dV = Pᵀ dO,  dS = P ∘ (dO Vᵀ - Δ) / √D,  dQ = dS K,  dK = dSᵀ Q

evaluated in float64 with, for 16-bit `tiles`, one rounding to the tile format at each
point DESIGN.md §5 names for the shipped kernels and nowhere else:

  * Q · log2e/√D, K, V and dO on their way into the tiles;
  * the forward's scores are in log2 units; P = exp2(s - m) is rounded for P·V;
  * the forward's row sum, by kernel family (`tiles`):
      "fp16", "bf16"   the compiler-scheduled kernels add up the packed P itself, in fp32
                       (v_dot2 against ones: "l sums exactly the P the PV MFMAs multiply");
      "fp16_hs"        the hand-scheduled fp16 forward (FWD_HS, FWD_SPLIT, full grids) adds
                       the packed P with v_pk_add_f16: per 64-key tile, lane half and
                       16-bit lane, 16 P through five 16-bit roundings (pairs, two more
                       terms each, then a tree over the four partials), fp32 from there on;
      "bf16_hs"        the hand-scheduled bf16 forward adds the unrounded P in fp32;
  * the backward's P = exp2(s - LSE · log2e) is rounded for Pᵀ·dO;
  * Δ = rowsum(dO ∘ O) from the unrounded dO and the forward's O as stored (fp32);
  * dS = P · (dP - Δ) is rounded once; in the fp16 dK/dV kernels it is the packed product
    (v_pk_mul_f16) of the rounded P and the rounded (dP - Δ), rounded again;
  * the dQ kernels hold the forward's tiles (Q · log2e/√D and K): dQ = dS · K / √D;
  * the dK/dV kernels (and roles) hold K · log2e/√D and the unscaled Q instead, so their
    scores, and the P of dV and dK, carry other roundings than the LSE they subtract
    (a row with one key has P = 1 in the forward and 1 +- a few ulp here):
    dV = Pᵀ · dO,  dK = dSᵀ · (rounded Q) / √D;
  * the backward consumes the model's own O and LSE (stored as fp32), as the kernels
    consume their own.

Every accumulation is exact (float64): fp32 accumulation order and the hardware exp2 are
what the margins cover.  `tiles="fp32"` is the same closed form evaluated in np.float32
with no 16-bit rounding, the yardstick of the exact-fp32 path: its products are k-ordered
float32 FMA chains (what v_mfma_f32_32x32x2_f32 computes), and the backward's score and dP
chains start from the seeds -LSE · log2e and -Δ as the kernels' accumulators do (DESIGN.md
§3), so every step of them rounds at the magnitude of the seed.  `tiles=None` is the float64
closed form itself (equal to causal_ref, test_rounding_model_cpu.py), which is also where
the `defect` argument applies the deliberate defects of the CPU defect table.

`errors(got, exact)` reduces a result to per-head figures, and `violations` is THE budget
check: the GPU test and the CPU defect table both call it with the constants below.
"""
import numpy as np

LOG2E = 1.4426950408889634
TENSORS = ("o", "lse", "dq", "dk", "dv")

# The margins of the budget: kernel error <= margin x model error, per tensor and per head
# (measured kernel/model ratios and how these were set: DESIGN.md §5 and the docstring of
# tests/test_gpu_error_budget.py).
M_RMS = {"fp16": 2.0, "bf16": 2.0, "fp32": 3.0}
M_MAX = {"fp16": 3.0, "bf16": 3.0, "fp32": 3.5}
TILES = ("fp16", "bf16", "fp16_hs", "bf16_hs", "fp32")  # model variants; margins go by the part before "_"

# Shapes of the budget cases (the smallest that reach each edge; S = 1024 is the smallest
# listed shape that BWD_SPLIT = 2 and the D = 64 FWD_SPLIT = 2 serve: S % 128 == 0).
SHAPES = [(1, 2, 33, 64), (2, 3, 65, 32), (1, 2, 257, 128), (2, 2, 300, 64), (1, 2, 576, 64), (1, 2, 777, 32),
          (1, 1, 640, 128), (1, 1, 1000, 64), (1, 2, 1024, 64)]
KINDS = ("uniform", "gaussian")


def inputs(shape, kind):
    """(q, k, v, do): Q, K, V of oracle.fa2_oracle.harness_inputs (U[0,1), "uniform") or
    cli_inputs (N(0,1), "gaussian"); dO ~ N(0,1)"""
    from oracle import fa2_oracle as fo

    q, k, v = fo.harness_inputs(*shape) if kind == "uniform" else fo.cli_inputs(*shape, seed=7)
    return q, k, v, np.random.RandomState(43).randn(*shape).astype(np.float32)


DEFECTS = ("drop_key", "swap_v", "scale", "dq_zero", "dk_last_row_zero", "diag_excluded", "delta_rounded_o")


def round_fp16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def round_bf16(x):
    """round-to-nearest-even to bfloat16 on the uint32 view of the float32 image"""
    u = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32)).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


ROUND = {"fp16": round_fp16, "bf16": round_bf16}


def packed_fp16_rowsum(p16):
    """row sums [..., S, 1] of the fp16 P [..., S, S'] (S' % 64 == 0) as the hand-scheduled
    fp16 forward adds them: per 64-key tile four groups (lane half x 16-bit lane) of 16 P,
    each through five fp16 roundings -- ((a + b) + c) + d for four partials, then
    (t0 + t1) + (t2 + t3) -- and exact (fp32 in the kernel) from there on.  Which 16 keys
    share a group does not matter to the size of the error; here they are contiguous."""
    r = round_fp16
    assert p16.shape[-1] % 64 == 0
    g = p16.reshape(p16.shape[:-1] + (-1, 4, 4))  # [..., groups of 16, partial, term]
    t = r(r(r(g[..., 0] + g[..., 1]) + g[..., 2]) + g[..., 3])
    t = r(r(t[..., 0] + t[..., 1]) + r(t[..., 2] + t[..., 3]))
    return t.sum(-1, keepdims=True)


def chain_matmul32(a, b, seed=None):
    """seed + a @ b as the fp32 MFMA computes it: per output element one k-ordered chain of
    fused multiply-adds from the seed, each rounded to float32 (the float64 product of two
    float32 is exact)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    acc = np.zeros(a.shape[:-1] + b.shape[-1:], np.float32)
    if seed is not None:
        acc = acc + np.asarray(seed, np.float32)
    for kk in range(a.shape[-1]):
        acc = (acc + a[..., :, kk:kk + 1] * b[..., kk:kk + 1, :]).astype(np.float32)
    return acc


def _mask(S, causal, defect):
    """boolean [S, S] of the allowed (query i, key j) pairs, or None for all"""
    if not causal:
        allowed = None
    elif defect == "diag_excluded":
        allowed = np.tril(np.ones((S, S), bool), -1)
        allowed[0, 0] = True  # row 0 keeps its only key, so the defective result stays finite
    else:
        allowed = np.tril(np.ones((S, S), bool))
    if defect == "drop_key":
        allowed = np.ones((S, S), bool) if allowed is None else allowed
        allowed[:, S // 2 if causal else S - 1] = False
    return allowed


def attention(q, k, v, do, causal=False, tiles=None, defect=None, defect_round="fp16"):
    """dict of o, lse, dq, dk, dv, delta (float64 arrays) for [B, H, S, D] inputs.

    `defect` (tiles=None only) is one of DEFECTS: one key dropped (S-1, or S//2 under the
    mask), the V rows of keys 40 and 41 swapped, 1/√D scaled by 1 + 2^-7, dQ = 0, dK's last
    row zeroed, the causal diagonal excluded, Δ taken from an O rounded to `defect_round`."""
    assert tiles in (None,) + TILES and (defect is None or (tiles is None and defect in DEFECTS))
    ft = np.float32 if tiles == "fp32" else np.float64
    fmt = tiles.split("_")[0] if tiles else None
    r16 = ROUND.get(fmt, lambda x: x)
    q, k, v, do = (np.asarray(x, ft) for x in (q, k, v, do))
    S, D = q.shape[-2], q.shape[-1]
    T = lambda x: np.swapaxes(x, -1, -2)  # noqa: E731
    mm = chain_matmul32 if tiles == "fp32" else np.matmul
    rsd = ft(1.0) / np.sqrt(ft(D))
    if defect == "scale":
        rsd = rsd * (1.0 + 2.0 ** -7)
    log2e, ln2 = ft(LOG2E), ft(1.0 / LOG2E)
    qs, kr, vr, dor = r16(q * (log2e * rsd)), r16(k), r16(v), r16(do)
    vf = vr
    if defect == "swap_v":
        vf = vr.copy()
        vf[..., [40, 41], :] = vr[..., [41, 40], :]
    # forward
    s = mm(qs, T(kr))  # log2 units
    allowed = _mask(S, causal, defect)
    if allowed is not None:
        s = np.where(allowed, s, ft(-np.inf))
    m = s.max(-1, keepdims=True)
    p = np.exp2(s - m)
    p16 = r16(p)
    if tiles == "fp16_hs":
        l = packed_fp16_rowsum(p16)
    else:
        l = (p if tiles == "bf16_hs" else p16).sum(-1, keepdims=True)
    o = mm(p16, vf) / l
    lse = ((m + np.log2(l)) * ln2)[..., 0]
    if fmt in ROUND:  # O and LSE as the kernels store them
        o, lse = o.astype(np.float32).astype(np.float64), lse.astype(np.float32).astype(np.float64)
    # backward, from the O and LSE above
    o_delta = ROUND[defect_round](o) if defect == "delta_rounded_o" else o
    delta = (do * o_delta).sum(-1)
    if tiles == "fp32":  # the accumulators are seeded with -LSE · log2e and -Δ
        sb = mm(qs, T(kr), seed=-(lse * log2e)[..., None])
        pb = np.exp2(sb if allowed is None else np.where(allowed, sb, ft(-np.inf)))
        dpd = mm(dor, T(vr), seed=-delta[..., None])
    else:
        pb = np.exp2(s - lse[..., None] * log2e)
        dpd = mm(dor, T(vr)) - delta[..., None]
    dq = mm(r16(pb * dpd), kr) * rsd
    if fmt in ROUND:
        # the dK/dV kernels keep K · log2e/√D and the unscaled Q in their tiles: the same
        # scores from other roundings than the forward's, so their P is not the forward's
        qr, ks = r16(q), r16(k * (log2e * rsd))
        skv = mm(qr, T(ks))
        pkv = np.exp2((skv if allowed is None else np.where(allowed, skv, -np.inf)) - lse[..., None] * log2e)
        dskv = r16(r16(pkv) * r16(dpd)) if fmt == "fp16" else r16(pkv * dpd)
        dv = mm(T(r16(pkv)), dor)
        dk = mm(T(dskv), qr) * rsd
    else:
        dv = mm(T(pb), dor)
        dk = mm(T(pb * dpd), qs) * ln2
    if defect == "dq_zero":
        dq = np.zeros_like(dq)
    if defect == "dk_last_row_zero":
        dk[..., -1, :] = 0.0
    return {n: np.asarray(x, np.float64) for n, x in
            (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv), ("delta", delta))}


def errors(got, exact):
    """{tensor: {"relmax": [B, H], "relrms": [B, H]}} of `got` against `exact` per head:
    relmax = max|got - exact| / max|exact|, relrms = rms(got - exact) / rms(exact); LSE is
    absolute (no division).  Tensors missing from `got` are left out."""
    out = {}
    for n in TENSORS:
        if n not in got:
            continue
        g, e = np.asarray(got[n], np.float64), np.asarray(exact[n], np.float64)
        assert g.shape == e.shape, (n, g.shape, e.shape)
        ax = (-1,) if n == "lse" else (-2, -1)
        d = g - e
        mx, rms = np.abs(d).max(ax), np.sqrt((d * d).mean(ax))
        if n != "lse":
            mx, rms = mx / np.abs(e).max(ax), rms / np.sqrt((e * e).mean(ax))
        out[n] = {"relmax": mx, "relrms": rms}
    return out


def ratios(kernel_err, model_err):
    """{tensor: {"relmax": worst kernel/model over heads, "relrms": ...}}"""
    return {n: {st: float((kernel_err[n][st] / model_err[n][st]).max()) for st in ("relmax", "relrms")}
            for n in kernel_err}


def violations(kernel_err, model_err, tiles):
    """The budget check: [(tensor, statistic, (b, h), kernel error, bound)] of every tensor
    and head whose error exceeds M_RMS[tiles] x the model's relrms or M_MAX[tiles] x the
    model's relmax (a non-finite error is a violation)."""
    fmt = tiles.split("_")[0]
    margin = {"relrms": M_RMS[fmt], "relmax": M_MAX[fmt]}
    bad = []
    for n, stats in kernel_err.items():
        for st, ke in stats.items():
            bound = margin[st] * model_err[n][st]
            for idx in zip(*np.nonzero(~(ke <= bound))):
                bad.append((n, st, tuple(int(i) for i in idx), float(ke[idx]), float(bound[idx])))
    return bad
