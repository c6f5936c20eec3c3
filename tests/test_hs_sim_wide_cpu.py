"""CPU checks of the four-chain forward loop (512-row workgroups, D = 64), no GPU needed.

gen/asmsim.py runs the FA2_HS4 blocks of kernels/fa2_fwd_hs.inc lane by lane, as it does
the two-chain loop (tests/test_hs_sim_cpu.py): four waves of four 32-row chains, the
barriers between them, every counted wait (a register read or written while its load is
outstanding fails the run).  Checked here:
  * the result against float64 attention at the project's tolerances (1e-2 fp16, 2e-2
    bf16, asserted inside the simulator), for both tile types, both loop exits (an odd
    and an even number of tiles), a block with waves past S and a second block;
  * O and LSE of the four-chain loop are bit for bit those of the two-chain loop: per row
    the two loops issue the same arithmetic in the same order;
  * a late score spike raises the flag, and only in the wave that holds the spiked rows;
  * a dropped wait is caught (the simulator's own guard works on this loop);
  * the committed .inc is what the generator writes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

GEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-flash-attention_amd", "gen")
sys.path.insert(0, GEN)
import asmsim  # noqa: E402


def sim(*args):
    r = subprocess.run([sys.executable, os.path.join(GEN, "asmsim.py"), "--kernel", "fwd", "--D", "64", "--chains", "4",
                        *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("S,block,bf16", [(128, 0, False), (192, 0, True), (256, 0, False), (320, 0, True),
                                          (576, 1, False)])
def test_wide_forward_loop(S, block, bf16):
    out = sim("--S", str(S), "--block", str(block), *(["--bf16"] if bf16 else []))
    assert "restart flag False" in out


@pytest.mark.parametrize("bf16", [False, True])
def test_wide_forward_loop_flags_a_late_spike(bf16):
    """a late key far above the first tile's row max raises every wave's restart flag"""
    out = sim("--S", "512", "--spike", *(["--bf16"] if bf16 else []))
    assert "restart flag True" in out and "flagged waves: [0, 1, 2, 3]" in out


@pytest.mark.parametrize("bf16", [False, True])
def test_wide_forward_loop_flags_only_the_spiked_wave(bf16):
    """rows 160..191 are chain 1 of wave 1: a key late in the head that only they score high on
    flags that wave alone (the flag is per wave: its four chains restart together)"""
    out = sim("--S", "512", "--spike", "--spike-rows", "160:192", *(["--bf16"] if bf16 else []))
    assert "restart flag True" in out and "flagged waves: [1]" in out


def _inputs(S, D=64):
    rng = np.random.RandomState(7)
    return [rng.rand(S, D).astype(np.float32) for _ in range(3)]


@pytest.mark.parametrize("bf16", [False, True])
def test_wide_rows_are_bitwise_the_two_chain_rows(bf16):
    S, D = 512, 64
    Q, K, V = _inputs(S)
    o4, l4, f4, _ = asmsim.Sim(D, bf16, S, Q, K, V, 0, 4).run()
    assert not f4
    for blk in range(2):
        o2, l2, f2, _ = asmsim.Sim(D, bf16, S, Q, K, V, blk, 2).run()
        assert not f2
        rows = slice(256 * blk, 256 * blk + 256)
        assert np.array_equal(o4[rows].view(np.uint32), o2.view(np.uint32))
        assert np.array_equal(l4[rows].view(np.uint32), l2.view(np.uint32))


def test_a_dropped_wait_fails_the_wide_run():
    """without one of the loop's counted waits a register is read before its load lands"""
    S, D = 256, 64
    Q, K, V = _inputs(S)
    s = asmsim.Sim(D, False, S, Q, K, V, 0, 4)
    text = s.asm_text(macro="FA2_HS4_ASM")
    loop = text.index("FA2HS_LOOP_0:")
    drop = next(i for i in range(loop, len(text)) if text[i].startswith("s_waitcnt vmcnt"))
    s.asm_text = lambda **kw: text[:drop] + text[drop + 1:]
    with pytest.raises(RuntimeError, match="before its load was waited for|with its load outstanding|already outstanding"):
        s.run()


def test_generated_wide_loop_is_current():
    """gen_fwd_hs.py --check covers the FA2_HS4 blocks: they are in kernels/fa2_fwd_hs.inc"""
    inc = open(os.path.join(GEN, "..", "kernels", "fa2_fwd_hs.inc")).read()
    assert "#define FA2_HS4_ASM_D64_F16" in inc and "#define FA2_HS4_ASM_D64_BF16" in inc
    r = subprocess.run([sys.executable, os.path.join(GEN, "gen_fwd_hs.py"), "--check"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
