#!/usr/bin/env python3
"""CPU simulator of the generated forward asm (gen_fwd_hs.py), for logic checks without a GPU.

Runs one 256-thread workgroup of fa2_fwd_hs_kernel<D>: the C++ prologue (Q block and the
first K/V tile staged into a swizzled fp16 LDS image, per-lane operand values), the asm
block of kernels/fa2_fwd_hs.inc instruction by instruction for the four waves (barriers
synchronise them), and the C++ epilogue (O rows from the LDS stage, LSE).  It checks:
  * every read of a register with an outstanding ds_read / buffer_load is covered by an
    earlier s_waitcnt (loads land only when a wait retires them, in issue order);
  * the result against float64 attention.
Instruction semantics (lane layouts of v_mfma_f32_32x32x16_*, ds_read_b64_tr_b16's 16-lane
transpose, buffer range checks) are the ones the library's compiled kernels rely on.
Timing and hazard wait states are not modelled (the generator inserts those).

  python3 asmsim.py [--D 64] [--S 256] [--bf16] [--spike] [--chains 4] [--spike-rows 160:192]
--chains 4 runs the four-chain loop (FA2_HS4_*: 512-row workgroups, D = 64).
"""
import argparse
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_fwd_hs as G  # noqa: E402

LOG2E = 1.4426950408889634


# ---------------------------------------------------------------------------------------
# 16-bit conversions
# ---------------------------------------------------------------------------------------
def f2h(x):
    return np.asarray(x, np.float32).astype(np.float16).view(np.uint16).astype(np.uint32)


def h2f(u):
    return (np.asarray(u, np.uint32) & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)


def f2bf(x):
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (r & 0xFFFF).astype(np.uint32)


def bf2f(u):
    return ((np.asarray(u, np.uint32) & 0xFFFF) << 16).astype(np.uint32).view(np.float32)


def u2f(u):
    return np.asarray(u, np.uint32).view(np.float32)


def f2u(f):
    return np.asarray(f, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------
# host-side replicas of the C++ helpers (kernel_fa2_optimized_f16.cu)
# ---------------------------------------------------------------------------------------
def swz_bwd(D, r):
    """f-attn2-backward_f16.cu's Swz<D> (conflict-free for both MFMA shapes)"""
    if D == 32:
        return ((r >> 2) & 1) | ((((r >> 2) ^ (r >> 3)) & 1) << 1)
    if D == 64:
        return ((r >> 1) & 1) | ((((r >> 1) ^ (r >> 2)) & 1) << 1) | ((((r >> 1) ^ (r >> 3)) & 1) << 2)
    return (r & 1) | (((r >> 1) & 1) << 1) | (((r ^ (r >> 2)) & 1) << 2) | (((r ^ (r >> 1) ^ (r >> 3)) & 1) << 3)


def swz(D, r):
    if D == 32:
        return ((r >> 2) & 1) | (((r >> 3) & 1) << 1)
    if D == 64:
        return ((r >> 1) & 1) | (((r >> 2) & 1) << 1) | ((((r >> 1) ^ (r >> 3)) & 1) << 2)
    return (r & 1) | (((r >> 1) & 1) << 1) | (((r ^ (r >> 2)) & 1) << 2) | ((((r >> 1) ^ (r >> 3)) & 1) << 3)


SWZ = [swz]


def tile_off(D, row, col):
    return row * D + (((col >> 3) ^ SWZ[0](D, row)) << 3) + (col & 7)


class Sim:
    def __init__(self, D, bf16, S, Q, K, V, block=0, chains=2):
        self.D, self.bf16, self.S = D, bf16, S
        self.chains = chains  # 32-row chains per wave of the forward (2, or 4: 512-row workgroups)
        cfg = G.Cfg(D, bf16, chains)
        self.cfg = cfg
        self.lds = np.zeros(cfg.lds_bytes // 4, np.uint32)  # dword-addressed
        self.Q, self.K, self.V = Q, K, V  # one head [S][D] float32
        self.block = block
        self.tensors = {"K": K, "V": V, "Q": Q}
        self.to16 = f2bf if bf16 else f2h
        self.from16 = bf2f if bf16 else h2f

    # LDS access (byte addresses)
    def lds_read16(self, addr):  # 16-bit element at byte addr
        w = self.lds[addr >> 2]
        return (w >> 16) & 0xFFFF if addr & 2 else w & 0xFFFF

    def lds_write16(self, addr, v):
        i = addr >> 2
        if addr & 2:
            self.lds[i] = (self.lds[i] & 0xFFFF) | (np.uint32(v) << 16)
        else:
            self.lds[i] = (self.lds[i] & 0xFFFF0000) | np.uint32(v)

    def stage(self, src, rows0, nrows, base_halves, scale):
        """TileStager<D, nrows, 256>.store: fp32 rows -> 16-bit swizzled image"""
        D = self.D
        for row in range(nrows):
            g = rows0 + row
            vals = src[g] * scale if g < self.S else np.zeros(D, np.float32)
            h = self.to16(vals.astype(np.float32))
            for col in range(D):
                self.lds_write16(2 * (base_halves + tile_off(D, row, col)), int(h[col]))

    def run(self, spike_check=True):
        """fa2_fwd_hs_kernel<D, NC>: the C++ prologue, the asm of fa2_fwd_hs.inc, the C++ epilogue"""
        D = self.D
        cfg = self.cfg
        TB = 64 * D
        NC = self.chains
        WR, ROWS = 32 * NC, 128 * NC  # query rows per wave and per workgroup
        q0 = self.block * ROWS
        self.stage(self.Q, q0, ROWS, 4 * TB, np.float32(LOG2E / np.sqrt(D)))
        self.stage(self.K, 0, 64, 0, np.float32(1.0))
        self.stage(self.V, 0, 64, 2 * TB, np.float32(1.0))
        lanes = np.arange(64)
        r, h = lanes & 31, lanes >> 5
        g, i16 = lanes >> 4, lanes & 15
        ka = [np.array([2 * tile_off(D, int(r[l]), 16 * t + 8 * int(h[l])) for l in lanes]) for t in range(D // 16)]
        rt = 4 * (g >> 1) + (i16 >> 2)
        ct = 16 * (g & 1) + 4 * (i16 & 3)
        va = [[np.array([2 * tile_off(D, int(rt[l]) + 8 * k, 32 * b + int(ct[l])) for l in lanes]) for k in range(2)]
              for b in range(D // 32)]
        waves = []
        text = self.asm_text(macro="FA2_HS4_ASM" if NC == 4 else "FA2_HS_ASM")
        for w in range(4):
            tid = 64 * w + lanes
            CPR = D // 8
            vo, lo = [], None
            for c in range(D // 32):
                x = tid + 256 * c
                row, ch = x // CPR, x % CPR
                vo.append((row * D + ch * 8) * 4)
                if c == 0:
                    lo = 2 * np.array([row[l] * D + ((ch[l] ^ SWZ[0](D, int(row[l]))) << 3) for l in lanes])
            ops = {"qb": 4 * TB * 2 + w * WR * D * 2, "cnt": self.S // 64 - 1, "goff": 64 * D * 4, "flg": 0,
                   "oa": ((w * WR + r) * cfg.OST + 4 * h) * 4, "lo": lo, "rsk": "K", "rsv": "V"}
            for t in range(len(ka)):
                ops[f"ka{t}"] = ka[t]
            for b in range(len(va)):
                for k in range(2):
                    ops[f"va{b}_{k}"] = va[b][k]
            for c in range(D // 32):
                ops[f"vo{c}"] = vo[c]
            waves.append(Wave(self, w, text, ops))
        # run the waves to each barrier in turn
        gens = [wv.execute() for wv in waves]
        live = list(range(4))
        while live:
            states = {}
            for k in live:
                states[k] = next(gens[k], "done")
            if any(s == "done" for s in states.values()):
                assert all(s == "done" for s in states.values()), f"barrier mismatch: {states}"
                break
        # C++ epilogue
        flag = any(wv.ops["flg"] for wv in waves)
        O = np.zeros((ROWS, D), np.float32)
        LSE = np.zeros(ROWS, np.float32)
        for w, wv in enumerate(waves):
            for c in range(NC):
                l = wv.ops[f"ol{c}"]
                lt = l[:32] + l[32:]
                m = wv.ops[f"om{c}"][:32]
                for q in range(32):
                    R = w * WR + c * 32 + q
                    row = u2f(self.lds[(R * cfg.OST * 4) // 4: (R * cfg.OST * 4) // 4 + D])
                    O[R] = row / lt[q]
                    LSE[R] = m[q] * np.log(2.0) + np.log(lt[q])
        return O, LSE, flag, waves

    def run_dq(self, dO, LSE, Delta):
        """fa2_bwd_dq_hs_kernel<64>: the C++ prologue, the asm of fa2_bwd_dq_hs.inc, the dQ rows"""
        import gen_bwd_dq as GD
        SWZ[0] = swz_bwd
        D = self.D
        cfg = GD.Cfg(D, self.bf16)
        m16 = True
        TB = 64 * D
        self.lds = np.zeros(cfg.lds_bytes // 4, np.uint32)
        q0 = self.block * 256
        self.stage(self.Q, q0, 256, 4 * TB, np.float32(LOG2E / np.sqrt(D)))
        self.stage(dO, q0, 256, 8 * TB, np.float32(1.0))
        self.stage(self.K, 0, 64, 0, np.float32(1.0))
        self.stage(self.V, 0, 64, 2 * TB, np.float32(1.0))
        lanes = np.arange(64)
        r, h = lanes & 31, lanes >> 5
        g, i16 = lanes >> 4, lanes & 15
        ka = [np.array([2 * tile_off(D, int(r[l]), 16 * t + 8 * int(h[l])) for l in lanes]) for t in range(D // 16)]
        rt = 4 * (g >> 1) + (i16 >> 2)
        ct = 16 * (g & 1) + 4 * (i16 & 3)
        kt = [[np.array([2 * tile_off(D, int(rt[l]) + 8 * k, 32 * b + int(ct[l])) for l in lanes]) for k in range(2)]
              for b in range(D // 32)]
        if m16:
            ka = [np.array([2 * tile_off(D, int(i16[l]), 32 * ks + 8 * int(g[l])) for l in lanes]) for ks in range(D // 32)]
            kt = [[np.array([2 * tile_off(D, 16 * k + 4 * int(g[l]) + (int(i16[l]) >> 2), 16 * db + 4 * (int(i16[l]) & 3))
                             for l in lanes]) for k in range(2)] for db in range(D // 16)]
        text = self.asm_text("fa2_bwd_dq_hs.inc", "FA2_DQ_ASM")
        waves = []
        for w in range(4):
            tid = 64 * w + lanes
            CPR = D // 8
            vo, lo = [], None
            for c in range(D // 32):
                x = tid + 256 * c
                row, ch = x // CPR, x % CPR
                vo.append((row * D + ch * 8) * 4)
                if c == 0:
                    lo = 2 * np.array([row[l] * D + ((ch[l] ^ SWZ[0](D, int(row[l]))) << 3) for l in lanes])
            ops = {"qb": 4 * TB * 2 + w * 64 * D * 2, "db": 8 * TB * 2 + w * 64 * D * 2, "cnt": self.S // 64 - 1,
                   "goff": 64 * D * 4, "oa": ((w * 64 + r) * cfg.OST + 4 * h) * 4, "lo": lo, "rsk": "K", "rsv": "V"}
            nblk, rows = (4, lambda c: 16 * c + i16) if m16 else (2, lambda c: 32 * c + r)
            for c in range(nblk):
                qq = q0 + w * 64 + rows(c)
                ok = qq < self.S
                nl = np.where(ok, -LSE[np.minimum(qq, self.S - 1)] * LOG2E, -np.inf).astype(np.float32)
                nd = np.where(ok, -Delta[np.minimum(qq, self.S - 1)], 0).astype(np.float32)
                ops[f"nl{c}"], ops[f"nd{c}"] = f2u(nl), f2u(nd)
            if m16:
                ops["oa"] = ((w * 64 + i16) * cfg.OST + 4 * g) * 4
            for t in range(len(ka)):
                ops[f"ka{t}"] = ka[t]
            for b in range(len(kt)):
                for k in range(2):
                    ops[f"kt{b}_{k}"] = kt[b][k]
            for c in range(D // 32):
                ops[f"vo{c}"] = vo[c]
            waves.append(Wave(self, w, text, ops))
        gens = [wv.execute() for wv in waves]
        while True:
            states = [next(gn, "done") for gn in gens]
            if "done" in states:
                assert all(st == "done" for st in states), f"barrier mismatch: {states}"
                break
        dQ = np.zeros((256, D), np.float32)
        for R_ in range(256):
            dQ[R_] = u2f(self.lds[R_ * cfg.OST: R_ * cfg.OST + D]) / np.sqrt(D)
        SWZ[0] = swz
        return dQ

    def run_dkdv(self, dO, LSE, Delta):
        """fa2_bwd_dkdv_hs_kernel<64>: the C++ prologue, the asm of fa2_bwd_dkdv_hs.inc, dK and dV rows"""
        import gen_bwd_dkdv as GK
        SWZ[0] = swz_bwd
        D = self.D
        cfg = GK.Cfg(D, self.bf16)
        TB = 64 * D
        self.lds = np.zeros(cfg.lds_bytes // 4, np.uint32)
        self.tensors.update({"dO": dO, "LSE": LSE, "Delta": Delta, "null": np.zeros(0, np.float32)})
        k0 = self.block * 256
        self.stage(self.K, k0, 256, cfg.KVB // 2, np.float32(LOG2E / np.sqrt(D)))
        self.stage(self.V, k0, 256, cfg.KVB // 2 + 256 * D, np.float32(1.0))
        self.stage(self.Q, 0, 64, 0, np.float32(1.0))
        self.stage(dO, 0, 64, TB, np.float32(1.0))
        for q in range(64):
            ok = q < self.S
            self.lds[(cfg.RC >> 2) + q] = f2u(np.float32(-LSE[q] * LOG2E if ok else 0.0))
            self.lds[(cfg.RC >> 2) + 64 + q] = f2u(np.float32(-Delta[q] if ok else 0.0))
        lanes = np.arange(64)
        g, i16 = lanes >> 4, lanes & 15
        # 16x16x32 maps (FragOffsets16): row reads row l & 15, columns 32 ks + 8g; transposed
        # reads rows 16k + 4g + (i >> 2), columns 16 md + 4 (i & 3)
        ka = [np.array([2 * tile_off(D, int(i16[l]), 32 * ks + 8 * int(g[l])) for l in lanes]) for ks in range(D // 32)]
        tr = [[np.array([2 * tile_off(D, 16 * k + 4 * int(g[l]) + (int(i16[l]) >> 2), 16 * md + 4 * (int(i16[l]) & 3))
                         for l in lanes]) for k in range(2)] for md in range(D // 16)]
        text = self.asm_text("fa2_bwd_dkdv_hs.inc", "FA2_DK_ASM")
        waves = []
        for w in range(4):
            tid = 64 * w + lanes
            CPR = D // 8
            vo, lo = [], None
            for c in range(D // 32):
                x = tid + 256 * c
                row, ch = x // CPR, x % CPR
                vo.append((row * D + ch * 8) * 4)
                if c == 0:
                    lo = 2 * np.array([row[l] * D + ((ch[l] ^ SWZ[0](D, int(row[l]))) << 3) for l in lanes])
            oak = ((w * 64 + i16) * cfg.OST + 4 * g) * 4
            ops = {"cnt": self.S // 64 - 1, "goff": 64 * D * 4, "roff": 256, "lo": lo, "rco": 16 * g,
                   "rvo": 4 * lanes, "rcw": (256 * w if w < 2 else 512) + 4 * lanes, "oak": oak,
                   "oav": oak + 256 * cfg.OST * 4, "rsq": "Q", "rsd": "dO",
                   "rsc": ["LSE", "Delta", "null", "null"][w],
                   "rsm": int(f2u(np.float32([-LOG2E, -1.0, 0.0, 0.0][w]))), "kvb": cfg.KVB + w * 64 * D * 2}
            for t in range(D // 32):
                ops[f"ka{t}"] = ka[t]
            for b in range(D // 16):
                for k in range(2):
                    ops[f"tr{b}_{k}"] = tr[b][k]
            for c in range(D // 32):
                ops[f"vo{c}"] = vo[c]
            waves.append(Wave(self, w, text, ops))
        gens = [wv.execute() for wv in waves]
        while True:
            states = [next(gn, "done") for gn in gens]
            if "done" in states:
                assert all(st == "done" for st in states), f"barrier mismatch: {states}"
                break
        dK = np.zeros((256, D), np.float32)
        dV = np.zeros((256, D), np.float32)
        for R_ in range(256):
            dK[R_] = u2f(self.lds[R_ * cfg.OST: R_ * cfg.OST + D]) / np.sqrt(D)
            dV[R_] = u2f(self.lds[(256 + R_) * cfg.OST: (256 + R_) * cfg.OST + D])
        SWZ[0] = swz
        return dK, dV

    def asm_text(self, inc="fa2_fwd_hs.inc", macro="FA2_HS_ASM"):
        path = os.path.join(HERE, "..", "kernels", inc)
        tag = f"D{self.D}_{'BF16' if self.bf16 else 'F16'}"
        src = open(path).read()
        blk = src.split(f"#define {macro}_{tag} \\\n")[1].split('    ""')[0]
        lines = [ln.strip()[1:].split("\\n")[0] for ln in blk.splitlines() if ln.strip().startswith('"')]
        return [ln.replace("%=", "0") for ln in lines]


class Wave:
    def __init__(self, sim, wid, text, ops):
        self.sim, self.wid, self.text, self.ops = sim, wid, text, ops
        self.v = np.zeros((256, 64), np.uint32)
        self.a = np.zeros((256, 64), np.uint32)
        self.vcc = np.zeros(64, bool)
        self.scc = False
        self.lgkm, self.vm = [], []  # outstanding: (regs, landing function)
        self.pending = set()
        self.labels = {ln[:-1]: i for i, ln in enumerate(text) if ln.endswith(":")}

    # register helpers
    def regs(self, tok):
        m = re.fullmatch(r"([va])\[(\d+):(\d+)\]", tok)
        if m:
            return [(m.group(1), k) for k in range(int(m.group(2)), int(m.group(3)) + 1)]
        m = re.fullmatch(r"([va])(\d+)", tok)
        if m:
            return [(m.group(1), int(m.group(2)))]
        return []

    def get(self, f, k):
        if (f, k) in self.pending:
            raise RuntimeError(f"wave {self.wid}: read of {f}{k} before its load was waited for (line {self.pc})")
        return (self.v if f == "v" else self.a)[k]

    def put(self, f, k, val):
        if (f, k) in self.pending:
            raise RuntimeError(f"wave {self.wid}: write of {f}{k} with its load outstanding (line {self.pc})")
        (self.v if f == "v" else self.a)[k] = np.asarray(val, np.uint32)

    def vsrc(self, tok):
        """per-lane uint32 value of a source token"""
        if tok.startswith("%["):
            val = self.ops[tok[2:-1]]
            return np.broadcast_to(np.asarray(val, np.int64).astype(np.uint32), (64,)).copy()
        if tok.startswith("0x"):
            return np.full(64, int(tok, 16), np.uint32)
        if re.fullmatch(r"-?\d+", tok):
            return f2u(np.full(64, float(tok), np.float32)) if tok != "0" else np.zeros(64, np.uint32)
        (f, k), = self.regs(tok)
        return self.get(f, k)

    def wait(self, q, n):
        while len(q) > n:
            regs, land = q.pop(0)
            for rr in regs:
                self.pending.discard(rr)
            land()

    def execute(self):
        sim = self.sim
        D = sim.D
        self.pc = 0
        text = self.text
        while self.pc < len(text):
            ln = text[self.pc]
            self.pc += 1
            if ln.endswith(":"):
                continue
            op, _, rest = ln.partition(" ")
            args = [a.strip() for a in re.split(r",\s*(?![^\[]*\])", rest)] if rest else []
            if op == "s_waitcnt":
                for part in rest.split():
                    n = int(part.split("(")[1][:-1])
                    self.wait(self.lgkm if part.startswith("lgkmcnt") else self.vm, n)
            elif op == "s_nop":
                pass
            elif op == "s_barrier":
                yield "barrier"
            elif op == "s_mov_b64":
                self.ops[args[0][2:-1]] = 0
            elif op == "s_or_b64":
                self.ops["flg"] = int(self.ops["flg"]) | int(self.vcc.any())
            elif op == "s_add_u32":
                self.ops[args[0][2:-1]] = int(self.ops[args[1][2:-1]]) + int(args[2])
            elif op == "s_sub_u32":
                self.ops[args[0][2:-1]] = int(self.ops[args[1][2:-1]]) - int(args[2])
                self.scc = False
            elif op == "s_cmp_eq_u32":
                self.scc = int(self.ops[args[0][2:-1]]) == int(args[1])
            elif op == "s_cmp_lg_u32":
                self.scc = int(self.ops[args[0][2:-1]]) != int(args[1])
            elif op == "s_cbranch_scc1":
                if self.scc:
                    self.pc = self.labels[args[0]]
            elif op == "buffer_load_dwordx4":
                dst = self.regs(args[0])
                voff = self.vsrc(args[1]).astype(np.int64)
                tens = sim.tensors[self.ops[args[2][2:-1]]]
                soff = int(self.ops[args[3].split()[0][2:-1]])
                imm = int(args[3].split("offset:")[1]) if "offset:" in args[3] else 0
                flat = tens.reshape(-1)
                addr = voff + soff + imm
                data = np.zeros((4, 64), np.uint32)
                for e in range(4):
                    idx = (addr + 4 * e) // 4
                    ok = (addr + 4 * e + 4) <= flat.size * 4
                    data[e] = np.where(ok, f2u(flat[np.minimum(idx, flat.size - 1)]), 0)
                self.issue(self.vm, dst, data)
            elif op == "buffer_load_dword":
                dst = self.regs(args[0])
                voff = self.vsrc(args[1]).astype(np.int64)
                flat = sim.tensors[self.ops[args[2][2:-1]]].reshape(-1)
                soff = int(self.ops[args[3].split()[0][2:-1]])
                addr = voff + soff
                ok = (addr + 4) <= flat.size * 4
                data = np.where(ok, f2u(flat[np.minimum(addr // 4, max(flat.size - 1, 0))]) if flat.size else 0, 0)
                self.issue(self.vm, dst, np.asarray(data, np.uint32).reshape(1, 64))
            elif op == "ds_write_b32":
                dtok, _, offs = args[1].partition(" offset:")
                addr = self.vsrc(args[0]).astype(np.int64) + (int(offs) if offs else 0)
                src = self.vsrc(dtok)
                for l in range(64):
                    sim.lds[int(addr[l]) >> 2] = src[l]
                self.lgkm.append(([], lambda: None))
            elif op == "s_branch":
                self.pc = self.labels[args[0]]
            elif op in ("ds_read_b128", "ds_read_b64_tr_b16"):
                dst = self.regs(args[0])
                tok, _, offs = args[1].partition(" offset:")
                addr = self.vsrc(tok).astype(np.int64) + (int(offs) if offs else 0)
                if op == "ds_read_b128":
                    data = np.stack([sim.lds[(addr >> 2) + e] for e in range(4)])
                else:
                    # each lane reads 4 x 16-bit at its address; within each 16-lane group,
                    # output lane o, value j = element (o & 3) of source lane 4j + (o >> 2)
                    el = np.array([[sim.lds_read16(int(addr[l]) + 2 * e) for e in range(4)] for l in range(64)],
                                  np.uint32)
                    out = np.zeros((64, 4), np.uint32)
                    for grp in range(4):
                        for o in range(16):
                            for j in range(4):
                                out[16 * grp + o, j] = el[16 * grp + 4 * j + (o >> 2), o & 3]
                    data = np.stack([out[:, 0] | (out[:, 1] << 16), out[:, 2] | (out[:, 3] << 16)])
                self.issue(self.lgkm, dst, data)
            elif op == "ds_write_b128":
                dtok, _, offs = args[1].partition(" offset:")
                addr = self.vsrc(args[0]).astype(np.int64) + (int(offs) if offs else 0)
                src = [self.get(f, k) for f, k in self.regs(dtok)]
                for l in range(64):
                    for e in range(4):
                        sim.lds[(int(addr[l]) >> 2) + e] = src[e][l]
                self.lgkm.append(([], lambda: None))
            elif op.startswith("v_mfma_f32_32x32x16"):
                self.mfma(args)
            elif op.startswith("v_mfma_f32_16x16x32"):
                self.mfma16(args)
            elif op == "v_exp_f32":
                (f, k), = self.regs(args[0])
                x = u2f(self.vsrc(args[1]))
                with np.errstate(over="ignore"):
                    self.put(f, k, f2u(np.exp2(x.astype(np.float64)).astype(np.float32)))
            elif op in ("v_add_f32", "v_sub_f32", "v_max_f32", "v_max3_f32", "v_mul_f32"):
                (f, k), = self.regs(args[0])
                xs = [u2f(self.vsrc(a)).astype(np.float32) for a in args[1:]]
                if op == "v_add_f32":
                    y = xs[0] + xs[1]
                elif op == "v_sub_f32":
                    y = xs[0] - xs[1]
                elif op == "v_mul_f32":
                    y = xs[0] * xs[1]
                else:
                    y = np.maximum.reduce(xs)
                self.put(f, k, f2u(y))
            elif op in ("v_pk_add_f16", "v_pk_mul_f16"):
                (f, k), = self.regs(args[0])
                x, y = self.vsrc(args[1]), self.vsrc(args[2])
                h = lambda u, sh: ((u >> sh) & 0xFFFF).astype(np.uint16).view(np.float16)
                fn = (lambda a, b: a + b) if op == "v_pk_add_f16" else (lambda a, b: a * b)
                lo = fn(h(x, 0), h(y, 0)).astype(np.float16).view(np.uint16).astype(np.uint32)
                hi = fn(h(x, 16), h(y, 16)).astype(np.float16).view(np.uint16).astype(np.uint32)
                self.put(f, k, lo | (hi << 16))
            elif op in ("v_cvt_f32_f16_e32", "v_cvt_f32_f16_sdwa"):
                (f, k), = self.regs(args[0])
                x = self.vsrc(args[1].split()[0])
                sh = 16 if op.endswith("sdwa") and "src0_sel:WORD_1" in ln else 0
                self.put(f, k, f2u(((x >> sh) & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)))
            elif op == "v_add_u32":
                (f, k), = self.regs(args[0])
                self.put(f, k, (self.vsrc(args[1]).astype(np.uint64) + self.vsrc(args[2])).astype(np.uint32))
            elif op == "v_mov_b32":
                val = self.vsrc(args[1])
                if args[0].startswith("%["):
                    self.ops[args[0][2:-1]] = u2f(val).copy()
                else:
                    (f, k), = self.regs(args[0])
                    self.put(f, k, val)
            elif op == "v_accvgpr_write_b32":
                (f, k), = self.regs(args[0])
                self.put(f, k, self.vsrc(args[1]))
            elif op == "v_permlane16_swap_b32":
                # odd 16-lane rows of the first operand <-> even rows of the second
                (fa, ka), = self.regs(args[0])
                (fb, kb), = self.regs(args[1])
                x, y = self.get(fa, ka).copy(), self.get(fb, kb).copy()
                x2, y2 = x.copy(), y.copy()
                for rw in (0, 2):
                    x2[16 * (rw + 1):16 * (rw + 2)] = y[16 * rw:16 * (rw + 1)]
                    y2[16 * rw:16 * (rw + 1)] = x[16 * (rw + 1):16 * (rw + 2)]
                self.put(fa, ka, x2)
                self.put(fb, kb, y2)
            elif op == "v_permlane32_swap_b32":
                (fa, ka), = self.regs(args[0])
                (fb, kb), = self.regs(args[1])
                x, y = self.get(fa, ka).copy(), self.get(fb, kb).copy()
                x2, y2 = x.copy(), y.copy()
                x2[32:] = y[:32]
                y2[:32] = x[32:]
                self.put(fa, ka, x2)
                self.put(fb, kb, y2)
            elif op in ("v_cvt_pk_f16_f32", "v_cvt_pk_bf16_f32"):
                (f, k), = self.regs(args[0])
                lo, hi = u2f(self.vsrc(args[1])), u2f(self.vsrc(args[2]))
                self.put(f, k, sim.to16(lo) | (sim.to16(hi) << 16))
            elif op in ("v_cmp_nle_f32", "v_cmp_nge_f32"):
                c = u2f(self.vsrc(args[1]))
                x = u2f(self.vsrc(args[2]))
                self.vcc = ~(c <= x) if op == "v_cmp_nle_f32" else ~(c >= x)
            else:
                raise RuntimeError(f"unsupported instruction: {ln}")
        yield "done"

    def issue(self, q, dst, data):
        for rr in dst:
            if rr in self.pending:
                raise RuntimeError(f"wave {self.wid}: load into {rr} with a load already outstanding")
        regs = list(dst)

        def land():
            for e, (f, k) in enumerate(regs):
                (self.v if f == "v" else self.a)[k] = data[e]
        for rr in dst:
            self.pending.add(rr)
        q.append((regs, land))

    def mfma(self, args):
        sim = self.sim
        dst = self.regs(args[0])
        A = np.stack([self.get(f, k) for f, k in self.regs(args[1])])  # 4 regs x 64 lanes
        B = np.stack([self.get(f, k) for f, k in self.regs(args[2])])
        C = np.zeros((16, 64), np.float32) if args[3] == "0" else np.stack(
            [u2f(self.get(f, k)) for f, k in self.regs(args[3])])

        def halves(X):  # [64 lanes][8] floats
            return np.stack([sim.from16(X[e // 2] >> (16 * (e % 2))) for e in range(8)], axis=1)
        a, b = halves(A).astype(np.float64), halves(B).astype(np.float64)
        Am = np.zeros((32, 16))
        Bm = np.zeros((16, 32))
        for l in range(64):
            for j in range(8):
                Am[l % 32, 8 * (l // 32) + j] = a[l, j]
                Bm[8 * (l // 32) + j, l % 32] = b[l, j]
        P = Am @ Bm
        out = np.zeros((16, 64), np.float32)
        for l in range(64):
            for i in range(16):
                m = (i & 3) + 8 * (i >> 2) + 4 * (l // 32)
                out[i, l] = np.float32(C[i, l] + P[m, l % 32])
        for i, (f, k) in enumerate(dst):
            self.put(f, k, f2u(out[i]))


    def mfma16(self, args):
        """v_mfma_f32_16x16x32: A[l % 16][8 (l / 16) + j], B[8 (l / 16) + j][l % 16],
        D reg i -> row 4 (l / 16) + i, column l % 16"""
        sim = self.sim
        dst = self.regs(args[0])
        A = np.stack([self.get(f, k) for f, k in self.regs(args[1])])
        B = np.stack([self.get(f, k) for f, k in self.regs(args[2])])
        C = np.zeros((4, 64), np.float32) if args[3] == "0" else np.stack(
            [u2f(self.get(f, k)) for f, k in self.regs(args[3])])

        def halves(X):
            return np.stack([sim.from16(X[e // 2] >> (16 * (e % 2))) for e in range(8)], axis=1)
        a, b = halves(A).astype(np.float64), halves(B).astype(np.float64)
        Am = np.zeros((16, 32))
        Bm = np.zeros((32, 16))
        for l in range(64):
            for j in range(8):
                Am[l % 16, 8 * (l // 16) + j] = a[l, j]
                Bm[8 * (l // 16) + j, l % 16] = b[l, j]
        P = Am @ Bm
        out = np.zeros((4, 64), np.float32)
        for l in range(64):
            for i in range(4):
                out[i, l] = np.float32(C[i, l] + P[4 * (l // 16) + i, l % 16])
        for i, (f, k) in enumerate(dst):
            self.put(f, k, f2u(out[i]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--spike", action="store_true")
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--kernel", choices=["fwd", "dq", "dkdv"], default="fwd")
    ap.add_argument("--chains", type=int, choices=[2, 4], default=2, help="forward: 32-row chains per wave")
    ap.add_argument("--spike-rows", default="", help="forward: lo:hi, the query rows a late key spikes (with --spike)")
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    S, D = a.S, a.D
    Q, K, V = (rng.rand(S, D).astype(np.float32) for _ in range(3))
    if a.kernel == "dkdv":
        dO = rng.randn(S, D).astype(np.float32)
        s64 = (Q.astype(np.float64) @ K.T.astype(np.float64)) / np.sqrt(D)
        mx = s64.max(1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(s64 - mx).sum(1))
        P = np.exp(s64 - lse[:, None])
        O = P @ V.astype(np.float64)
        delta = (dO.astype(np.float64) * O).sum(1)
        dS = P * (dO.astype(np.float64) @ V.T.astype(np.float64) - delta[:, None])
        edk = dS.T @ Q.astype(np.float64) / np.sqrt(D)
        edv = P.T @ dO.astype(np.float64)
        sim = Sim(D, a.bf16, S, Q, K, V, a.block)
        dk, dv = sim.run_dkdv(dO, lse.astype(np.float32), delta.astype(np.float32))
        k0 = a.block * 256
        nk = min(256, S - k0)
        ek = np.abs(dk[:nk] - edk[k0:k0 + nk]).max() / max(1.0, np.abs(edk).max())
        ev = np.abs(dv[:nk] - edv[k0:k0 + nk]).max() / max(1.0, np.abs(edv).max())
        print(f"dKdV D={D} S={S} {'bf16' if a.bf16 else 'fp16'} block {a.block}: rel max|ddK| {ek:.3e}, |ddV| {ev:.3e}")
        tol = 2e-2 if a.bf16 else 1e-2
        assert ek < tol and ev < tol, "mismatch"
        return
    if a.kernel == "dq":
        dO = rng.randn(S, D).astype(np.float32)
        s64 = (Q.astype(np.float64) @ K.T.astype(np.float64)) / np.sqrt(D)
        mx = s64.max(1, keepdims=True)
        lse = mx[:, 0] + np.log(np.exp(s64 - mx).sum(1))
        P = np.exp(s64 - lse[:, None])
        O = P @ V.astype(np.float64)
        delta = (dO.astype(np.float64) * O).sum(1)
        dS = P * (dO.astype(np.float64) @ V.T.astype(np.float64) - delta[:, None])
        edq = dS @ K.astype(np.float64) / np.sqrt(D)
        sim = Sim(D, a.bf16, S, Q, K, V, a.block)
        dq = sim.run_dq(dO, lse.astype(np.float32), delta.astype(np.float32))
        q0 = a.block * 256
        nq = min(256, S - q0)
        err = np.abs(dq[:nq] - edq[q0:q0 + nq]).max()
        scale = max(1.0, np.abs(edq).max())
        print(f"dQ D={D} S={S} {'bf16' if a.bf16 else 'fp16'} block {a.block}: max|ddQ| {err:.3e} (scale {scale:.2f})")
        assert err < (2e-2 if a.bf16 else 1e-2) * scale, "mismatch"
        return
    if a.spike and a.spike_rows:
        # only rows lo..hi-1 see the late key: their Q rows and that key share one large column
        lo, hi = (int(x) for x in a.spike_rows.split(":"))
        Q[:, 0] = 0.0
        Q[lo:hi, 0] = 30.0
        K[:, 0] = 0.0
        K[S - 3, 0] = 30.0
    elif a.spike:
        K[S - 3] = 3.0
    sim = Sim(D, a.bf16, S, Q, K, V, a.block, a.chains)
    O, LSE, flag, waves = sim.run()
    rows = 128 * a.chains
    q0 = a.block * rows
    nq = min(rows, S - q0)
    s = (Q[q0:q0 + nq].astype(np.float64) @ K.T.astype(np.float64)) / np.sqrt(D)
    mx = s.max(1, keepdims=True)
    p = np.exp(s - mx)
    lse = (mx[:, 0] + np.log(p.sum(1)))
    o = (p / p.sum(1, keepdims=True)) @ V.astype(np.float64)
    eo = np.abs(O[:nq] - o).max()
    el = np.abs(LSE[:nq] - lse).max()
    print(f"D={D} S={S} {'bf16' if a.bf16 else 'fp16'} block {a.block}: restart flag {flag}, "
          f"max|dO| {eo:.3e}, max|dLSE| {el:.3e}")
    print("flagged waves:", [w for w, wv in enumerate(waves) if wv.ops["flg"]])
    if not flag:
        tol = 2e-2 if a.bf16 else 1e-2
        assert eo < tol and el < tol, "mismatch"


if __name__ == "__main__":
    main()
