"""TEST INFRASTRUCTURE ONLY -- exact inputs for the tiled W4A16 grouped GEMM (csrc/k_moe_gemm4.h, vl2_moe_gemm_mxfp4): the case table, the
generator, the guards and the runners shared by tests/test_gpu_moe_gemm4.py and tests/test_moe_gemm4_host.py.  Built on
tests/moe_exact.py (GemmCase, its checker and its frame conventions) and tests/moe_mxfp4_exact.py (the MXFP4-exact stacks, `survives`).

THE RULE.  Expert weights are g 2^p (moe_mxfp4_exact.mx4_stack): g on the E2M1 grid, every non-zero block holds a 4 or a 6, one block and one
row of every stack are zero, and p = (e + n + 2 b) % 3 per block of 32 k.  p differs between the two blocks of one 64-deep K-tile (2 % 3),
between neighbouring rows, between the gate and the up row of a SwiGLU pair (rows 32 apart: 32 % 3 = 2) and between neighbouring experts
(asserted by tests/test_moe_gemm4_host.py), so a swapped k-step scale, a wrong row's scale, gate and up scales swapped and a wrong expert's
scales each change the output.  The quantiser's exponent of such a block is p and nothing rounds: quantise -> dequantise returns the stack
(`survives`, asserted per case on tests/mxfp4_oracle.py) and the fp64 answer on the 16-bit stack IS the kernel's answer.  All weights lie in
[0.5, 24]: normal halves, the cases run on the fp16 build.

THE GUARDS, per case: moe_exact.GemmCase's with the quantum of this rule.  Activations are small integers times A's power of two sa, so every
product is a multiple of u = 0.5 sa (0.5 = the smallest non-zero |weight|), and every pre-activation value a multiple of q = u (u / 8 with the
row norm); the sum of |products| stays below 2^24 q per output (asserted), so the accumulation is exact in any order -- in this kernel and in
moe_gemm_kernel on the dequantised stack alike.

STORAGE.  q is a strided view of a byte allocation filled with 0x77 (two codes of 6): ldq = K / 2 + 16, q_stride = (N + 1) ldq; s of an
allocation filled with 0xFF (E8M0 NaN): lds = K / 32 + 3 (the scales travel as byte pieces: no alignment rule), s_stride = (N + 1) lds; A,
row_norm and the SENTINEL frame of C as in GemmCase.

Nothing under videollama2_amd/ imports this file."""
import math

import torch

from tests import gemm_exact as G
from tests import moe_exact as X
from tests import moe_mxfp4_exact as X4
from tests import mxfp4_oracle as M4

NAN, SENTINEL, EPS, MOE_BM = X.NAN, X.SENTINEL, X.EPS, X.MOE_BM
RING = 7                                           # k_moe_gemm4.h MOE4_STAGES (held against the header in tests/test_moe_gemm4_host.py)
K4_ALL = G.K_ALL + (64 * RING, 64 * (RING + 1))    # K_ALL holds 1 .. 5 and 17 K-tiles: below the ring depth; RING and RING + 1 are added
W_UNIT = 0.5                                       # the smallest non-zero |weight| of mx4_stack at shift 0


def gemm4_table():
    """moe_gemm8_exact.gemm8_table's axes -- per-expert counts from GEMM_COUNTS, each the first, a middle and the last expert, E in {2, 8, 64},
    N = one, two and three column tiles, the three epilogues, the shrunk-counts rows -- with K from K4_ALL and with N and the epilogue
    rotating independently (every (N, epilogue) pair occurs for E = 2 and for E = 8)."""
    rows, i, c = [], 0, X.GEMM_COUNTS
    for E in (2, 8, 64):
        for r in range(len(c)):
            counts = tuple(c[(r + 4 * j) % 9] for j in range(2)) if E == 2 else tuple(c[(r + j) % 9] for j in range(E))
            K = K4_ALL[i % len(K4_ALL)] if E < 64 else K4_ALL[i % 3]
            rows.append(X.GRow(E, counts, (128, 256, 384)[i % 3] if E < 64 else (128, 256)[i % 2], K, X.MOE_EPIS[(i // 3) % 3]))
            i += 1
    for epi in X.MOE_EPIS:
        rows.append(X.GRow(8, (129, 40, 0, 128, 1, 257, 33, 127), 256, 192, epi, ((0, 30), (1, 16), (3, 127), (5, 0), (7, 1))))
    return rows


class Gemm4Case(X.GemmCase):
    """One vl2_moe_gemm_mxfp4 call: moe_exact.GemmCase (tables, A rows, row norms, references, frame) on an MXFP4-exact expert stack, with the
    guard of this file's docstring and the strided, poisoned (q, s) storages."""

    def __init__(self, row, seed=0):
        self.row = row
        E, alloc, N, K, epi, shrink = row
        self.E, self.N, self.K = E, N, K
        self.swiglu, self.rms = epi.startswith("swiglu"), epi.endswith("rms")
        self.n_out = n_out = N // 2 if self.swiglu else N
        given = list(alloc)
        for e, cnt in (shrink or ()):
            assert cnt < alloc[e]
            given[e] = cnt
        self.k = k = min(2, E)
        self.S = S = max(1, -(-sum(alloc) // k))
        self.P = P = X.moe_rows(S, k, E)
        offs = [0]
        for cnt in alloc:
            offs.append(offs[-1] + (cnt + MOE_BM - 1) // MOE_BM * MOE_BM)
        assert offs[-1] <= P
        self.counts, self.offs = torch.tensor(given, dtype=torch.int32), torch.tensor(offs, dtype=torch.int32)
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + E + sum(alloc) + sum(map(ord, epi)) + 4)
        wi = X4.mx4_stack(g, E, N, K)
        a = torch.full((P, K), NAN, dtype=torch.float64)
        live = torch.zeros(P, dtype=torch.bool)
        owner = torch.full((P,), -1, dtype=torch.int64)
        for e in range(E):
            a[offs[e]:offs[e] + alloc[e]] = X._ints(g, (alloc[e], K), -8, 8).double()      # the leftover rows of a shrunk expert hold numbers too
            live[offs[e]:offs[e] + given[e]] = True
            owner[offs[e]:offs[e] + given[e]] = e
        self.live, self.owner = live, owner
        rs = torch.exp2(-((torch.arange(P) * 5 + seed) % 4).double()) if self.rms else None
        rows = torch.nonzero(live).flatten()
        acc = torch.zeros((len(rows), N), dtype=torch.float64)
        mag = torch.zeros((len(rows), N), dtype=torch.float64)
        for e in range(E):
            m = owner[rows] == e
            if bool(m.any()):
                acc[m] = a[rows[m]] @ wi[e].T
                mag[m] = a[rows[m]].abs() @ wi[e].abs().T
        rs_live = rs[rows] if rs is not None else None
        sa = 1.0
        if self.swiglu and len(rows):           # A carries a power of two that brings the largest gate values to about +-8 (gemm_exact's rule)
            pre = X._epilogue(acc, rs_live, False, torch.float64).reshape(len(rows), -1, 2, 32)[:, :, 0]
            sa = 2.0 ** -max(0, math.ceil(math.log2(max(float(pre.abs().max()), 8.0) / 8.0)))
        self.sa = sa
        self.quantum = q = sa * W_UNIT * (0.125 if self.rms else 1.0)
        assert q >= 2.0 ** -20 and math.frexp(q)[0] == 0.5, f"quantum {q} is not a power of two >= 2^-20"
        pre = X._epilogue(acc * sa, rs_live, False, torch.float64)
        assert G._multiple(pre, q), "a pre-activation value is not a multiple of the quantum"
        tot = mag * sa * (rs_live[:, None] if rs_live is not None else 1.0)
        self.bound = float((tot / q).max()) if len(rows) else 0.0
        assert self.bound < 2.0 ** 24, f"exactness guard: sum of |products| / quantum = {self.bound:.0f} >= 2^24"
        self.a64, self.w64, self.wi, self.acc, self.rs_live, self.rows = a * sa, wi, wi, acc * sa, rs_live, rows
        self.ref = X._epilogue(self.acc, rs_live, self.swiglu, torch.float64)
        self.R = len(rows)
        # storages: A [P + 1, K + 8]; codes [E, N + 1, K / 2 + 16] of 0x77; scales [E, N + 1, K / 32 + 3] of 0xFF; the dequantised 16-bit stack
        # as GemmCase keeps its own ([E, N + 1, K + 8] of NaN: moe_gemm's operand of the bit-for-bit comparison); rn [P + 1, 2]
        ast = torch.full((P + 1, K + 8), NAN, dtype=torch.float32)
        ast[:P, :K] = (a * sa).float()
        qst = torch.full((E, N + 1, K // 2 + 16), 0x77, dtype=torch.uint8)
        sst = torch.full((E, N + 1, K // 32 + 3), 0xFF, dtype=torch.uint8)
        wst = torch.full((E, N + 1, K + 8), NAN, dtype=torch.float32)
        for e in range(E):
            qe, se = M4.quant_blocks(wi[e])
            qst[e, :N, :K // 2], sst[e, :N, :K // 32] = qe, se
            wst[e, :N, :K] = M4.dequant(qe, se)
        assert torch.equal(wst[:, :N, :K].double(), wi), "the stack does not survive quantise -> dequantise"
        self.store = dict(a=ast, q=qst, s=sst, w=wst)
        if self.rms:
            rn = torch.full((P + 1, 2), NAN, dtype=torch.float32)
            rn[rows, 0], rn[rows, 1] = 0.0, rs_live.float()
            self.store["rn"] = rn
        self.out_shape = (P + 2, n_out + 8)
        self.grid = (P // MOE_BM) * (N // 128)

    def coords(self):
        return super().coords().replace("moe_gemm ", "moe_gemm_mxfp4 ", 1)


def fits_fp16(c):
    """Whether the case runs unchanged on the fp16 build: A's power of two keeps every nonzero A value a normal half (>= 2^-14; the weights
    are normal halves by the rule) and every output stays below the largest half."""
    return c.sa >= 2.0 ** -14 and (c.R == 0 or float(c.ref.abs().max()) < 65504.0)


def run_gemm4(ops, c, dev, both=True):
    """-> (framed output of ops.moe_gemm_mxfp4, framed output of ops.moe_gemm on the dequantised stack or None), on the CPU."""
    el = X.elem_dtype()
    a, q, s = c.store["a"].to(el).to(dev), c.store["q"].to(dev), c.store["s"].to(dev)
    rn = c.store["rn"].to(dev) if c.rms else None
    route = dict(counts=c.counts.to(dev), offs=c.offs.to(dev))
    kw = dict(swiglu=c.swiglu, row_norm=None if rn is None else rn[:c.P], eps=EPS)
    out = torch.full(c.out_shape, SENTINEL, dtype=el, device=dev)
    ops.moe_gemm_mxfp4(a[:c.P, :c.K], q[:, :c.N, :c.K // 2], s[:, :c.N, :c.K // 32], route, c.S, c.k, out=out[1:c.P + 1, :c.n_out], **kw)
    ref = None
    if both:
        w = c.store["w"].to(el).to(dev)
        ref = torch.full(c.out_shape, SENTINEL, dtype=el, device=dev)
        ops.moe_gemm(a[:c.P, :c.K], w[:, :c.N, :c.K], route, c.S, c.k, out=ref[1:c.P + 1, :c.n_out], **kw)
        ref = ref.cpu()
    return out.cpu(), ref


def check_gemm4(c, out, ref):
    """-> (error or None, outputs one step from RNE(fp64) [SwiGLU only]): moe_exact.check_gemm (sentinels, exact / capped rows), then the
    contract: bit for bit the 16-bit grouped GEMM on the dequantised stack, sentinels included."""
    err, nd = X.check_gemm(c, out)
    if err is None and ref is not None and not torch.equal(out, ref):
        bad = torch.nonzero((out != ref) | (out.isnan() != ref.isnan()))
        r, n = bad[0].tolist()
        err = (f"{c.coords()}: {len(bad)} elements differ from moe_gemm on the dequantised stack, first at framed row {r} column {n}: "
               f"MXFP4 {out[r, n].item()!r}, 16-bit {ref[r, n].item()!r}")
    return err, nd
