"""TEST INFRASTRUCTURE ONLY -- exact inputs for the fp8 expert kernels of the MoE decode step (csrc/k_moe_fp8.h, the vl2_moe_*_fp8 entry points):
the case tables, generators, guards and references shared by tests/test_gpu_moe_fp8.py and tests/test_moe_fp8_host.py.
Built on tests/moe_exact.py; what can be imported from there is imported.

THE RULE.  Expert weights are integers w in [-15, 15] (at most 4 significant bits) times the row's own power of two 2^(n % 5).  Under the row
rule of vl2_pack_quant_fp8 (scale 2^e, e the smallest integer with max|row| <= 448 * 2^e) such a row becomes q = w * 2^s with s >= 4 whatever
power of two multiplies the row -- a value with at most 4 significant bits at most 448, exact in e4m3fn -- so quantise -> dequantise returns the
row unchanged (`survives`, asserted per case on oracle/fp8_oracle.py) and the fp64 answer on the 16-bit stack IS the fp8 kernels' answer.  The
row powers differ between neighbouring rows and the stacks of two experts differ, so a wrong scale index (expert or row) changes the output.

THE GUARDS of the down cases (`Down8Case`), per output row n with r = n % 5: the kernel sums q a over K in fp32 -- integers, sum of magnitudes
below 2^24 (asserted on the quantised integers) -- multiplies by the scale (exact) and runs o = fma(w_j, d_j, o) on dyadic weights (eighths):
every term is a multiple of q_n = 2^(r - 3) (of min(q_n, 1) with an integer residual row) and the sum of magnitudes stays below 2^24 q_n, so
every step is exact in any order and bf16(fp64 answer) is THE output.

Nothing under videollama2_amd/ imports this file."""
from fractions import Fraction

import torch

from oracle import fp8_oracle as F8
from tests import moe_exact as X

DRow, DYADIC, _ints, _ids_for = X.DRow, X.DYADIC, X._ints, X._ids_for
ROW_POW = 5                          # row n of every expert carries 2^(n % ROW_POW)

DOWN8_K = (16, 144, 1040,            # 1, 9, 65 vectors of 16 weights: one lane, part of one slot, lane 0's second slot
           8192, 8208)               # 512 vectors: the last one-pass K; 513: a second pass of one vector
DOWN8_N = X.DOWN_N                   # (1, 3, 4, 5, 41)
DOWN8_K_LDS = 20480                  # K k 2 = 160 KiB exactly at k = 4
DOWN8_K_REFUSED = 20496              # the first K % 16 == 0 beyond it
# gate/up (E, k, N, K): E in {4, 64}, k in {1, 2, 4}, N in {64, 192}, K = one vector; lane 0's second slot; the last NP = 2 shape; the first NP = 1
# shape; the last one-pass K; the first two-pass K.  Every value of every axis occurs; the large K ride on E = 4 (the stack is E N K elements).
GU8_CASES = ((4, 1, 64, 16), (64, 2, 64, 1040), (4, 4, 192, 4096), (4, 2, 192, 4112), (64, 4, 64, 16), (4, 1, 64, 8192), (4, 2, 64, 8208),
             (64, 1, 192, 1040), (4, 4, 64, 4112))
GU8_ROWS_S = 3                       # tokens of the rows form of every gate/up case


def row_powers(N):
    return torch.exp2((torch.arange(N) % ROW_POW).double())


def survives(wi):
    """wi [E, N, K] fp64 -> True when every expert's every row comes back unchanged from oracle/fp8_oracle.py quantise -> dequantise."""
    for e in range(wi.shape[0]):
        q, s = F8.quant_rows(wi[e].float())
        if not torch.equal(F8.dequant(q, s).double(), wi[e]):
            return False
    return True


def quant_ints(wi):
    """wi [E, N, K] fp64 -> the quantised values q = w / scale as fp64 [E, N, K] (what the kernels' fp32 sums run over)."""
    return torch.stack([F8.quant_rows(wi[e].float())[0].view(torch.float8_e4m3fn).double() for e in range(wi.shape[0])])


def down8_table():
    """tests/moe_exact.py down_table at K % 16 == 0: every K with every N (k, E and the residual rotating), every KS in 1 .. 4 at both pass
    counts with and without the residual, E = 64, the LDS limit at k = 4, and the batched entry at S in {1, 2, 5}."""
    rows, i = [], 0
    for K in DOWN8_K:
        for N in DOWN8_N:
            rows.append(DRow(1, (4, 8)[i % 2], 1 + i % 4, N, K, i % 2 == 0))
            i += 1
    for k in (1, 2, 3, 4):
        for K in (1040, 8208):
            rows.append(DRow(1, 4, k, 5, K, k % 2 == 1))
            rows.append(DRow(1, 4, k, 5, K, k % 2 == 0))
    rows.append(DRow(1, 64, 4, 41, 144, True))
    rows.append(DRow(1, 4, 4, 5, DOWN8_K_LDS, True))
    for S in (1, 2, 5):
        for k, N, K in ((2, 5, 1040), (4, 41, 144), (3, 3, 8208), (1, 4, 16)):
            rows.append(DRow(S, 8, k, N, K, (S + k) % 2 == 0, True))
    rows.append(DRow(2, 4, 4, 5, DOWN8_K_LDS, True, True))
    return list(dict.fromkeys(rows))


class Down8Case(X.DownCase):
    """moe_exact.DownCase with every expert row times its power of two, and the per-row guards of this file's docstring."""

    def __init__(self, row, seed=0):
        self.row = row
        S, E, k, N, K, has_res, batched = row
        assert K % 16 == 0
        self.S, self.E, self.k, self.N, self.K, self.batched = S, E, k, N, K, batched
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + 5 * S + k + E)
        self.ids = _ids_for(S, E, k, g)
        self.wts = torch.tensor([DYADIC[k][(t + seed) % len(DYADIC[k])] for t in range(S)], dtype=torch.float64)
        ra = 8 if K <= 8192 else 2
        a = _ints(g, (S * k, K), -ra, ra).double()
        wi = _ints(g, (E, N, K), -15, 15).double() * row_powers(N)[None, :, None]
        res = _ints(g, (S, N), -64, 64).double() if has_res else None
        self.finish8(a, wi, res)

    def finish8(self, a, wi, res, guarded=True, q=0.125):
        self._finish(a, wi, res, q, guarded=False)
        self.wi, self.a = wi, a
        if not guarded:
            return
        S, k = self.S, self.k
        qi = quant_ints(wi)
        isum = torch.stack([qi[self.ids[t, j]].abs() @ a[t * k + j].abs() for t in range(S) for j in range(k)])
        assert float(isum.max()) < 2.0 ** 24, f"the integer sums of q a reach {float(isum.max()):.0f} >= 2^24"
        mags = torch.stack([torch.stack([wi[self.ids[t, j]].abs() @ a[t * k + j].abs() for j in range(k)]) for t in range(S)])
        tot = (mags * self.wts[:, :, None].abs()).sum(1) + (res.abs() if res is not None else 0.0)
        qn = row_powers(self.N) / 8.0
        if res is not None:
            qn = qn.clamp(max=1.0)
        assert bool(((self.ref / qn[None, :]) % 1.0 == 0).all()), "an output is not a multiple of its row's quantum"
        self.bound = float((tot / qn[None, :]).max())
        assert self.bound < 2.0 ** 24, f"exactness guard: sum of magnitudes / row quantum = {self.bound:.0f} >= 2^24"

    @classmethod
    def order_case8(cls):
        """moe_exact.DownCase.order_case with its weights in fp8-exact form: the magnitudes of slot 0's dot product A = -1024 + 3 * 2^-10 move
        from expert 3's rows (-1024, 2^-9, 2^-10: the small ones would vanish under the row's scale) into the SwiGLU row a_0 = (1024, 2^-9, 2^-10)
        against the weights (-1, 1, 1); slot 1 keeps (1024, 1) . (1, 1) = 1025.  The slot-order argument is order_case's, word for word."""
        c = cls.__new__(cls)
        c.row = DRow(1, 4, 2, 3, 16, False)
        c.S, c.E, c.k, c.N, c.K, c.batched = 1, 4, 2, 3, 16, False
        c.ids = torch.tensor([[3, 0]])
        c.wts = torch.tensor([[1.0, 1.0 + 2.0 ** -20]], dtype=torch.float64)
        a = torch.zeros((2, 16), dtype=torch.float64)
        a[0, 0], a[0, 1], a[0, 2] = 1024.0, 2.0 ** -9, 2.0 ** -10
        a[1, :2] = 1.0
        wi = torch.zeros((4, 3, 16), dtype=torch.float64)
        wi[3, :, 0], wi[3, :, 1], wi[3, :, 2] = -1.0, 1.0, 1.0
        wi[0, :, 0], wi[0, :, 1] = 1024.0, 1.0
        c.finish8(a, wi, None, guarded=False, q=2.0 ** -20)      # not exact in any order -- that is the point (order_case)
        assert c.ref.float().bfloat16().tolist() == [[1.0078125] * 3]
        assert torch.equal(c.dots[0, 0], torch.full((3,), -1024.0 + 3 * 2.0 ** -10, dtype=torch.float64))
        return c


class GateUp8Case(X.GateUpCase):
    """moe_exact.GateUpCase's inputs (RMSNorm of +-4 rows: the staged x is +-1) with every weight row times its power of two: the reference of the
    GPU test is ops.gemv_fp8 per slot, and this stack is what `survives` is asserted on."""

    def __init__(self, S, E, k, N, K, batched, seed=0):
        self.S, self.E, self.k, self.N, self.K, self.batched = S, E, k, N, K, batched
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + 5 * S + k + E)
        self.ids = _ids_for(S, E, k, g)
        self.x = (_ints(g, (S, K), 0, 1).double() * 2 - 1) * 4.0
        p = 4 + (K.bit_length() + 1) // 2                     # gate sums of a few units at every K: silu is not saturated, fp16 holds the products
        self.wi = _ints(g, (E, N, K), -15, 15).double() * row_powers(N)[None, :, None] * 2.0 ** -p


# the grouped skinny-M cases: per-expert counts 0, 1, 16, 17, 33 and 64 all occur (E = 8, k = 2)
SKINNY8_CASES = {"two_of_eight": (64, [64, 64, 0, 0, 0, 0, 0, 0]), "ragged": (64, [33, 17, 16, 1, 0, 30, 20, 11]),
                 "five": (5, [5, 1, 0, 2, 2, 0, 0, 0]), "seventeen": (17, [17, 16, 1, 0, 0, 0, 0, 0])}


def skinny8_stack(E, N, K, seed):
    """An fp8-exact expert stack [E, N, K] fp64 for the grouped skinny-M cases: small integers times the row powers, times 2^-6."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * N + K)
    return _ints(g, (E, N, K), -15, 15).double() * row_powers(N)[None, :, None] / 64.0


def quant_stack(n_exp=3, N=11, K=32):
    """The quantiser's stack [E, N, K] fp32: random values, row n times 2^(n % 5), expert e times its own magnitude 3^e / 7, one row all zero."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn((n_exp, N, K), generator=g) * row_powers(N).float()[None, :, None]
    w = w * (3.0 ** torch.arange(n_exp).float() / 7.0)[:, None, None]
    w[1, 4] = 0.0
    return w


def round_f32(x):
    """A Fraction -> the nearest fp32 value (ties to even) as a Fraction; normal range only (asserted)."""
    if x == 0:
        return Fraction(0)
    s, a = (-1 if x < 0 else 1), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length() - 24
    while a / Fraction(2) ** e >= 2 ** 24:
        e += 1
    while a / Fraction(2) ** e < 2 ** 23:
        e -= 1
    assert -149 <= e <= 104, "outside the normal range of fp32"
    m = a / Fraction(2) ** e
    n, r = divmod(m.numerator, m.denominator)
    if 2 * r > m.denominator or (2 * r == m.denominator and n % 2):
        n += 1
    return s * n * Fraction(2) ** e


def fma_chain(ws, ds, res):
    """o = fma(w_j, d_j, o) over the slots in order from 0, each fma rounded once to fp32 (exact rational arithmetic), then fl32(res + o)
    (res None: o itself) -> python float (exactly an fp32 value)."""
    o = Fraction(0)
    for w, d in zip(ws, ds):
        o = round_f32(Fraction(float(w)) * Fraction(float(d)) + o)
    if res is not None:
        o = round_f32(Fraction(float(res)) + o)
    return float(o)
