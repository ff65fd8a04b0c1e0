"""TEST INFRASTRUCTURE ONLY -- exact inputs for the MXFP4 expert kernels of the MoE decode step (csrc/k_moe_mxfp4.h, the vl2_moe_*_mxfp4 entry
points): the case tables, generators, guards and references shared by tests/test_gpu_moe_mxfp4.py and tests/test_moe_mxfp4_host.py (DESIGN.md
section 22e).  Built on tests/moe_exact.py, tests/moe_fp8_exact.py and tests/mxfp4_oracle.py; what can be imported from there is imported.

THE RULE.  Expert weights are g * 2^p: g on the E2M1 grid +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, p one exponent per block of 32 k that varies over
rows, blocks and experts (`block_powers`: neighbours in every direction differ, so a wrong scale index -- expert, row or block -- changes the
output), and every non-zero block holds at least one |g| in {4, 6}.  The quantiser's exponent of such a block is floor(log2(amax)) - 2 = p and
every element scaled by 2^-p IS a grid value: nothing rounds, quantise -> dequantise returns the stack unchanged (`survives`, asserted per case
on tests/mxfp4_oracle.py) and the fp64 answer on the 16-bit stack IS the MXFP4 kernels' answer.  One block and one row of every stack that is
large enough are zero (scale byte 127, codes 0).

THE GUARDS.  Activations are small integers, so every product is a multiple of u = 0.5 * 2^pmin (the smallest non-zero |weight|); the sum of
|products| in units of u stays below 2^24 (`products_bound`, asserted per case), so every fp32 partial sum is exact in any order.  The down
cases add moe_exact.DownCase's guard for the fma chain on dyadic weights (eighths): every term is a multiple of u / 8 = 2^-4 and the sum of
magnitudes stays below 2^24 of them.

Nothing under videollama2_amd/ imports this file."""
import torch

from tests import moe_exact as X
from tests import moe_fp8_exact as X8
from tests import moe_oracle as MO
from tests import mxfp4_oracle as M4

DRow, DYADIC, _ints, _ids_for = X.DRow, X.DYADIC, X._ints, X._ids_for
fma_chain, round_f32, SKINNY4_CASES = X8.fma_chain, X8.round_f32, X8.SKINNY8_CASES
GRID = torch.tensor(M4.E2M1_VALUES, dtype=torch.float64)
BLOCK = M4.BLOCK

# csrc/k_moe_mxfp4.h MOE_MX4_DOWN_DEPTH = 8 vectors of 32 codes in flight per lane and expert: one pass of the down body covers 64 * 8 * 32 k
DOWN4_DEPTH = 8
DOWN4_K_PASS = 64 * DOWN4_DEPTH * 32          # 16384: the last one-pass K
DOWN4_K = (32, 288, 2080,                     # 1, 9, 65 vectors of 32 codes: one lane, part of one slot, lane 0's second slot
           DOWN4_K_PASS, DOWN4_K_PASS + 32)   # the pass edge, and a second pass of one vector
DOWN4_N = X.DOWN_N                            # (1, 3, 4, 5, 41)
DOWN4_K_LDS = 20480                           # K k 2 = 160 KiB exactly at k = 4
DOWN4_K_REFUSED = 20512                       # the first K % 32 == 0 beyond it
# gate/up (E, k, N, K): E in {4, 64}, k in {1, 2, 4}, N in {64, 192}, K = one vector; lane 0's second vector; the last NP = 4 shape; the first
# NP = 1 shape; the one-pass edge; the first two-pass K.  Every value of every axis occurs; the large K ride on E = 4 (the stack is E N K elements).
GU4_CASES = ((4, 1, 64, 32), (64, 2, 64, 2080), (4, 4, 192, 4096), (4, 2, 192, 4128), (64, 4, 64, 32), (4, 1, 64, 16384), (4, 2, 64, 16416),
             (64, 1, 192, 32), (4, 4, 64, 4128))
GU4_ROWS_S = 3                                # tokens of the rows form of every gate/up case


def block_powers(E, N, K):
    """p [E, N, K / 32] in {0, 1, 2}: differs between neighbouring experts, rows and blocks."""
    e, n, b = torch.meshgrid(torch.arange(E), torch.arange(N), torch.arange(K // BLOCK), indexing="ij")
    return (e + n + 2 * b) % 3


def mx4_stack(g, E, N, K, shift=0, zeros=True):
    """An MXFP4-exact expert stack [E, N, K] fp64 (the module docstring's rule) times 2^shift."""
    nb = K // BLOCK
    mag = GRID[_ints(g, (E, N, K), 0, 7)]
    w = (mag * (_ints(g, (E, N, K), 0, 1).double() * 2 - 1)).view(E, N, nb, BLOCK)
    e, n, b = torch.meshgrid(torch.arange(E), torch.arange(N), torch.arange(nb), indexing="ij")
    pos = (n + 3 * b + 5 * e) % BLOCK                                   # where the block's 4 or 6 sits
    big = torch.where((n + b + e) % 2 == 0, 4.0, 6.0) * torch.where((n + e) % 3 == 0, -1.0, 1.0)
    w.scatter_(3, pos[..., None], big.double()[..., None])
    w = (w * torch.exp2((block_powers(E, N, K) + shift).double())[..., None]).view(E, N, K).contiguous()
    if zeros:
        if K >= 2 * BLOCK:
            w[0, 0, K - BLOCK:] = 0.0                                   # one zero block (the last of expert 0's row 0)
        if N >= 3:
            w[E - 1, 1] = 0.0                                           # one zero row (expert E - 1 is always chosen)
    return w


def survives(wi):
    """wi [E, N, K] fp64 -> True when every expert comes back unchanged from tests/mxfp4_oracle.py quantise -> dequantise."""
    for e in range(wi.shape[0]):
        q, s = M4.quant_blocks(wi[e])
        if not torch.equal(M4.dequant(q, s).double(), wi[e]):
            return False
    return True


def products_bound(w_rows, a_rows):
    """max over the (weight matrix [N, K], activation row [K]) pairs of sum_k |w a| in units of the smallest non-zero |w| times the smallest
    non-zero |a| over all pairs: below 2^24 every fp32 partial sum of the products is exact in any order."""
    unit = min(float(w[w != 0].abs().min()) for w in w_rows if bool((w != 0).any())) * min(float(a[a != 0].abs().min()) for a in a_rows)
    return max(float((w.abs() @ a.abs()).max()) for w, a in zip(w_rows, a_rows)) / unit


def down4_table():
    """moe_fp8_exact.down8_table at K % 32 == 0: every K with every N (k, E and the residual rotating), every KS in 1 .. 4 at both pass counts
    with and without the residual, E = 64, the LDS limit at k = 4, and the batched entry at S in {1, 2, 5}."""
    rows, i = [], 0
    for K in DOWN4_K:
        for N in DOWN4_N:
            rows.append(DRow(1, (4, 8)[i % 2], 1 + i % 4, N, K, i % 2 == 0))
            i += 1
    for k in (1, 2, 3, 4):
        for K in (2080, DOWN4_K_PASS + 32):
            rows.append(DRow(1, 4, k, 5, K, k % 2 == 1))
            rows.append(DRow(1, 4, k, 5, K, k % 2 == 0))
    rows.append(DRow(1, 64, 4, 41, 288, True))
    rows.append(DRow(1, 4, 4, 5, DOWN4_K_LDS, True))
    for S in (1, 2, 5):
        for k, N, K in ((2, 5, 2080), (4, 41, 288), (3, 3, DOWN4_K_PASS + 32), (1, 4, 32)):
            rows.append(DRow(S, 8, k, N, K, (S + k) % 2 == 0, True))
    rows.append(DRow(2, 4, 4, 5, DOWN4_K_LDS, True, True))
    return list(dict.fromkeys(rows))


class Down4Case(X.DownCase):
    """moe_exact.DownCase on an MXFP4-exact stack: weights are multiples of 0.5, activations integers, routing weights eighths, so every term
    of the fma chain is a multiple of 2^-4 and DownCase's guard (sum of magnitudes / 2^-4 < 2^24) holds the chain; `isum` holds the dot
    products' own fp32 sums."""

    def __init__(self, row, seed=0):
        self.row = row
        S, E, k, N, K, has_res, batched = row
        assert K % BLOCK == 0
        self.S, self.E, self.k, self.N, self.K, self.batched = S, E, k, N, K, batched
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + 5 * S + k + E)
        self.ids = _ids_for(S, E, k, g)
        self.wts = torch.tensor([DYADIC[k][(t + seed) % len(DYADIC[k])] for t in range(S)], dtype=torch.float64)
        ra = 8 if K <= 2080 else 2
        a = _ints(g, (S * k, K), -ra, ra).double()
        wi = mx4_stack(g, E, N, K)
        res = _ints(g, (S, N), -64, 64).double() if has_res else None
        self.finish4(a, wi, res)

    def finish4(self, a, wi, res, guarded=True, q=2.0 ** -4):
        self._finish(a, wi, res, q, guarded=guarded)
        self.wi, self.a = wi, a
        if guarded:
            S, k = self.S, self.k
            self.isum = products_bound([wi[self.ids[t, j]] for t in range(S) for j in range(k)], [a[t * k + j] for t in range(S) for j in range(k)])
            assert self.isum < 2.0 ** 24, f"the sums of |w a| reach {self.isum:.0f} >= 2^24 units"

    @classmethod
    def order_case4(cls):
        """moe_exact.DownCase.order_case with its weights in MXFP4-exact form (K = 32, one block per row): slot 0's dot product A = -1024 +
        3 * 2^-10 is the SwiGLU row a_0 = (1024, 2^-9, 2^-10) against expert 3's weights (-1, 1, 1) = (-4, 4, 4) * 2^-2; slot 1's 1025 is
        a_1 = (1024, 1) against expert 0's (1, 1).  The slot-order argument is order_case's, word for word."""
        c = cls.__new__(cls)
        c.row = DRow(1, 4, 2, 3, 32, False)
        c.S, c.E, c.k, c.N, c.K, c.batched = 1, 4, 2, 3, 32, False
        c.ids = torch.tensor([[3, 0]])
        c.wts = torch.tensor([[1.0, 1.0 + 2.0 ** -20]], dtype=torch.float64)
        a = torch.zeros((2, 32), dtype=torch.float64)
        a[0, 0], a[0, 1], a[0, 2] = 1024.0, 2.0 ** -9, 2.0 ** -10
        a[1, 0], a[1, 1] = 1024.0, 1.0
        wi = torch.zeros((4, 3, 32), dtype=torch.float64)
        wi[3, :, 0], wi[3, :, 1], wi[3, :, 2] = -1.0, 1.0, 1.0
        wi[0, :, 0], wi[0, :, 1] = 1.0, 1.0
        c.finish4(a, wi, None, guarded=False, q=2.0 ** -20)      # not exact in any order -- that is the point (order_case)
        assert c.ref.float().bfloat16().tolist() == [[1.0078125] * 3]
        assert torch.equal(c.dots[0, 0], torch.full((3,), -1024.0 + 3 * 2.0 ** -10, dtype=torch.float64))
        assert torch.equal(c.dots[0, 1], torch.full((3,), 1025.0, dtype=torch.float64))
        return c


class GateUp4Case:
    """moe_exact.GateUpCase's inputs (RMSNorm of +-4 rows: the staged x is +-1) on an MXFP4-exact stack times a power of two that keeps the gate
    sums at a few units: the reference of the GPU test is ops.gemv_mxfp4 per slot, and this stack is what `survives` is asserted on."""

    def __init__(self, S, E, k, N, K, batched, seed=0):
        self.S, self.E, self.k, self.N, self.K, self.batched = S, E, k, N, K, batched
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + 5 * S + k + E)
        self.ids = _ids_for(S, E, k, g)
        self.x = (_ints(g, (S, K), 0, 1).double() * 2 - 1) * 4.0
        p = 1 + (K.bit_length() + 1) // 2                     # gate sums of a few units at every K: silu is not saturated, fp16 holds the products
        self.wi = mx4_stack(g, E, N, K, shift=-p)

    def bound(self):
        S, k = self.S, self.k
        return products_bound([self.wi[self.ids[t, j]] for t in range(S) for j in range(k)], [self.x[t] / 4.0 for t in range(S) for j in range(k)])


def skinny4_stack(E, N, K, seed):
    """An MXFP4-exact expert stack [E, N, K] fp64 for the grouped skinny-M cases, times 2^-5."""
    return mx4_stack(torch.Generator().manual_seed(7919 * seed + 31 * N + K), E, N, K, shift=-5)


def quant_stack(n_exp=3, N=11, K=64):
    """The quantiser's stack [E, N, K] fp32: random values, block (n, b) times 2^((n + 2b) % 5), expert e times its own magnitude 3^e / 7, one
    row and one block all zero."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn((n_exp, N, K), generator=g).view(n_exp, N, K // BLOCK, BLOCK)
    n, b = torch.meshgrid(torch.arange(N), torch.arange(K // BLOCK), indexing="ij")
    w = (w * torch.exp2(((n + 2 * b) % 5).float())[None, :, :, None]).view(n_exp, N, K)
    w = w * (3.0 ** torch.arange(n_exp).float() / 7.0)[:, None, None]
    w[1, 4] = 0.0
    w[2, 0, BLOCK:] = 0.0
    return w


# ---------------------------------------------------------------------------------------------------------------- the decoder tests' prompts
# Request i of the decoder tests is seeded on its own (DEC_SEED, i) and has 1 + 7 i mod 40 rows, so any subset is the same requests.  Model seed
# and subsets were chosen on the CPU oracle (tests/test_moe_mxfp4_host.py asserts the criterion): on requests 7, 26, 38, 41, 42 and 49 every
# routing decision of all three decode steps has margin >= 2e-2 on the original AND on the dequantised experts.
DEC_SEED, DEC_NEW = 3, 4
DEC64_CHECK = (7, 26, 38, 41, 42, 49)        # the requests of the 64-request case that get a solo reference
DEC8_IDS = DEC64_CHECK + (0, 1)              # the 8-request case; its first four run the dequantised 16-bit comparison


def dec_prompt(i, D=256):
    g = torch.Generator().manual_seed(1000 * DEC_SEED + i)
    return (0.5 * torch.randn(1 + (7 * i) % 40, D, generator=g)).bfloat16()


def dequantised_state_dict(sd, cfg):
    """sd (fp32, transformers >= 5 names) -> a copy whose expert weights are the dequantised MXFP4 copies the decoder streams.  The decoder
    quantises wgu = bf16(gate_up * g) (g = the post-attention norm weight, folded in as videollama2_amd/weights.py fold_norm does), so the
    state dict gets dequant(quant(bf16(gate_up * g))) / g: the oracle multiplies by g again (equal up to one fp32 rounding per weight)."""
    out = dict(sd)
    l = cfg["llm"]
    for i in range(l["num_hidden_layers"]):
        p = f"model.layers.{i}."
        g = sd[p + "post_attention_layernorm.weight"].bfloat16().float()
        gu, dn = sd[p + "mlp.experts.gate_up_proj"], sd[p + "mlp.experts.down_proj"]
        folded = (gu.bfloat16().float() * g[None, None, :]).bfloat16().float()
        out[p + "mlp.experts.gate_up_proj"] = torch.stack([M4.dequant(*M4.quant_blocks(folded[e])) for e in range(gu.shape[0])]) / g[None, None, :]
        out[p + "mlp.experts.down_proj"] = torch.stack([M4.dequant(*M4.quant_blocks(dn[e].bfloat16().float())) for e in range(dn.shape[0])])
    return out


def oracle_free_margins(sd, cfg, x, n_new):
    """Free-running greedy decoding on the fp32 oracle -> (tokens [n_new], margins [n_new - 1]): margins[s - 1] = the smallest top-k margin over
    the layers of the forward that turns token s - 1 into step s's logits."""
    rec, orig = [], MO.route

    def spy(h, wr, k):
        out = orig(h, wr, k)
        rec.append(MO.margins(out[2], k))
        return out
    MO.route = spy
    try:
        with torch.no_grad():
            logits, caches = MO.mixtral_forward(sd, cfg, x)
            pos, toks, res = x.shape[0], [int(logits[-1].argmax())], []
            for _ in range(n_new - 1):
                rec.clear()
                logits, caches = MO.mixtral_forward(sd, cfg, sd["model.embed_tokens.weight"][toks[-1]:toks[-1] + 1], pos, caches)
                res.append(min(float(m.min()) for m in rec))
                toks.append(int(logits[-1].argmax()))
                pos += 1
    finally:
        MO.route = orig
    return toks, res


def decidable_pairs(margins, bar=1e-2):
    """The number of leading steps of one request whose routing margin is >= bar (the GPU tests stop at the first step below it)."""
    n = 0
    for m in margins:
        if m < bar:
            break
        n += 1
    return n
