"""TEST INFRASTRUCTURE ONLY -- exact inputs for the tiled GEMM family (vl2_gemm: csrc/gemm_plan.h, k_gemm.h, k_gemm6/7/9.h): generators, the
exactness guards, the fp64 references, the checker and the case tables of tests/test_gpu_gemm_edges.py and tests/test_gemm_edges_host.py
(DESIGN.md section 15b).  The rule and the conventions are tests/decode_exact.py's; what can be imported from there is imported.

THE RULE.  A [M, K] and W [N, K] are small integers times powers of two, so with the common quantum q (a power of two, >= 2^-20) every product,
bias, residual and norm term is an integer multiple of q and for every output  (sum_k |a w| + |mean colsum| + |bias| + |res|) / q < 2^24
(`guard_case`, asserted per case, on top of decode_exact.guard).  Every partial sum in every association order is then exact in fp32, the fp64
reference is THE answer and every kernel form -- the 32 x 32 x 16 family, the 16 x 16 x 32 set, split-K, fp8 with power-of-two scales -- must
give it with `torch.equal`.  The magnitudes are chosen so that a good share of the bf16 outputs have more than 8 significant bits, exact ties
included (`rounding_share`): RNE at the store is tested, not bypassed.

THE EPILOGUE CONTRACT, as read from k_gemm.h (gemm_store_patch; gemm_store_tr states the same arithmetic in the same order), all in fp32:
    v = acc                                                     (SwiGLU: g, u = the 32 gate | 32 up columns of every 64-column block)
    LayerNorm:  v = fma(-mean_m, colsum_n, v) * rstd_m          RMSNorm: v = v * rstd_m          (SwiGLU: RMSNorm only, on g and u)
    fp8:        v = v * row_tab[m][1] (as the RMSNorm rstd), then v = v * col_scale_n
    SwiGLU:     v = silu(g) * u                                 else:  v = v + bias_n, then v = act(v)
    v = v + res[m][n]
    ONE rounding: RNE to bf16 at the store (fp32 output: none)
    stats_out[m][n / 64] = (sum, sum of squares) of the 64 values AS STORED (bf16), not with SwiGLU / fp32 output
    row_norm_out[m] = row_norm_finalize(stats_out)[m]; the row tickets are re-armed (zero) when the call returns
`Case.epilogue` implements exactly this, in fp64 for the reference and in fp32 for the order-independence and reference-alone tests.

Approximate pieces: the activations (QGELU, GELU, SiLU, GELU_TANH) and silu of SwiGLU: one bf16 step of RNE(fp64 value), and the number of
outputs that differ capped by decode_exact's rule, max(1, outputs // 100) (`approx_cap`).

Every operand is a strided view of a poisoned allocation (row stride > width, one extra row, NaN padding, 0x7F bytes for fp8) and every output,
stats_out and row_norm_out sits inside a SENTINEL frame.  Nothing under videollama2_amd/ imports this file."""
import math
from collections import namedtuple

import torch

from tests import decode_exact as D

SENTINEL = D.SENTINEL
EPS = 1e-5
NORM_RMS, NORM_LN = 1, 2
ACT_CODE = {None: 0, "qgelu": 1, "gelu": 2, "silu": 3, "gelu_tanh": 5}
STAGE_NO_MIX = 2                        # ops.STAGE_NO_MIX (restated: nothing of the package is imported when this module is; conv3d_index imports on call)
WS_BYTES = 1 << 28                      # what the plan shim is told; the plan reads it for the lab stamps only


def _e(**kw):
    d = dict(f32=False, bias=False, res=False, act=None, swiglu=False, norm=0, stats=False, norm_out=0, gather=False, remap=False)
    d.update(kw)
    return d


EPILOGUES = {
    "plain": _e(), "f32": _e(f32=True), "bias": _e(bias=True), "res": _e(res=True), "bias_res": _e(bias=True, res=True),
    "bias_res_f32": _e(bias=True, res=True, f32=True),
    "stats": _e(res=True, stats=True),                                   # what the o / down / out_proj / fc2 producers run
    "rms": _e(norm=NORM_RMS), "ln": _e(norm=NORM_LN, bias=True),
    "swiglu": _e(swiglu=True), "swiglu_res": _e(swiglu=True, res=True), "swiglu_rms": _e(swiglu=True, norm=NORM_RMS),
    "norm_out": _e(bias=True, res=True, stats=True, norm_out=NORM_LN), "norm_out_rms": _e(res=True, stats=True, norm_out=NORM_RMS),
    "qgelu": _e(bias=True, act="qgelu", res=True), "gelu": _e(bias=True, act="gelu"), "silu": _e(bias=True, act="silu", res=True),
    "gelu_tanh": _e(bias=True, act="gelu_tanh"),
    "gather": _e(bias=True, gather=True), "gather_silu": _e(bias=True, act="silu", gather=True),
    "remap": _e(res=True, remap=True), "remap_bias": _e(bias=True, res=True, remap=True),
}
ACTS = ("qgelu", "gelu", "silu", "gelu_tanh")
ROW_EPIS = ("plain", "bias", "res", "bias_res", "stats", "rms", "ln", "norm_out", "norm_out_rms")
SW_EPIS = ("swiglu", "swiglu_res", "swiglu_rms")
F32_EPIS = ("f32", "bias_res_f32")

# form, tile height, variant, M, N, K, epilogue; the launch controls; what the plan must answer (`forms` = every launch's form, in order)
Row = namedtuple("Row", "form th variant M N K epi mfma16 splitk split stage tile_ctr fp8 gather remap forms mode dyn",
                 defaults=(False, False, 1, 0, False, False, None, None, None, 0, 0))


def approx(row):
    e = EPILOGUES[row.epi]
    return e["swiglu"] or e["act"] is not None


def pre_amp(row):
    """The range +-amp the pre-activation values are scaled into.  silu and QuickGELU (x / (1 + e^-cx)) keep their relative accuracy over +-8.
    GELU and GELU_TANH form 1 + erf(x / sqrt 2) resp. 2 - 2 / (1 + e^2u) in fp32: an absolute error of 2^-24 on a factor that is 2.7e-3 at
    x = -3 (relative 2e-5, far inside half a bf16 step) but 6e-5 at x = -4 and 6e-7 at x = -5, where no fp32 evaluation -- torch's included --
    is within a bf16 step of the fp64 value any more: these two are tested over +-2, which the bias of +-1 widens to +-3."""
    return 2.0 if EPILOGUES[row.epi]["act"] in ("gelu", "gelu_tanh") else 8.0


# ---------------------------------------------------------------------------------------------------------------- the case tables
K_ALL = (64, 128, 192, 256,     # 1 ... 4 K-tiles: at, below and above the depth of every LDS ring (2, 3, 4 or 5 stages)
         320,                   # 5: an odd count for the two-per-trip loop of gemm_bf16_kernel
         1088)                  # 17: a long odd loop


def _grid(form, v, h, w, epis, Ks=K_ALL, Ms=None, full_at=None, **opt):
    """Every M edge of the h-row tile (1, 32, 33, h - 1, h, h + 1, 2 h + 1: a last row tile with 1, a fragment boundary +- 1 and h - 1 live rows),
    one, two and three tile widths, every K; the epilogue rotates over the grid and the full list runs once at a partial last row tile."""
    Ms = Ms or (1, 32, 33, h - 1, h, h + 1, 2 * h + 1)
    Ns = (w, 2 * w, 3 * w)
    rows, i = [], 0

    def add(M, N, K, e=None):
        nonlocal i
        if e is None:
            e = epis[i % len(epis)]
            i += 1
        rows.append(Row(form, h, v, M, N, K, e, **opt))
    for j, M in enumerate(Ms):
        add(M, Ns[j % 3], Ks[j % len(Ks)])
    for j, K in enumerate(Ks):
        add(Ms[(j + 3) % len(Ms)], Ns[(j + 1) % 3], K)
    for N in Ns:
        add(Ms[-2], N, Ks[1 % len(Ks)])
    M, N, K = full_at or (Ms[-2], w, Ks[2 % len(Ks)])
    for e in epis:
        add(M, N, K, e)
    return list(dict.fromkeys(rows))


ALL_128 = ROW_EPIS + F32_EPIS + SW_EPIS + ACTS
NO_SW = ROW_EPIS + F32_EPIS + ACTS                     # gemm7: no SwiGLU instance
SMALL_M = ROW_EPIS + ACTS                                # gemm_s: neither SwiGLU nor fp32 output
PERSIST = ("plain", "bias", "rms", "ln", "swiglu", "swiglu_rms", "gelu", "gelu_tanh")      # gemm6_ok: no residual, no statistics, bf16 output
SET16 = ROW_EPIS + SW_EPIS                               # gemm_ok16: bf16 output, no activation
SET16_ROWS = ROW_EPIS                                    # the one-round tile of the set: no SwiGLU

FAMILY = {      # test group -> rows
    # variant 1: the root of every twin-equality test of tests/test_gpu_ops.py
    "v1_128": _grid("GF_128", 1, 128, 128, ALL_128),
    "v32_64": _grid("GF_64", 32, 64, 128, SMALL_M),                          # 64 x 64 tiles; N % 128 == 0 still holds: 2, 4 and 6 tile widths
    "v256_l8": _grid("GF_L8", 256, 128, 128, ALL_128),
    "v4_128x256": _grid("GF_128x256", 4, 128, 256, ALL_128)
                  + [Row("GF_128", 128, 4, 129, 384, 128, "bias_res")],        # N % 256 != 0: the 128 x 128 kernel
    "v8_256": _grid("GF_G4_256", 8, 256, 256, ALL_128)
              + [Row("GF_128", 128, 8, 257, 384, 128, "stats")],
    "v12_192": _grid("GF_G4_192", 12, 192, 256, ROW_EPIS + SW_EPIS + ACTS)     # (fp32 output: the plan gives the 256-row form, next line)
               + [Row("GF_G4_256", 256, 12, 193, 256, 192, "f32"), Row("GF_128", 128, 12, 193, 384, 128, "ln")],
    "v224_gemm7": _grid("GF_GEMM7", 224, 224, 128, NO_SW),
    "v192_gemm7": _grid("GF_GEMM7", 192, 192, 128, NO_SW),
    # the 16 x 16 x 32 set
    "v16_gemm9": _grid("GF_GEMM9", 16, 256, 256, SET16, mfma16=False, mode=0),
    "v26_gemm9": _grid("GF_GEMM9", 26, 256, 256, SET16, mode=9),
    "v256_l8_16": _grid("GF_L8_16", 256, 128, 256, SET16_ROWS, mfma16=True),
}
# the persistent form needs K >= 1024 and M >= its tile height (gemm6_ok); 60 / 61 walk statically, 70 / 71 / 80 / 81 draw tiles from a counter block
for _v, _h, _dyn in ((60, 256, 0), (61, 192, 0), (70, 256, 1), (71, 192, 1), (80, 256, 2), (81, 192, 2)):
    FAMILY[f"v{_v}_gemm6"] = _grid("GF_GEMM6", _v, _h, 256, PERSIST, Ks=(1024, 1088), Ms=(_h, _h + 1, 2 * _h + 1), tile_ctr=_dyn > 0, dyn=_dyn)
# N % 256 != 0: forced_gemm6 answers 0 and the call is planned as the automatic choice without the persistent form -- small-M tiles, no tile from the
# counter (dyn 0).  A counter block is attached all the same: it must come back zero.
for _v, _h in ((60, 256), (61, 192), (70, 256), (71, 192), (80, 256), (81, 192)):
    FAMILY[f"v{_v}_gemm6"].append(Row("GF_64", 64, _v, _h + 1, 384, 1024, ("plain", "bias", "rms")[_v % 3], tile_ctr=True, dyn=0))

# split-K (ops.set_splitk with the workspace): tiles <= 192 and K / 64 >= 32; `split` = the factor choose_splitk answers
SPLITK_EPIS = ("plain", "f32", "bias", "res", "bias_res", "stats", "rms", "ln", "norm_out", "swiglu", "swiglu_res", "qgelu", "gelu")
SPLITK = [Row("GF_128_SPLITK", 128, v, M, N, K, SPLITK_EPIS[i % len(SPLITK_EPIS)], splitk=True, split=s)
          for i, (v, M, N, K, s) in enumerate((
              (1, 1, 128, 2048, 8), (0, 32, 256, 2048, 8), (1, 33, 128, 2048, 8), (0, 127, 256, 2048, 8), (1, 128, 128, 2048, 8), (0, 129, 256, 2048, 8),
              (1, 129, 128, 2048, 8), (0, 1, 256, 8192, 16), (1, 33, 128, 8192, 16), (0, 129, 128, 8192, 16), (1, 129, 256, 8192, 16),
              (1, 127, 128, 8192, 16), (0, 128, 256, 2048, 8)))]

# the remap form (patch embed): out_row = m + (m / grp) * 1 + 1, res_row = m % grp + 1; `remap` = (grp, groups): M = grp * groups
REMAP = [Row("GF_REMAP", 128, 0, g * n, N, K, e, remap=(g, n)) for g, n, N, K, e in (
    (50, 3, 128, 64, "remap"),          # a group boundary inside a tile, two row tiles
    (5, 7, 256, 192, "remap_bias"),     # many tiny groups
    (129, 2, 128, 320, "remap"),        # group = tile height + 1
    (128, 1, 384, 128, "remap_bias"),   # one group, one full tile
    (1, 33, 128, 256, "remap"))]        # every row its own group

# gathered A (Conv3d k2 s2 p1 as a GEMM): `gather` = (T, H, W, seg_k); M = To Ho Wo, K = 8 seg_k; taps outside the volume are -1 (zero rows)
GATHER = [Row(f, th, v, M, N, 8 * sk, e, gather=(T, H, W, sk)) for f, th, v, (T, H, W, M), N, sk, e in (
    ("GF_128", 128, 1, (4, 12, 12, 147), 128, 64, "gather"), ("GF_128", 128, 1, (2, 5, 5, 18), 256, 128, "gather_silu"),
    ("GF_64", 64, 32, (4, 12, 12, 147), 128, 128, "gather_silu"), ("GF_64", 64, 32, (3, 9, 9, 50), 256, 64, "gather"),
    ("GF_GEMM7", 224, 224, (4, 12, 16, 189), 128, 64, "gather"), ("GF_GEMM7", 224, 224, (6, 12, 12, 196), 256, 128, "gather_silu"),
    ("GF_GEMM7", 192, 192, (4, 12, 16, 189), 256, 128, "gather"), ("GF_GEMM7", 192, 192, (6, 12, 12, 196), 128, 64, "gather_silu"))]

# the fp8 forms: K in 128-byte tiles; variant 0 at these sizes is the 128 x 256 kernel (choose_gemm_kernel: at most one 128 x 128 tile per CU)
FP8_EPIS = ("plain", "f32", "bias", "res", "silu", "swiglu")
FP8_K = (128, 256, 384, 640)
FP8 = {f"fp8_v{v}": _grid(form, v, h, 256, epis, Ks=FP8_K, fp8=True)
       for v, form, h, epis in ((4, "GF_FP8_128x256", 128, FP8_EPIS), (0, "GF_FP8_128x256", 128, FP8_EPIS), (8, "GF_FP8_256", 256, FP8_EPIS),
                                (12, "GF_FP8_192", 192, tuple(e for e in FP8_EPIS if e != "f32")))}
FP8["fp8_v12"].append(Row("GF_FP8_256", 256, 12, 193, 256, 256, "f32", fp8=True))      # fp32 output has no 192-row instance

# Mixed-form shapes: reached by the automatic choice only, and only where m_split_rows splits (M >= 1024, K >= 1024, whole rounds of 256-row
# tiles + a tail of 129 ... 512 tiles of 128 x 128).  The smallest such shapes of at most 8192 rows (tests/test_gemm_edges_host.py searches them
# with the plan shim): 4609 x 4096 (16 row tiles = one round of 16-tile rows, + 513 rows = 5 x 32 tail tiles) and 2305 x 8192 (eight row tiles
# of 32-tile rows, + 257 rows = 3 x 64 tail tiles); the 16 x 16 x 32 SwiGLU row also runs 1281 x 16384 (four + 2 -> 3 x 128).
MIX_SHAPES = ((4609, 4096, 1024), (2305, 8192, 1024))
MIXED = (
    [Row("GF_MIX", 256, 0, M, N, K, e, forms=("GF_MIX",)) for (M, N, K), e in zip(MIX_SHAPES + MIX_SHAPES[:1], ("plain", "stats", "swiglu"))]
    + [Row("GF_MIX16", 256, 0, 2305, 8192, 1024, "stats", mfma16=True, forms=("GF_MIX16",), mode=0),
       Row("GF_MIX16", 256, 0, 1281, 16384, 1024, "swiglu", mfma16=True, forms=("GF_MIX16",), mode=9),       # the flag's form on SwiGLU: 64-deep phases
       Row("GF_MIX16", 256, 16, 2305, 8192, 1024, "swiglu", forms=("GF_MIX16",), mode=0),                     # variant 16: the 32-deep form
       # two launches: K >= 2048 with STAGE_NO_MIX -- 256-row tiles on the whole rounds, the chooser's pick (small-M tiles) for the 257 tail rows
       Row("GF_G4_256", 256, 0, 2305, 8192, 2048, "stats", stage=STAGE_NO_MIX, forms=("GF_G4_256", "GF_128")),
       Row("GF_G4_256", 256, 0, 2305, 8192, 2048, "swiglu", stage=STAGE_NO_MIX, forms=("GF_G4_256", "GF_128")),
       Row("GF_G4_256", 256, 0, 2305, 8192, 2048, "plain", stage=STAGE_NO_MIX, forms=("GF_G4_256", "GF_128"))])

# M independence across a tile boundary: (rows of the big call, rows of the small one), one form per instruction set
M_INDEP = (Row("GF_G4_256", 256, 8, 513, 256, 192, "bias_res"), Row("GF_GEMM9", 256, 16, 513, 256, 192, "bias_res", mode=0))
M_INDEP_M1 = 257


def all_tables():
    t = dict(FAMILY)
    t.update(FP8)
    t.update(splitk=SPLITK, remap=REMAP, gather=GATHER, mixed=MIXED)
    return t


def plan_inputs(r):
    """The columns of tests/test_gemm_plan_host.py's shim (IN_KEYS) for a table row, as vl2_gemm fills GemmPlanIn for the call run_case makes
    (the workspace is attached: tile_ctr and ws are always there)."""
    e = EPILOGUES[r.epi]
    if r.fp8:       # vl2_gemm's fp8 branch plans on M, N, K, f32 and the variant alone
        d = dict(M=r.M, N=r.N, K=r.K, f32=int(e["f32"]), fp8=1, v=r.variant)
    else:
        d = dict(M=r.M, N=r.N, K=r.K, act=int(e["act"] is not None), sw=int(e["swiglu"]), f32=int(e["f32"]), g=int(e["gather"]), remap=int(e["remap"]),
                 res=int(e["res"]), so=int(e["stats"]), norm=int(e["norm"] != 0), rn=int(e["norm"] != 0), rno=int(e["norm_out"] != 0), tctr=1, ws=1,
                 wsb=WS_BYTES, v=r.variant, splitk=int(r.splitk), nomix=int(bool(r.stage & STAGE_NO_MIX)), mfma16=int(r.mfma16), cus=256)
    return d


# ---------------------------------------------------------------------------------------------------------------- generators and guards
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)


def _pick_ranges(K, target):
    """Integer ranges (ra, rw) of A and W whose products sum to a standard deviation nearest `target` over K terms."""
    best = None
    for ra in range(1, 9):
        for rw in range(1, 16):
            s = math.sqrt(K * (ra * (ra + 1) / 3.0) * (rw * (rw + 1) / 3.0))
            if best is None or abs(s - target) < best[0]:
                best = (abs(s - target), ra, rw)
    return best[1], best[2]


def _framed(t, pad, dtype, poison, top=0):
    """t [r, c] -> storage [top + r + 1, c + pad] of `dtype` filled with `poison`, t inside at row `top`."""
    r, c = t.shape
    st = torch.full((top + r + 1, c + pad), poison, dtype=dtype)
    st[top:top + r, :c] = t.to(dtype)
    return st


def _framed1(t, pad, poison=float("nan")):
    st = torch.full((t.shape[0] + pad,), poison, dtype=torch.float32)
    st[:t.shape[0]] = t.float()
    return st


def conv3d_index(T, H, W):
    from videollama2_amd.connector import conv3d_k2s2p1_index
    idx, (To, Ho, Wo) = conv3d_k2s2p1_index(T, H, W, "cpu")
    return idx, To * Ho * Wo


def _act64(v, name):
    if name == "qgelu":
        return v * torch.sigmoid(1.702 * v)
    if name == "gelu":
        return torch.nn.functional.gelu(v)
    if name == "silu":
        return torch.nn.functional.silu(v)
    if name == "gelu_tanh":
        return torch.nn.functional.gelu(v, approximate="tanh")
    return v


def _multiple(t, q):
    return bool(((t / q) == (t / q).round()).all())


class Case:
    """One vl2_gemm call on exact inputs: the padded storages (`store`, CPU), the exact accumulators `acc` [M, N] fp64, the references
    (`expected`, `stats_ref`) and the coordinates.  dev: where the reference is computed and kept (the few large shapes: the GPU, in torch fp64)."""

    def __init__(self, row, seed=0, dev="cpu", wide=False):
        self.row, self.dev = row, dev
        e = self.e = EPILOGUES[row.epi]
        M, N, K = row.M, row.N, row.K
        self.M, self.N, self.K = M, N, K
        self.R = M                                                         # decode_exact's name for the rows of a case (swiglu_cap)
        sw = e["swiglu"]
        self.n_out = n_out = N // 2 if sw else N
        self.out_dtype = torch.float32 if e["f32"] else torch.bfloat16
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + M + 101 * row.variant + sum(map(ord, row.epi)))
        nan = float("nan")
        # ---- operand ranges: sums of about +-400 and beyond (more than 8 significant bits in a good share of the outputs); with statistics about
        # +-200, so that the sum of 64 squares stays below 2^24; approximate epilogues are rescaled below
        if wide:
            ra, rw = 8, 15
        elif e["stats"]:
            ra, rw = _pick_ranges(K, 200.0)
        elif row.fp8:
            ra, rw = (8, 15) if K <= 256 else (4, 15)
        else:
            ra, rw = (8, 15) if K <= 8192 else (2, 15)
        wi = _ints(g, (N, K), -rw, rw)
        store = {}
        if e["gather"]:
            T, H, W_, sk = row.gather
            idx, m = conv3d_index(T, H, W_)
            assert m == M and idx.shape[0] * sk == K, (m, M, idx.shape, sk, K)
            assert bool((idx < 0).any()) and bool((idx >= 0).any())
            pool = _ints(g, (T * H * W_, sk), -ra, ra)
            ai = torch.where((idx < 0)[:, :, None], torch.zeros((), dtype=torch.int64), pool[idx.clamp(min=0).long()])      # [nseg, M, sk]
            ai = ai.permute(1, 0, 2).reshape(M, K)
            self.idx, self.seg_k = idx, sk
            a_store_src = pool
        else:
            ai = _ints(g, (M, K), -ra, ra)
            a_store_src = ai
        a64, w64 = ai.double().to(dev), wi.double().to(dev)
        # ---- the norm table: integer means, per-row power-of-two rstd that differ from row to row (it need not agree with A)
        self.mu = self.rs = self.cs = None
        qn = 1.0
        if e["norm"]:
            self.rs = torch.exp2(-((torch.arange(M) * 5 + seed) % 4).double()).to(dev)           # 1, 1/2, 1/4, 1/8
            self.mu = ((torch.arange(M) * 3) % 7 - 3).double().to(dev) if e["norm"] == NORM_LN else torch.zeros(M, dtype=torch.float64, device=dev)
            if e["norm"] == NORM_LN:
                self.cs = w64.sum(1)
            qn = 0.125
        if row.fp8:     # row scale in the rstd column of the row table, one scale per weight row; neighbours differ
            self.rs = torch.exp2(((torch.arange(M) * 3) % 4 - 2).double()).to(dev)
            self.mu = torch.zeros(M, dtype=torch.float64, device=dev)
            self.col = torch.exp2(((torch.arange(N) * 5) % 4 - 2).double()).to(dev)
            qn = 2.0 ** -4
        acc = a64 @ w64.T                                                  # [M, N]: exact in fp64
        # ---- approximate epilogues: A carries a power of two that brings the pre-activation values to about +-8 (nothing saturates)
        sa = 1.0
        if approx(row):
            pre = self._pre(acc, torch.float64)
            if sw:
                pre = pre.reshape(M, -1, 2, 32)[:, :, 0]
            amp = pre_amp(row)
            sa = 2.0 ** -max(0, math.ceil(math.log2(max(float(pre.abs().max()), amp) / amp)))
            if row.fp8:
                self.rs = self.rs * sa                                     # the e4m3 codes stay integers: the scale rides in the row table
            else:
                a64, acc = a64 * sa, acc * sa
        self.sa = sa
        self.a64, self.w64, self.acc = a64, w64, acc
        q = self.quantum = min(sa * qn, 2.0 ** -3) if approx(row) else sa * qn
        rb, rr = (100, 64) if not approx(row) else (8, 16)
        self.bias = (_ints(g, (N,), -rb, rb).double() * (2.0 ** -3 if approx(row) else 1.0)).to(dev) if e["bias"] else None
        res_rows = row.remap[0] + 1 if e["remap"] else M
        self.res_tab = (_ints(g, (res_rows, n_out), -rr, rr).double() * (2.0 ** -4 if approx(row) else 1.0)).to(dev) if e["res"] else None
        self.res = None
        if e["res"]:
            self.res = self.res_tab[torch.arange(M, device=dev) % row.remap[0] + 1] if e["remap"] else self.res_tab
        self.bound = self.guard_case()
        self.ref = self.epilogue(acc, torch.float64)
        if approx(row) and e["res"]:
            # no output may cancel: where act(..) + res falls below 2^-6 the residual moves half a unit further out.  The fp32 evaluation error
            # of a term that can cancel against |res| <= 1.5 is about 1e-7; half a bf16 step of a sum of 2^-6 is 3e-5: the one-step rule holds
            # for any fp32 evaluation, the reference's or a kernel's, and not by the luck of the draw.
            near = (self.ref.abs() < 2.0 ** -6) & (self.res != 0)
            self.res_tab = self.res = torch.where(near, self.res + 0.5 * torch.sign(self.res), self.res)
            self.ref = self.epilogue(acc, torch.float64)
            assert float(self.ref.abs()[self.res != 0].min()) >= 2.0 ** -6
        # ---- storages
        if row.fp8:
            store["a"] = _framed(D.e4m3_codes(ai), 16, torch.uint8, 0x7F)
            store["w"] = _framed(D.e4m3_codes(wi), 16, torch.uint8, 0x7F)
            store["col_scale"] = _framed1(self.col.cpu(), 8)
        else:
            store["a"] = _framed((a_store_src.double() * sa), 8, torch.bfloat16, nan)
            store["w"] = _framed(wi.double(), 8, torch.bfloat16, nan)
            assert torch.equal(store["w"][:N, :K].double(), wi.double()) and torch.equal(store["a"][:a_store_src.shape[0], :a_store_src.shape[1]].double(), a_store_src.double() * sa)
        if self.rs is not None:
            tab = torch.full((M + 1, 2), nan, dtype=torch.float32)
            tab[:M, 0], tab[:M, 1] = self.mu.float().cpu(), self.rs.float().cpu()
            store["row_norm"] = tab
        if self.cs is not None:
            store["colsum"] = _framed1(self.cs.cpu(), 8)
        if self.bias is not None:
            store["bias"] = _framed1(self.bias.cpu(), 8)
        if self.res_tab is not None:
            store["res"] = _framed(self.res_tab.cpu(), 16, torch.bfloat16, nan)
            assert torch.equal(store["res"][:res_rows, :n_out].double(), self.res_tab.cpu())
        self.store = store
        self.out_rows = M + (M // row.remap[0] if e["remap"] else 0)       # rows of C the call may touch, behind the frame's first row
        self.out_shape = (self.out_rows + 2, n_out + 8)
        self.live = torch.zeros(self.out_shape, dtype=torch.bool)
        self.live[1 + self.out_row_of(torch.arange(M)), :n_out] = True
        if e["stats"]:
            self.stats_bound = self.guard_stats()

    # ---- the epilogue contract (module docstring), in `dt` = fp64 (the reference) or fp32 (order independence, the reference alone)
    def _pre(self, acc, dt):
        """acc -> the value the activation / SwiGLU sees, without the bias."""
        v = acc.to(dt)
        if self.e["norm"] == NORM_LN:
            v = (v - self.mu.to(dt)[:, None] * self.cs.to(dt)[None, :]) * self.rs.to(dt)[:, None]
        elif self.rs is not None:
            v = v * self.rs.to(dt)[:, None]
        if self.row.fp8:
            v = v * self.col.to(dt)[None, :]
        return v

    def epilogue(self, acc, dt):
        v = self._pre(acc, dt)
        if self.e["swiglu"]:
            y = v.reshape(self.M, -1, 2, 32)
            v = (torch.nn.functional.silu(y[:, :, 0]) * y[:, :, 1]).reshape(self.M, -1)
        else:
            if self.bias is not None:
                v = v + self.bias.to(dt)
            v = _act64(v, self.e["act"])
        if self.res is not None:
            v = v + self.res.to(dt)
        return v

    def guard_case(self):
        """decode_exact.guard on (A, W, bias, res) where it applies unchanged, then the same rule with the norm / scale terms: every value the
        epilogue forms before the activation is a multiple of the case's quantum and the sum of magnitudes / quantum stays below 2^24."""
        q, a, w = self.quantum, self.a64, self.w64
        assert q >= 2.0 ** -20 and math.frexp(q)[0] == 0.5, f"quantum {q} is not a power of two >= 2^-20"
        ap = approx(self.row)
        if self.rs is None and self.dev == "cpu":                          # no norm / scale term: decode_exact's guard as it stands (A's quantum = q)
            D.guard(w, a, None if ap else self.bias, None if ap else self.res, 1.0, q if not ap else self.sa)
        total = a.abs() @ w.abs().T
        if self.e["norm"] == NORM_LN:
            total = total + self.mu.abs()[:, None] * self.cs.abs()[None, :]
        if self.rs is not None:
            total = total * self.rs[:, None]
        if self.row.fp8:
            total = total * self.col[None, :]
        pre = self._pre(self.acc, torch.float64)
        assert _multiple(pre, q), "a pre-activation value is not a multiple of the quantum"
        if not ap:                                                         # (approximate epilogues: bias and residual join behind the exact part)
            for name, t in (("bias", self.bias), ("res", self.res)):
                if t is not None:
                    assert _multiple(t, q), f"{name} is not a multiple of the quantum"
                    total = total + t.abs()
        elif self.bias is not None:
            assert _multiple(self.bias, q)
            total = total + self.bias.abs()
        bound = float((total / q).max())
        assert bound < 2.0 ** 24, f"exactness guard: sum of magnitudes / quantum = {bound:.0f} >= 2^24"
        return bound

    def guard_stats(self):
        """The second guard: per row and 64-column block of the STORED output, sum |y| / q and sum y^2 / q^2 stay below 2^24 -- the statistics
        are exact in fp32 in any order as well."""
        y = self.expected().double().reshape(self.M, -1, 64)
        q = self.quantum
        assert _multiple(y, q)
        b = max(float((y.abs().sum(-1) / q).max()), float(((y * y).sum(-1) / (q * q)).max()))
        assert b < 2.0 ** 24, f"statistics guard: sum of squares / quantum^2 = {b:.0f} >= 2^24"
        return b

    def out_row_of(self, m):
        if self.e["remap"]:
            return m + (m // self.row.remap[0]) + 1
        return m

    def coords(self):
        r = self.row
        extra = "".join(f" {k}" for k, on in (("mfma16", r.mfma16), ("splitk", r.splitk), ("fp8", r.fp8), ("no_mix", r.stage & STAGE_NO_MIX)) if on)
        return f"{r.form}/v{r.variant}{extra} M={r.M} N={r.N} K={r.K} {r.epi}"

    def expected(self, ref=None):
        """THE output [M, n_out] in the output type: the fp64 value rounded once (approximate epilogues: compared to one step by check_case)."""
        ref = self.ref if ref is None else ref
        return ref.float() if self.e["f32"] else ref.float().bfloat16()

    def stats_ref(self, stored=None):
        """(sum, sum of squares) per row and 64-column block of the stored output, fp64 -> fp32 [M, N / 64, 2] (exact under guard_stats)."""
        y = (self.expected() if stored is None else stored).double().reshape(self.M, -1, 64)
        return torch.stack((y.sum(-1), (y * y).sum(-1)), -1).float()

    def rounding_share(self):
        """(share of the bf16 outputs whose fp64 value is not a bf16 number, number of exact ties among them)."""
        r64 = self.ref
        lo = r64.float().bfloat16().double()
        inexact = lo != r64
        # an exact tie: the value sits half-way between two neighbouring bf16 numbers
        step = torch.exp2(torch.floor(torch.log2(r64.abs().clamp(min=1e-30))) - 7)
        ties = inexact & (((r64 / step) % 1.0) == 0.5)
        return float(inexact.double().mean()), int(ties.sum())

    def perfect(self):
        """What a correct kernel leaves behind, in the layout of run_case's snapshots (for the planted-fault tests)."""
        out = torch.full(self.out_shape, SENTINEL, dtype=self.out_dtype)
        out[1 + self.out_row_of(torch.arange(self.M)), :self.n_out] = self.expected().cpu()
        snap = dict(out=out)
        if self.e["stats"]:
            st = torch.full((self.M + 2, self.N // 64, 2), SENTINEL, dtype=torch.float32)
            st[1:self.M + 1] = self.stats_ref().cpu()
            snap["stats"] = st
        if self.e["norm_out"]:      # (mean, rstd) in fp64 -> fp32 stands in for row_norm_finalize, which is a kernel: check_case compares rn with rn_ref only
            y = self.expected().double()
            mean = y.mean(1) if self.e["norm_out"] == NORM_LN else torch.zeros(self.M, dtype=torch.float64)
            rstd = torch.rsqrt((y * y).mean(1) - mean * mean + EPS)
            snap["rn_ref"] = torch.stack((mean, rstd), 1).float().cpu()
            rn = torch.full((self.M + 2, 2), SENTINEL, dtype=torch.float32)
            rn[1:self.M + 1] = snap["rn_ref"]
            snap["rn"], snap["tick"] = rn, torch.zeros(self.M // 64 + 2, dtype=torch.int32)
        if self.row.tile_ctr:
            snap["ctr"] = torch.zeros(16, dtype=torch.int32)
        return snap


def approx_cap(c):
    """decode_exact.swiglu_cap itself (max(1, outputs // 100)): it reads c.n_out and c.R, the rows of the case."""
    return D.swiglu_cap(c)


def run_case(ops, c, dev, reps=2, m_rows=None):
    """Run case `c` through ops.gemm / ops.gemm_fp8 on `dev`, `reps` times on the SAME buffers, with strided views of the poisoned storages; the
    forced variant, the stage flags and split-K are restored in `finally`.  -> one snapshot per repetition: dict(out, stats, rn, rn_ref, tick, ctr),
    whole storages, on c.dev.  m_rows: the call on the first m_rows rows only (plain rows, no statistics: the M-independence test)."""
    r, e = c.row, c.e
    M, N, K, n_out = c.M, c.N, c.K, c.n_out
    st = {k: v.to(dev) for k, v in c.store.items()}
    out_st = torch.full(c.out_shape, SENTINEL, dtype=c.out_dtype, device=dev)
    out = out_st[1:1 + c.out_rows, :n_out]
    if m_rows is not None:
        assert not (e["stats"] or e["gather"] or e["remap"] or r.fp8 or e["norm"])
        M, out = m_rows, out[:m_rows]
    kw = dict(swiglu=e["swiglu"], out_f32=e["f32"], act=ACT_CODE[e["act"]], out=out)
    if e["bias"]:
        kw["bias"] = st["bias"][:N]
    if e["res"]:
        kw["res"] = st["res"][:c.res_tab.shape[0] if m_rows is None else m_rows, :n_out]
    stats_st = rn_st = tick = ctr = rn_ref = None
    if not r.fp8:
        if e["norm"]:
            kw["norm"] = (e["norm"], st["row_norm"][:M], EPS, st["colsum"][:N] if e["norm"] == NORM_LN else None)
        if e["stats"]:
            stats_st = torch.full((M + 2, N // 64, 2), SENTINEL, dtype=torch.float32, device=dev)
            kw["stats_out"] = stats_st[1:M + 1]
        if e["norm_out"]:
            rn_st = torch.full((M + 2, 2), SENTINEL, dtype=torch.float32, device=dev)
            tick = torch.zeros(M // 64 + 2, dtype=torch.int32, device=dev)
            kw["norm_out"] = (e["norm_out"], EPS, rn_st[1:M + 1], tick)
            rn_ref = ops.row_norm_finalize(c.stats_ref().to(dev).contiguous(), N, e["norm_out"], EPS)
        if r.tile_ctr:
            ctr = torch.zeros(16, dtype=torch.int32, device=dev)
            kw["tile_ctr"] = ctr
        if e["gather"]:
            kw["gather"] = (c.idx.to(dev), None, c.seg_k)
        if e["remap"]:
            kw["out_map"], kw["res_map"] = (r.remap[0], 1, 1), (r.remap[0], 1)
        kw["mfma16"] = r.mfma16
    snaps = []
    try:
        ops.set_gemm_variant(r.variant)
        ops.set_stage_flags(r.stage)
        ops.set_splitk(r.splitk)
        for _ in range(reps):
            if r.fp8:
                fk = {k: v for k, v in kw.items() if k in ("bias", "res", "act", "swiglu", "out_f32", "out")}
                ops.gemm_fp8(st["a"][:M, :K], st["row_norm"][:M], st["w"][:N, :K], st["col_scale"][:N], **fk)
            else:
                a = st["a"][:c.store["a"].shape[0] - 1 if m_rows is None else m_rows, :c.store["a"].shape[1] - 8]
                ops.gemm(a, st["w"][:N, :K], **kw)
            snap = dict(out=out_st.clone(), stats=stats_st, rn=rn_st, tick=tick, ctr=ctr, rn_ref=rn_ref)
            snaps.append({k: (v.clone().to(c.dev) if v is not None else None) for k, v in snap.items()})
    finally:
        ops.set_gemm_variant(0)
        ops.set_stage_flags(0)
        ops.set_splitk(False)
    return snaps


def same_bits(s1, s2):
    """Two snapshots agree bit for bit (every buffer the call wrote)."""
    for k in ("out", "stats", "rn"):
        a, b = s1.get(k), s2.get(k)
        if a is not None:
            va = a.contiguous().view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32)
            vb = b.contiguous().view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)
            if not torch.equal(va, vb):
                return False
    return True


def _frame_intact(buf, live):
    keep = torch.full_like(buf, SENTINEL)
    return bool((buf[~live] == keep[~live]).all())


def check_case(c, snap):
    """-> (error message or None, number of outputs that differ from the rounded fp64 value [approximate epilogues only])."""
    out_st = snap["out"]
    live = c.live.to(out_st.device)
    if not _frame_intact(out_st, live):
        bad = torch.nonzero((out_st != SENTINEL) & ~live)
        return f"{c.coords()}: canary overwritten at {[tuple(i) for i in bad[:4].tolist()]} of the framed output {tuple(out_st.shape)}", 0
    y = out_st[1 + c.out_row_of(torch.arange(c.M, device=out_st.device)), :c.n_out]
    exp = c.expected()
    nd = 0
    if not approx(c.row):
        if not torch.equal(y, exp):
            diff = torch.nonzero((y != exp) | y.isnan())
            m, n = diff[0].tolist()
            return (f"{c.coords()}: {len(diff)} of {y.numel()} outputs differ, first at row {m} column {n}: got {y[m, n].item()!r}, "
                    f"exact {exp[m, n].item()!r}"), len(diff)
    else:
        if bool(y.isnan().any()):
            return f"{c.coords()}: NaN in the output (a poisoned pad was read)", int(y.isnan().sum())
        d = D.ulp_distance(y, exp)
        nd = int((d > 0).sum())
        if int(d.max()) > 1:
            m, n = torch.nonzero(d > 1)[0].tolist()
            return f"{c.coords()}: row {m} column {n} is {int(d[m, n])} bf16 steps from RNE of the fp64 value: got {y[m, n].item()!r}, exact {exp[m, n].item()!r}", nd
        if nd > approx_cap(c):
            return f"{c.coords()}: {nd} outputs differ from RNE of the fp64 value by one step, cap {approx_cap(c)}", nd
    if c.e["stats"]:
        s = snap["stats"]
        if not (bool((s[0] == SENTINEL).all()) and bool((s[-1] == SENTINEL).all())):
            return f"{c.coords()}: the frame of stats_out was overwritten", nd
        ref = c.stats_ref().to(s.device)
        if not torch.equal(s[1:-1], ref):
            m, b, k = torch.nonzero(s[1:-1] != ref)[0].tolist()
            return f"{c.coords()}: stats_out row {m} block {b} [{k}] is {s[1 + m, b, k].item()!r}, exact {ref[m, b, k].item()!r}", nd
    if c.e["norm_out"] and snap.get("rn") is not None:
        rn, ref = snap["rn"], snap["rn_ref"]
        if not (bool((rn[0] == SENTINEL).all()) and bool((rn[-1] == SENTINEL).all())):
            return f"{c.coords()}: the frame of row_norm_out was overwritten", nd
        if not torch.equal(rn[1:-1], ref):
            m = torch.nonzero((rn[1:-1] != ref).any(1))[0].item()
            return f"{c.coords()}: row_norm_out row {m} is {rn[1 + m].tolist()}, row_norm_finalize of the exact statistics {ref[m].tolist()}", nd
        if int(snap["tick"].abs().sum()) != 0:
            return f"{c.coords()}: the row tickets were not re-armed", nd
    if snap.get("ctr") is not None and int(snap["ctr"].abs().sum()) != 0:
        return f"{c.coords()}: the tile counter block was not re-armed: {snap['ctr'][:4].tolist()}", nd
    return None, nd


def reference_alone_share(c):
    """The reference alone: the epilogue in torch fp32 on the exact accumulators against the fp64 one -> (outputs that differ, largest distance)."""
    d = D.ulp_distance(c.expected(c.epilogue(c.acc.float(), torch.float32).double()), c.expected())
    return int((d > 0).sum()), int(d.max())


def acc_in_other_orders(c):
    """The accumulators summed in fp32 in three other associations: 16-wide steps forwards, 32-wide steps with the 64-element tiles in reverse
    order, and d = 3 partial sums over thirds of the K-tiles added at the end (split-K's shape)."""
    a, w = c.a64.float(), c.w64.float()
    K = c.K

    def chain(bounds):
        s = torch.zeros((c.M, c.N), dtype=torch.float32)
        for lo, hi in bounds:
            s = s + a[:, lo:hi] @ w[:, lo:hi].T
        return s
    f16 = chain([(k, k + 16) for k in range(0, K, 16)])
    r32 = chain([(k, k + 32) for k in range(K - 32, -1, -32)])
    nt = K // 64
    cuts = [0, (nt + 2) // 3 * 64, (2 * nt + 2) // 3 * 64, K]
    parts = [chain([(k, k + 64) for k in range(cuts[i], cuts[i + 1], 64)]) for i in range(3)]
    return f16, r32, (parts[0] + parts[1]) + parts[2]
