"""TEST INFRASTRUCTURE ONLY -- exact inputs for the decode projections (GEMV, multi-row GEMV, skinny-M GEMM on 16-bit, fp8 and MXFP4 weights):
generators, the exactness guard, the fp64 references and the case tables of tests/test_gpu_decode_edges.py and tests/test_decode_edges_emu.py
(DESIGN.md section 15).

THE RULE.  Operands are small integers times powers of two.  With a common quantum q (a power of two, >= 2^-20) every product w[n][k] x[k], every
bias and every residual is an integer multiple of q, and for every output n

    (sum_k |w[n][k] x[k]| + |bias[n]| + |res[n]|) / q  <  2^24                                                       (`guard`, asserted per case)

so every partial sum in every association order is an integer multiple of q below 2^24 q: exactly representable in fp32.  The fp64 reference is
then THE answer, and a projection output is compared with `torch.equal` -- no tolerance.  (Only silu of the SwiGLU epilogue and the statistic of
the staged-x probe are approximate; their one-ulp rules and caps are `swiglu_cap` and `probe_cap`.)

Every operand is allocated with a row stride larger than its width plus one extra row, the padding poisoned (NaN elements, 0x7F fp8 bytes, 0xFF
scale bytes, 0x77 code bytes: all inside the allocation, so an over-read shows as a NaN or a wrong number), and the output pre-filled with a
sentinel that must survive everywhere outside [rows, n_out].

Nothing under videollama2_amd/ imports this file."""
import math

import torch

from oracle import fp8_oracle as F8
from tests import mxfp4_oracle as M4

SENTINEL = -777.0
EPS = 1e-5
GEMV_RMS_PLAIN, GEMM_SWIGLU, GEMM_OUT_F32 = 32, 1, 2
FORMATS = ("b16", "fp8", "mx4")
NL = {"b16": 8, "fp8": 16, "mx4": 16}              # weight words in flight per lane of gemm_skinny_body (k_skinny.h, k_skinny_fp8.h, k_mxfp4.h)

# epilogue name -> (norm, swiglu, out_f32, bias, res)
EPILOGUES = {
    "plain": (None, False, False, False, False), "f32": (None, False, True, False, False), "bias": (None, False, False, True, False),
    "res": (None, False, False, False, True), "bias_res": (None, False, True, True, True), "norm_w": ("w", False, False, False, False),
    "rms_plain": ("plain", False, True, False, False), "swiglu": (None, True, False, False, False),
    "swiglu_res": (None, True, False, False, True), "swiglu_norm": ("w", True, False, False, False),
}
ROW_EPIS = ("plain", "f32", "bias", "res", "bias_res", "norm_w", "rms_plain")
SW_EPIS = ("swiglu", "swiglu_res", "swiglu_norm")
SKINNY_ROW_EPIS = ("plain", "f32", "bias", "res", "bias_res")
SKINNY_SW_EPIS = ("swiglu", "swiglu_res")


# ---------------------------------------------------------------------------------------------------------------- the case tables
# Single-row GEMV.  K (why), from k_decode.h / k_fp8.h / k_mxfp4.h and the launchers of vl2_abi.hip:
GEMV_K = {
    # 16-B vector = 8 k; 512 vectors per pass; x-first kernel iff a norm and K <= 4096
    "b16": (8,          # one vector
            72,         # 9 vectors: part of one slot
            520,        # 65 vectors: second slot, one lane
            2056,       # 257 vectors: second x register of the x-first kernel / second trip of gemv_stage_x hold one vector
            4096,       # 512 vectors: last one-pass, last x-first
            4104,       # 513: second pass of one vector; a norm now runs gemv_bf16_kernel
            32704),     # the maximum (x fills the LDS)
    # vector = 16 k; NP = 2, 4 slots for K <= 4096, else NP = 1, 8 slots
    "fp8": (16, 1040,   # one vector; 65 vectors
            4096,       # 256 vectors: last NP = 2, its one pass full
            4112,       # first NP = 1
            8192,       # 512 vectors: last one-pass of NP = 1
            8208,       # 513: a second pass of one vector
            32704),
    # vector = 32 k = one scale block; NP = 4, 2 slots for K <= 4096, else NP = 1, 8 slots
    "mx4": (32, 2080,   # one vector; 65 vectors
            4096,       # 128 vectors: last NP = 4
            4128,       # first NP = 1
            16384,      # 512 vectors: last one-pass
            16416,      # 513
            32704),
}
GEMV_N = {
    "b16": (1, 3, 4, 5, 41),        # one row per wave, four per workgroup: part of a workgroup, a full one, one row into the second, eleven
    "fp8": (2, 6, 10, 18, 34),      # pairs.  NP = 2: 6 = wave 1 has one live and one dead pair; 18 = the second workgroup has one pair; NP = 1: other tails
    "mx4": (2, 6, 10, 34),          # 16 pairs per workgroup at NP = 4; 34 = 17 pairs
}
GEMV_N_SWIGLU = (64, 192)           # packed rows: one and three 64-row blocks
# the regimes in which the FULL epilogue list runs once: (K, N rows, N swiglu)
GEMV_REGIMES = {
    "b16": ((2056, 5, 64),          # one pass; with a norm: x-first
            (4104, 5, 64)),         # two passes; with a norm: not x-first      (without a norm both are gemv_bf16_kernel: covered by the same lists)
    "fp8": ((1040, 6, 64), (8208, 6, 64)),
    "mx4": ((2080, 6, 64), (16416, 6, 64)),
}


def gemv_cases(fmt):
    """[(K, N, epilogue)]: every K with every N, the epilogue rotating; the SwiGLU widths with every K; the full list once per regime."""
    out, i = [], 0
    for K in GEMV_K[fmt]:
        for N in GEMV_N[fmt]:
            out.append((K, N, ROW_EPIS[i % len(ROW_EPIS)]))
            i += 1
    i = 0
    for K in GEMV_K[fmt]:
        for N in GEMV_N_SWIGLU:
            out.append((K, N, SW_EPIS[i % len(SW_EPIS)]))
            i += 1
    for K, N, Nsw in GEMV_REGIMES[fmt]:
        out += [(K, N, e) for e in ROW_EPIS] + [(K, Nsw, e) for e in SW_EPIS]
    return list(dict.fromkeys(out))


# Batched GEMV.  MB rows of x; the launchers take cap = min(4, LDS / (2 K)) rows per launch.
BATCH_MB = (1, 2, 3, 4, 5, 7)
BATCH_K = {"b16": (8, 520, 4096, 4104), "fp8": (16, 1040, 4096, 4112), "mx4": (32, 2080, 4096, 4128)}     # smallest, 65 vectors, 4096, first above
BATCH_N = {"b16": (1, 7, 8, 9, 41),     # two rows per wave, eight per workgroup: 1, 7, 9 = a wave with its first row live and its second dead
           "fp8": GEMV_N["fp8"], "mx4": GEMV_N["mx4"]}
BATCH_LDS = {                           # (K, MB): the LDS splits
    "b16": ((8192, 4),                  # exactly 64 KiB of x beside the static red[MB][4]
            (8200, 4),                  # cap 3: 3 + 1, a multi-row and a single-row launch in one call
            (16384, 4), (16384, 5),     # cap 2: 2 + 2, 2 + 2 + 1
            (32704, 2), (32704, 3)),    # cap 1
    "fp8": ((8192, 4), (8208, 4), (16384, 4), (16384, 5), (32704, 2), (32704, 3)),
    "mx4": ((8192, 4),                  # 3 + 1: the launcher reserves 64 B for red
            (8224, 4), (16384, 3),      # cap 1 at 16384
            (32704, 2)),
}


def batched_cases(fmt):
    """[(MB, K, N, epilogue)]: MB x K with N and the epilogue rotating, MB x N at the smallest K, the LDS splits."""
    epis = tuple(e for e in ROW_EPIS + SW_EPIS if not (fmt == "b16" and e == "rms_plain"))      # the 16-bit batched entry has no rms_plain form
    out, i = [], 0

    def add(MB, K, N):
        nonlocal i
        e = epis[i % len(epis)]
        i += 1
        out.append((MB, K, GEMV_N_SWIGLU[i % 2] if EPILOGUES[e][1] else N, e))
    Ns = BATCH_N[fmt]
    for MB in BATCH_MB:
        for K in BATCH_K[fmt]:
            add(MB, K, Ns[i % len(Ns)])
    for MB in BATCH_MB:
        for N in Ns:
            out.append((MB, BATCH_K[fmt][0], N, ROW_EPIS[i % 5]))
            i += 1
    for K, MB in BATCH_LDS[fmt]:
        add(MB, K, Ns[i % len(Ns)])
        add(MB, K, Ns[i % len(Ns)])
    return list(dict.fromkeys(out))


# Skinny-M GEMM.
SKINNY_M = (1, 15, 16, 17, 32, 33, 64)
SKINNY_NK = (
    (64, 32, None),         # one step, split 1
    (64, 96, None),         # split 3: slices of one step
    (64, 1184, None),       # 37 steps, a prime: split 1; M <= 16 one chunk of 37 = 4 * 8 + 5 = 2 * 16 + 5 steps, M > 16 the LDS limit forces 37 one-step chunks
    (64, 2368, None),       # split 2, slices of 1184
    (192, 4128, None),      # 129 = 3 * 43 steps: split 3
    (128, 8192, "swiglu"),  # split 32, slices of 8 steps = NL (16-bit), < NL (fp8, MXFP4)
    (256, 512, "swiglu_res"),   # split 16, one step
    (8192, 64, "all"),      # wide N, split 2
    (64, 16384, None),      # 512 steps, split 32: slices of 16 steps = NL (fp8, MXFP4), 2 NL (16-bit); at M > 32 the LDS limit makes two chunks of 8
    (64, 5120, None),       # 160 steps, split 32: slices of 5 steps < NL for every format
)


def skinny_plan(M, N, K, ws_bytes=1 << 40, shrink=False, lds_cap=65536):
    """csrc/skinny_plan.h restated (tests/test_decode_edges_emu.py holds it against the header): mt, ks, kslice, kchunk, ws_need.  shrink = the
    16-bit entry's rule: a split whose partials exceed the workspace of `ws_bytes` is made smaller until they fit."""
    mt = 1 if M <= 16 else 2 if M <= 32 else 4
    Mp, steps = 16 * mt, K // 32
    ks = max(1, min(32, (4096 + N // 16 - 1) // (N // 16)))
    while ks > 1 and (steps % ks or (shrink and ks * Mp * N * 4 > ws_bytes)):
        ks -= 1
    kslice = K // ks
    kchunk = kslice
    while kchunk > 32 and (kslice % kchunk or kchunk % 32 or Mp * (kchunk + 8) * 2 > lds_cap):
        kchunk -= 32
    return dict(mt=mt, ks=ks, kslice=kslice, kchunk=kchunk, ws_need=ks * Mp * N * 4)


def skinny_cases():
    """[(M, N, K, epilogue)]: every M with every (N, K)."""
    out, i = [], 0
    for N, K, kind in SKINNY_NK:
        for M in SKINNY_M:
            if kind in ("swiglu", "swiglu_res"):
                e = kind
            elif kind == "all":
                e = (SKINNY_ROW_EPIS + SKINNY_SW_EPIS)[i % 7]
            else:
                e = SKINNY_ROW_EPIS[i % 5]
            i += 1
            out.append((M, N, K, e))
    return out


# ---------------------------------------------------------------------------------------------------------------- generators
def _ints(g, shape, lo, hi, nonzero=False):
    t = torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64)
    if nonzero:
        t = torch.where(t == 0, torch.full_like(t, hi), t)
    return t


_E4M3_OF_INT = None


def e4m3_codes(ints):
    """integers in [-15, 15] (at most four significant bits: exact in e4m3fn) -> bytes, through oracle.fp8_oracle.e4m3fn_encode."""
    global _E4M3_OF_INT
    if _E4M3_OF_INT is None:
        _E4M3_OF_INT = torch.tensor([F8.e4m3fn_encode(float(v)) for v in range(-15, 16)], dtype=torch.uint8)
    assert int(ints.abs().max()) <= 15
    return _E4M3_OF_INT[ints + 15]


def ranges(fmt, K, wide=False):
    """The value ranges per format and K, narrowed so that the guard holds for every K the entry points accept (wide=True: the narrowing off,
    for the unit test that shows the guard firing)."""
    r = dict(w=15, x=8, res=64, bias=100, e=(-3, 2), sb=(125, 129))
    if wide:
        return r
    if fmt == "fp8" and K > 4096:       # 15 * 2^(2 + 3) * 8 * K < 2^24 needs K <= 4369
        r.update(x=2, e=(-1, 1))        # 15 * 4 * 2 * 32704 = 3.9 M
    if fmt == "mx4":
        if K > 8224:                    # 12 * 2^4 * 8 * K < 2^24 needs K <= 10922
            r.update(x=2)               # 12 * 16 * 2 * 32704 = 12.6 M
    return r


class Weights:
    """One weight matrix [N, K] in its padded, poisoned storage.  `store` = the tensors the kernel reads (views are cut by `views`), `w64` = the
    dequantised matrix in fp64, `quantum` = the power of two every element is a multiple of."""

    def __init__(self, fmt, N, K, g, swiglu=False, wide=False, shift=0):
        self.fmt, self.N, self.K = fmt, N, K
        r = ranges(fmt, K, wide)
        nan16 = float("nan")
        if fmt == "b16":
            wi = _ints(g, (N, K), -r["w"], r["w"])
            self.quantum = 2.0 ** shift
            self.w64 = wi.double() * self.quantum
            st = torch.full((N + 1, K + 8), nan16, dtype=torch.bfloat16)
            st[:N, :K] = self.w64.bfloat16()
            self.store = dict(w=st)
        elif fmt == "fp8":
            wi = _ints(g, (N, K), -r["w"], r["w"])
            lo, hi = r["e"]
            e = _ints(g, (N,), lo, hi)
            n = torch.arange(N)
            mate = (n - 32) if swiglu else (n - 1)                   # the other row of the pair (gemv_pair_rows): its scale must differ
            second = ((n % 64) >= 32) if swiglu else (n % 2 == 1)
            for i in torch.nonzero(second).flatten().tolist():
                if e[i] == e[mate[i]]:
                    e[i] = lo + (e[i] - lo + 1) % (hi - lo + 1)
            self.quantum = 2.0 ** lo
            self.scale = torch.exp2(e.double())
            self.w64 = wi.double() * self.scale[:, None]
            q = torch.full((N + 1, K + 16), 0x7F, dtype=torch.uint8)
            q[:N, :K] = e4m3_codes(wi)
            sc = torch.full((N + 1,), nan16, dtype=torch.float32)
            sc[:N] = self.scale.float()
            self.store = dict(q=q, scale=sc)
        else:
            codes = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
            lo, hi = r["sb"]
            span = hi - lo + 1                                        # a random walk with steps 1 .. span - 1 (mod span): neighbouring blocks of a row differ
            walk = torch.randint(1, span, (N, K // 32), generator=g, dtype=torch.int64).cumsum(dim=1)
            sb = lo + (walk + torch.randint(0, span, (N, 1), generator=g, dtype=torch.int64)) % span
            sb = sb.to(torch.uint8)
            q = torch.full((N + 1, K // 2 + 16), 0x77, dtype=torch.uint8)
            q[:N, :K // 2] = codes[:, 0::2] | (codes[:, 1::2] << 4)
            s = torch.full((N + 1, K // 32 + 3), 0xFF, dtype=torch.uint8)
            s[:N, :K // 32] = sb
            self.quantum = 0.5 * 2.0 ** (lo - 127)
            self.w64 = M4.dequant(q[:N, :K // 2], s[:N, :K // 32]).double()
            self.store = dict(q=q, s=s)

    def to(self, dev):
        return {k: v.to(dev) for k, v in self.store.items()}


def weight_views(fmt, st, N, K):
    if fmt == "b16":
        return (st["w"][:N, :K],)
    if fmt == "fp8":
        return (st["q"][:N, :K], st["scale"][:N])
    return (st["q"][:N, :K // 2], st["s"][:N, :K // 32])


def guard(w64, xs64, bias64, res64, qw, qx):
    """The exactness guard, in fp64: w [N, K] multiples of qw, xs [R, K] (the staged x rows) multiples of qx, bias [N] / res [R, N] (or None)
    multiples of q = qw qx >= 2^-20, and (sum |w x| + |bias| + |res|) / q < 2^24 for every output.  -> the largest such sum / q."""
    q = qw * qx
    assert q >= 2.0 ** -20 and math.frexp(q)[0] == 0.5, f"quantum {q} is not a power of two >= 2^-20"
    for name, t, qq in (("w", w64, qw), ("x", xs64, qx)):
        assert bool(((t / qq) == (t / qq).round()).all()), f"{name} is not a multiple of its quantum"
    total = (w64.abs() @ xs64.abs().T).T                              # [R, N]; exact in fp64: integer multiples of q far below 2^53 q
    for name, t in (("bias", bias64), ("res", res64)):
        if t is not None:
            total = total + t.abs()
            assert bool(((t / q) == (t / q).round()).all()), f"{name} is not a multiple of the quantum"
    bound = (total / q).max().item()
    assert bound < 2.0 ** 24, f"exactness guard: sum of magnitudes / quantum = {bound:.0f} >= 2^24"
    return bound


class Case:
    """One projection call on exact inputs: the padded storages (`store`), the fp64 reference [R, n_out] (`ref`; for SwiGLU also `g`, `u`) and
    the coordinates.  R = rows of x (1 for the single-row entries)."""

    def __init__(self, fmt, entry, R, N, K, epi, seed=0, wide=False):
        norm, sw, f32, has_bias, has_res = EPILOGUES[epi]
        self.fmt, self.entry, self.R, self.N, self.K, self.epi = fmt, entry, R, N, K, epi
        self.norm, self.swiglu, self.out_f32 = norm, sw, f32
        self.n_out = n_out = N // 2 if sw else N
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + R + sum(map(ord, fmt + entry + epi)))
        r = ranges(fmt, K, wide)
        W = self.W = Weights(fmt, N, K, g, swiglu=sw, wide=wide)
        # the staged x rows [R, K] as the kernel must see them after its prologue, and the raw x / norm weight that produce them
        nw = None
        if norm:
            sign = _ints(g, (R, K), 0, 1).double() * 2 - 1
            x = sign * 4.0                                            # +-2^2: mean x^2 = 16, x rstd = +-(1 - 3e-7), so (v rstd) w rounds to +-w
            if norm == "w":
                nw = _ints(g, (K,), -8, 8, nonzero=True).double()
            xs, qx = sign * (nw if nw is not None else 1.0), 1.0
        else:
            x = xs = _ints(g, (R, K), -r["x"], r["x"]).double()
            qx = 1.0
        if sw:      # scale by a power of two so that the gate sums spread over about +-8: silu is not saturated
            gate = (W.w64 @ xs.T).T.reshape(R, -1, 2, 32)[:, :, 0]
            p = max(0, math.ceil(math.log2(max(gate.abs().max().item(), 8.0) / 8.0)))
            f = 2.0 ** -p
            qx = f
            xs = xs * f
            if nw is not None:
                nw = nw * f                                           # x stays +-4: the scale rides in the norm weight
            else:
                x = x * f
        bias = _ints(g, (N,), -r["bias"], r["bias"]).double() if has_bias else None
        res = None
        if has_res:
            res = _ints(g, (R, n_out), -r["res"], r["res"]).double() * (2.0 ** -4 if sw else 1.0)
        self.quantum = W.quantum * qx
        if sw:      # the guard holds for the gate and the up sums; silu(g) u + res is the approximate part
            self.bound = guard(W.w64, xs, None, None, W.quantum, qx)
        else:
            self.bound = guard(W.w64, xs, bias, res, W.quantum, qx)
        y = (W.w64 @ xs.T).T                                          # [R, N] fp64: exact
        if sw:
            y = y.reshape(R, -1, 2, 32)
            self.g, self.u = y[:, :, 0].reshape(R, -1), y[:, :, 1].reshape(R, -1)
            y = torch.nn.functional.silu(self.g) * self.u
        if bias is not None:
            y = y + bias
        if res is not None:
            y = y + res
        self.ref = y
        self.xs64 = xs
        # storages.  Row pads: x / A K + 8 (NaN); GEMV y n_out + 5, res n_out + 3; skinny C n_out + 4, res n_out + 4; one extra row each
        nan = float("nan")
        skinny = entry == "skinny"
        xst = torch.full((R + 1, K + 8), nan, dtype=torch.bfloat16)
        xst[:R, :K] = x.bfloat16()
        assert torch.equal(xst[:R, :K].double(), x)
        self.store = dict(x=xst)
        if nw is not None:
            nst = torch.full((K + 8,), nan, dtype=torch.float32)
            nst[:K] = nw.float()
            self.store["norm_w"] = nst
        if bias is not None:
            bst = torch.full((N + 8,), nan, dtype=torch.float32)
            bst[:N] = bias.float()
            self.store["bias"] = bst
        if res is not None:
            rst = torch.full((R + 1, n_out + (4 if skinny else 3)), nan, dtype=torch.bfloat16)
            rst[:R, :n_out] = res.bfloat16()
            assert torch.equal(rst[:R, :n_out].double(), res)
            self.store["res"] = rst
        self.out_shape = (R + 1, n_out + (4 if skinny else 5))
        self.out_dtype = torch.float32 if f32 else torch.bfloat16

    def coords(self):
        return f"{self.fmt}/{self.entry} R={self.R} N={self.N} K={self.K} {self.epi}"

    def expected(self):
        """The one correct output [R, n_out] in the output type (SwiGLU: the fp64 value rounded; compared to one ulp by `swiglu_check`)."""
        return self.ref.float() if self.out_f32 else self.ref.float().bfloat16()


def run_case(ops, c, dev):
    """Run case `c` through its entry point on `dev` with strided views of the poisoned storages; returns the whole output storage
    [R + 1, n_out + pad] (CPU).  The 16-bit rms_plain form has no wrapper parameter: it goes through the C entry like decoder.py's call."""
    from videollama2_amd import _lib
    st = {k: v.to(dev) for k, v in c.store.items()}
    wst = c.W.to(dev)
    wv = weight_views(c.fmt, wst, c.N, c.K)
    R, K, n_out = c.R, c.K, c.n_out
    out_st = torch.full(c.out_shape, SENTINEL, dtype=c.out_dtype, device=dev)
    x2 = st["x"][:R, :K]
    res2 = st["res"][:R, :n_out] if "res" in st else None
    out2 = out_st[:R, :n_out]
    kw = dict(swiglu=c.swiglu, out_f32=c.out_f32, bias=st["bias"][:c.N] if "bias" in st else None)
    if c.entry == "skinny":
        fn = {"b16": ops.gemm_skinny, "fp8": ops.gemm_skinny_fp8, "mx4": ops.gemm_skinny_mxfp4}[c.fmt]
        fn(x2, *wv, res=res2, out=out2, **kw)
    else:
        single = c.entry == "gemv"
        xa, ra, oa = (x2[0], None if res2 is None else res2[0], out2[0]) if single else (x2, res2, out2)
        nk = dict(norm_w=st["norm_w"][:K], eps=EPS) if c.norm == "w" else {}
        if c.norm == "plain":
            if c.fmt == "b16":
                assert single, "the 16-bit batched entry has no rms_plain form"
                flags = GEMV_RMS_PLAIN | (GEMM_OUT_F32 if c.out_f32 else 0)
                _lib.call("vl2_gemv_bf16", ops._p(wv[0]), ops._p(xa), None, ops._p(ra), ops._p(kw["bias"]), ops._p(oa), c.N, K, wv[0].stride(0),
                          EPS, flags, ops._stream())
                return out_st.cpu()
            nk = dict(rms_plain=True, eps=EPS)
        fn = {("b16", True): ops.gemv, ("b16", False): ops.gemv_batched, ("fp8", True): ops.gemv_fp8, ("fp8", False): ops.gemv_batched_fp8,
              ("mx4", True): ops.gemv_mxfp4, ("mx4", False): ops.gemv_batched_mxfp4}[(c.fmt, single)]
        fn(*wv, xa, res=ra, out=oa, **nk, **kw)
    return out_st.cpu()


def canaries_intact(c, out_st):
    """Everything outside [R, n_out] of the output storage still holds the sentinel (pad columns, the extra row)."""
    keep = torch.full(c.out_shape, SENTINEL, dtype=c.out_dtype)
    m = torch.ones(c.out_shape, dtype=torch.bool)
    m[:c.R, :c.n_out] = False
    return bool((out_st[m] == keep[m]).all())


def ulp_distance(a, b):
    """|distance| in bf16 steps between two bf16 tensors of finite values (sign-magnitude bits -> a monotone integer line)."""
    def line(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


def swiglu_cap(c):
    return max(1, c.n_out * c.R // 100)


def probe_cap(K):
    return max(1, K // 1000)


def check_case(c, out_st):
    """-> (error message or None, number of outputs that differ from the rounded fp64 value [SwiGLU only])."""
    if not canaries_intact(c, out_st):
        bad = torch.nonzero(out_st != torch.full(c.out_shape, SENTINEL, dtype=c.out_dtype))
        bad = [tuple(i) for i in bad.tolist() if i[0] >= c.R or i[1] >= c.n_out]
        return f"{c.coords()}: canary overwritten at {bad[:4]}", 0
    y, exp = out_st[:c.R, :c.n_out], c.expected()
    if not c.swiglu:
        if torch.equal(y, exp):
            return None, 0
        diff = torch.nonzero((y != exp) | y.isnan())
        r, n = diff[0].tolist()
        return f"{c.coords()}: {len(diff)} of {y.numel()} outputs differ, first at row {r} column {n}: got {y[r, n].item()!r}, exact {exp[r, n].item()!r}", len(diff)
    if bool(y.isnan().any()):
        return f"{c.coords()}: NaN in the output (a poisoned pad was read)", int(y.isnan().sum())
    d = ulp_distance(y, exp)
    nd = int((d > 0).sum())
    if int(d.max()) > 1:
        r, n = torch.nonzero(d > 1)[0].tolist()
        return f"{c.coords()}: row {r} column {n} is {int(d[r, n])} bf16 steps from RNE(silu(g) u + res): got {y[r, n].item()!r}, exact {exp[r, n].item()!r}", nd
    if nd > swiglu_cap(c):
        return f"{c.coords()}: {nd} outputs differ from RNE(silu(g) u + res) by one step, cap {swiglu_cap(c)}", nd
    return None, nd


def swiglu_reference_share(c):
    """The reference alone: torch fp32 silu(g) * u (+ res) rounded to bf16 against the fp64 one on the same exact g and u -> outputs that differ."""
    y32 = torch.nn.functional.silu(c.g.float()) * c.u.float()
    if "res" in c.store:
        y32 = y32 + c.store["res"][:c.R, :c.n_out].float()
    d = ulp_distance(y32.bfloat16(), c.expected())
    return int((d > 0).sum()), int(d.max())


def three_orders_exact(c, rows=4):
    """The products of up to `rows` outputs summed in fp32 forward, reversed and in a random permutation all give the reference exactly."""
    g = torch.Generator().manual_seed(5)
    w32, x32 = c.W.w64.float(), c.xs64.float()
    y = (c.W.w64 @ c.xs64.T).T
    for n in torch.randperm(c.N, generator=g)[:rows].tolist():
        prod = w32[n] * x32[0]
        for order in (torch.arange(c.K), torch.arange(c.K - 1, -1, -1), torch.randperm(c.K, generator=g)):
            acc = torch.cumsum(prod[order], 0, dtype=torch.float32)      # a sequential fp32 sum: every prefix is rounded to fp32
            s = torch.zeros((), dtype=torch.float32)
            for chunk in prod[order].split(4096):                        # and a blocked one
                s = s + chunk.sum(dtype=torch.float32)
            if acc[-1].double() != y[0, n] or s.double() != y[0, n]:
                return False
    return True


# ---------------------------------------------------------------------------------------------------------------- the staged-x probe
PROBE_K = {"b16": (8, 72, 2056, 4096, 4104, 8192), "fp8": (16, 1040, 4096, 4112, 8192), "mx4": (32, 2080, 4096, 4128, 8192)}


def probe_inputs(K, rows=4, seed=0):
    """x [rows, K] random bf16, norm_w [K] = rand + 0.5 (fp32)."""
    g = torch.Generator().manual_seed(977 * K + seed)
    return torch.randn(rows, K, generator=g).bfloat16(), torch.rand(K, generator=g) + 0.5


def probe_reference(x, norm_w):
    """fp64 RMSNorm of the bf16 rows, rounded to bf16 once."""
    xd = x.double()
    y = xd * torch.rsqrt((xd * xd).mean(dim=-1, keepdim=True) + EPS)
    if norm_w is not None:
        y = y * norm_w.double()
    return y.float().bfloat16()


def probe_reference_fp32(x, norm_w):
    """The same in torch fp32 (HF MistralRMSNorm): what the reference alone does against fp64."""
    xf = x.float()
    y = xf * torch.rsqrt((xf * xf).mean(dim=-1, keepdim=True) + EPS)
    if norm_w is not None:
        y = y * norm_w
    return y.bfloat16()


def identity_weights(fmt, K, dev):
    """Identity [K, K] in the format, built on `dev`: a GEMV with fp32 output then returns its staged x exactly (one nonzero product each)."""
    if fmt == "b16":
        return (torch.eye(K, dtype=torch.bfloat16, device=dev),)
    if fmt == "fp8":
        q = torch.zeros((K, K), dtype=torch.uint8, device=dev)
        q.fill_diagonal_(F8.e4m3fn_encode(1.0))
        return q, torch.ones(K, dtype=torch.float32, device=dev)
    q = torch.zeros((K, K // 2), dtype=torch.uint8, device=dev)      # E2M1 code of 1.0 = 2: low nibble for even k, high for odd
    k = torch.arange(K, device=dev)
    q[k, k // 2] = torch.where(k % 2 == 0, 2, 2 << 4).to(torch.uint8)
    return q, torch.full((K, K // 32), 127, dtype=torch.uint8, device=dev)


def probe_collect(ops, fmt, K, x, norm_w, dev, batched=(2, 3, 4)):
    """{kernel name: staged x [rows, K] bf16 (CPU)} from every kernel of the format that stages x; norm_w None = rms_plain."""
    from videollama2_amd import _lib
    wv = identity_weights(fmt, K, dev)
    xd = x.to(dev)
    nk = dict(norm_w=norm_w.to(dev), eps=EPS) if norm_w is not None else dict(rms_plain=True, eps=EPS)
    out = {}

    def single(row):
        if fmt == "b16" and norm_w is None:
            y = torch.empty(K, dtype=torch.float32, device=dev)
            _lib.call("vl2_gemv_bf16", ops._p(wv[0]), ops._p(xd[row]), None, None, None, ops._p(y), K, K, K, EPS, GEMV_RMS_PLAIN | GEMM_OUT_F32,
                      ops._stream())
            return y
        fn = {"b16": ops.gemv, "fp8": ops.gemv_fp8, "mx4": ops.gemv_mxfp4}[fmt]
        return fn(*wv, xd[row], out_f32=True, **nk)
    out["single"] = torch.stack([single(r) for r in range(x.shape[0])]).cpu()
    if not (fmt == "b16" and norm_w is None):
        fn = {"b16": ops.gemv_batched, "fp8": ops.gemv_batched_fp8, "mx4": ops.gemv_batched_mxfp4}[fmt]
        for mb in batched:
            y = fn(*wv, xd[:mb], out_f32=True, **nk).cpu()
            out[f"batched{mb}"] = y
    for k, v in out.items():
        assert torch.equal(v.bfloat16().float(), v), f"{fmt} K={K} {k}: a staged value is not a 16-bit number"
    return {k: v.bfloat16() for k, v in out.items()}


def probe_check(fmt, K, probes, x, norm_w):
    """(a) all probes of one (x, norm) are bit-identical; (b) against the fp64 RMSNorm rounded to bf16 every element is equal or adjacent and at
    most probe_cap(K) per row differ.  -> (error or None, differing elements, elements)."""
    base = probes["single"]
    for k, v in probes.items():
        if not torch.equal(v.view(torch.int16), base[:v.shape[0]].view(torch.int16)):
            i = torch.nonzero(v.view(torch.int16) != base[:v.shape[0]].view(torch.int16))[0].tolist()
            return f"{fmt} K={K} norm={'w' if norm_w is not None else 'plain'}: the staged x of `{k}` differs from the single-row kernel's at {i}", 0, 0
    ref = probe_reference(x, norm_w)
    d = ulp_distance(base, ref)
    per_row = (d > 0).sum(dim=1)
    if int(d.max()) > 1:
        return f"{fmt} K={K}: a staged element is {int(d.max())} bf16 steps from the fp64 RMSNorm", int(per_row.sum()), d.numel()
    if int(per_row.max()) > probe_cap(K):
        return f"{fmt} K={K}: {int(per_row.max())} elements of a row differ from the fp64 RMSNorm, cap {probe_cap(K)}", int(per_row.sum()), d.numel()
    return None, int(per_row.sum()), d.numel()
