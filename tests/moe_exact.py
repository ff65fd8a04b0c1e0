"""TEST INFRASTRUCTURE ONLY -- exact inputs for the sparse-MoE kernels (csrc/k_moe.h, csrc/k_moe_skinny.h, the vl2_moe_* entry points): generators,
the exactness guards, the fp64 references, the case tables and the checkers of tests/test_gpu_moe_edges.py, tests/test_moe_edges_emu.py and
tests/test_moe_edges_host.py.  The rule and the conventions are tests/decode_exact.py's and tests/gemm_exact.py's; what
can be imported from there is imported.

THE RULE.  Operands are small integers times powers of two, every partial sum in every association order is an integer multiple of a quantum
q >= 2^-20 below 2^24 q (asserted per case), so fp32 accumulation is exact, the fp64 reference is THE answer and outputs are compared with
`torch.equal`.  Only silu of the SwiGLU forms (one 16-bit step of RNE(fp64), at most max(1, outputs // 100) outputs differing: decode_exact's
cap), the softmax weights, rsqrt and the logits' one product are approximate; their bounds are derived at `check_route` and `check_combine`.

THE ROUTER IS DETERMINED.  x rows are +-4 (mean x^2 = 16 exactly, one rstd for every row) and wr holds small integers, so every score
sum_d x wr is an exact integer in fp32.  The kernel's logit is fl(score * rstd) with one positive rstd: equal scores give bit-equal logits and
bit-equal probabilities, scores that differ by >= 1 give logits that differ by >= 0.25.  With the spread of a row's logits <= 16 (asserted on the
integer scores: spread of the scores <= 64) no __expf underflows, so no two different scores can land on the same probability: the k experts are
the first k of the order (score descending, expert index ascending) -- "ties -> the lower expert index" -- on EVERY row, no margin mask.

THE CONTRACTS, as read from the kernels:
    moe_router_kernel   wts[j] = moe_div(p_j, p_0 + ... + p_{k-1}), summed in slot order in fp32; k = 1: p / p = 1.0 exactly; k equal p: the sum
                        is exactly k p for k in {2, 4} (2 p is exact; fl(3 p) is off 3 p by at most half a unit, which the next sum's coarser
                        unit absorbs: 4 p), so the weights are exactly 1 / k.  moe_div is a division that holds this under the library's
                        -ffast-math (a plain `/` is a * rcp(b) there, and p rcp(p) can be 1 - 2^-24: what this test first found).
    moe_scan_kernel     counts, offs (each expert padded to the row tile), gather (ascending tokens inside an expert, -1 on every padding row up
                        to P), inv: pure functions of ids.
    moe_gather_kernel   live rows only: padding rows of xg / rn are not written.
    moe_gemm_kernel     gemm_exact's epilogue contract (RMSNorm v * rstd_m, SwiGLU silu(g) * u on the 32 | 32 columns of a 64-column block, one
                        rounding at the store) per expert on its own rows; rows >= counts[e] of an expert's range and rows >= offs[E] unwritten.
    moe_gemv_down_body  y[n] = bf16(res[n] + o), o = fma(w_j, dot_j, o) over the slots j = 0 .. k-1 IN SLOT ORDER, one rounding.  With dyadic
                        weights every step is exact; `DownCase.order_case` is the one input on which the order of the slots shows.
    moe_combine_kernel  acc = fma(w_j, y[inv[t][j]], acc) in slot order from 0, THEN x1 + acc (the residual is added last), one rounding;
                        rn[t] = (0, rsqrt(mean of the STORED row's squares + eps)).

Every operand is a strided view of a poisoned allocation (row stride > width, one extra row, NaN padding; NaN in the gaps of a strided expert
stack and in every padding row) and every output the caller allocates sits in a SENTINEL frame.  Where ops.moe_* allocates a buffer itself
(moe_route's xg, rn, gather, ...) the entry point is called through _lib.call with the test's own buffers.  Storages are kept in fp32 / fp64 on
the CPU and cast to the library's 16-bit element type at upload (every value is exact in bf16 and in fp16).

Nothing under videollama2_amd/ imports this file."""
import math
from collections import namedtuple

import torch

from tests import decode_exact as D
from tests import gemm_exact as G

SENTINEL, _ints, ulp_distance = D.SENTINEL, D._ints, D.ulp_distance
ISENT = int(SENTINEL)                   # the sentinel of the int32 tables
EPS = 1e-5
GEMM_SWIGLU = 1
MOE_BM, MOE_MAX_E, MOE_MAX_K, MOE_SCAN_MAX = 128, 64, 4, 16384      # k_moe.h (restated; tests/test_moe_edges_host.py holds them against the header)
NAN = float("nan")

WTS_TOL = 1e-5          # |wts - fp64| : the project's existing bound for this quantity (tests/test_gpu_moe.py test_route_tables)
RSTD_ULPS = 4           # the sum of squares is exact, so rstd = rsqrtf(fl(16 + eps)): one rounding of the sum (fl(16 + 1e-5) is 2.4e-7 relative
#                         from 16 + 1e-5 = a quarter of that, 0.5 ulp, in rsqrt) + rsqrtf itself (<= 1 ulp) + the reference's own rounding to fp32
#                         (0.5 ulp): 2 ulps; 4 leaves margin
LOGIT_ULPS = 1          # logit = fl(score * rstd): score is exact, rstd once rounded; against fl32(score) * fl32(rstd_ref) rounded once


def moe_rows(S, k, E):
    """ops.moe_rows restated (held against it in tests/test_moe_edges_host.py)."""
    return (S * k + E * (MOE_BM - 1) + MOE_BM - 1) // MOE_BM * MOE_BM


def ulp32(a, b):
    """|distance| in fp32 steps between two fp32 tensors of finite values."""
    def line(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (line(a) - line(b)).abs()


def elem_dtype():
    from videollama2_amd import _lib
    return _lib.elem_dtype()


def framed(shape, dtype, dev, fill=SENTINEL, front=8, back=8):
    """A flat storage of `fill` with `front` / `back` elements around a contiguous view of `shape` (front = 8 keeps the view 16-byte aligned
    for 16-bit and 32-bit elements) -> (storage, view)."""
    n = int(math.prod(shape))
    st = torch.full((front + n + back,), fill, dtype=dtype, device=dev)
    return st, st[front:front + n].view(shape)


def frame_intact(st, n, fill=SENTINEL, front=8):
    st = st.cpu()
    return bool((st[:front] == fill).all()) and bool((st[front + n:] == fill).all())


def _padded(t, pad, rows_extra=1):
    """t [r, c] fp64 -> fp32 storage [r + rows_extra, c + pad] of NaN with t inside."""
    r, c = t.shape
    st = torch.full((r + rows_extra, c + pad), NAN, dtype=torch.float32)
    st[:r, :c] = t.float()
    assert torch.equal(st[:r, :c].double(), t.double())
    return st


# ================================================================================================================ the router
LEVELS, REST, BLOCK = (8, 6, 4, 2), -2, 8      # planted block sums / 4 of the slots 0 .. 3 and of every other expert; columns owned by an expert


def ids_from_scores(sc, k):
    """THE ids: the first k experts of the order (score descending, index ascending).  sc int64 [S, E]."""
    E = sc.shape[1]
    key = -sc * E + torch.arange(E, dtype=torch.int64)[None, :]          # distinct keys: nothing is left to the sort's stability
    return torch.argsort(key, dim=1)[:, :k].contiguous()


def _from_levels(lev, g):
    """lev int64 [S, E], even, |lev| <= 8 -> x [S, 8 E] of +-4 and wr [E, 8 E] of 0 / 1: wr[e] is 1 on the block of 8 columns owned by expert e, and
    the signs inside token t's block e are set so that the block sums to 4 lev[t][e] ((8 + lev) / 2 columns of +4 at random places)."""
    S, E = lev.shape
    assert bool((lev % 2 == 0).all()) and int(lev.abs().max()) <= BLOCK
    plus = (BLOCK + lev) // 2
    place = torch.rand((S, E, BLOCK), generator=g).argsort(-1)
    x = torch.where(place < plus[:, :, None], 4, -4).reshape(S, E * BLOCK).to(torch.int64)
    wr = torch.zeros((E, E * BLOCK), dtype=torch.int64)
    for e in range(E):
        wr[e, e * BLOCK:(e + 1) * BLOCK] = 1
    return x, wr


def planted(want, E, g, levels=LEVELS, rest=REST):
    """The planted mode: a wanted ORDERED id table [S, k] -> (x, wr, scores) whose integer scores yield it.  levels[j] = the block sum / 4 of slot
    j, rest = that of every unchosen expert; equal levels plant ties (the caller's table must then follow the tie rule: the ids re-derived from
    the int64 scores are asserted equal to it)."""
    S, k = want.shape
    lev = torch.full((S, E), rest, dtype=torch.int64)
    lev.scatter_(1, want, torch.tensor(levels[:k], dtype=torch.int64)[None, :].expand(S, k))
    x, wr = _from_levels(lev, g)
    sc = x @ wr.T
    assert torch.equal(sc, 4 * lev)
    assert torch.equal(ids_from_scores(sc, k), want), "the planted table does not follow from its scores"
    return x, wr, sc


def want_random(S, E, k, g):
    return torch.rand((S, E), generator=g).argsort(1)[:, :k].contiguous()


def want_from_counts(counts, S, k):
    """A table [S, k] in which expert e is chosen counts[e] times and no token chooses an expert twice: the experts' runs laid over the (slot,
    token) grid slot by slot (a run of at most S entries never meets the same token twice)."""
    c = torch.tensor(counts, dtype=torch.int64)
    assert int(c.sum()) == S * k and int(c.max()) <= S, (counts, S, k)
    seq = torch.repeat_interleave(torch.arange(len(counts)), c)
    want = seq.view(k, S).T.contiguous()
    assert all(len(set(r)) == k for r in want.tolist())
    return want


TIES = ("pair", "rest", "chosen", "all")


def tie_levels(kind, k):
    """-> (levels, rest).  pair: the slots tie two by two above the rest; rest: the k-th slot ties with every unchosen expert; chosen: the k
    chosen tie among themselves above the rest (weights exactly 1 / k); all: every expert ties (ids 0 .. k-1, weights exactly 1 / k)."""
    if kind == "pair":
        return (6, 6, 4, 4)[:k], -2
    if kind == "rest":
        return LEVELS[:k], LEVELS[k - 1]
    if kind == "chosen":
        return (4,) * k, -2
    return (4,) * k, 4


def want_tied(S, E, k, g, levels, rest):
    """A random assignment of the levels to experts, and the table the tie rule derives from it."""
    lev = torch.full((S, E), rest, dtype=torch.int64)
    perm = torch.rand((S, E), generator=g).argsort(1)[:, :k]
    lev.scatter_(1, perm, torch.tensor(levels, dtype=torch.int64)[None, :].expand(S, k))
    return ids_from_scores(lev, k)


FREE_NNZ = 8            # nonzero columns of a free-mode router row: |score| <= 4 * 8, so the spread of a token's scores is <= 64
FREE_TIE_SHARE = 0.10   # the stated share of rows with a tie at the k-th place


def free(S, Dm, E, k, seed):
    """The free mode: x random +-4 over any D, wr in {-1, 0, 1} with FREE_NNZ nonzero columns per expert spread over the WHOLE row -- one in the
    first 16-byte vector, one in the last, one in vector 64 (lane 0's second trip of the `v = lane; v < nvec; v += 64` loops) where there is
    one, the others anywhere -- so that the spread bound holds at every D.  (A dense row of D = 4096 random +-1 has a spread of hundreds.)  The
    seed is advanced on the CPU until at least FREE_TIE_SHARE of the rows tie at the k-th place."""
    assert E > k, "a tie at the k-th place needs an unchosen expert"
    for s in range(seed, seed + 256):
        g = torch.Generator().manual_seed(7919 * s + 31 * Dm + E)
        x = _ints(g, (S, Dm), 0, 1) * 8 - 4
        wr = torch.zeros((E, Dm), dtype=torch.int64)
        for e in range(E):
            cols = {int(torch.randint(0, 8, (1,), generator=g)), Dm - 8 + int(torch.randint(0, 8, (1,), generator=g))}
            if Dm >= 520:
                cols.add(512 + int(torch.randint(0, 8, (1,), generator=g)))
            while len(cols) < min(FREE_NNZ, Dm):
                cols.add(int(torch.randint(0, Dm, (1,), generator=g)))
            cols = torch.tensor(sorted(cols))
            wr[e, cols] = _ints(g, (len(cols),), 0, 1) * 2 - 1
        sc = x @ wr.T
        top = sc.sort(1, descending=True).values
        if float((top[:, k - 1] == top[:, k]).double().mean()) >= FREE_TIE_SHARE:
            return x, wr, sc
    raise AssertionError(f"free mode: no seed gives {FREE_TIE_SHARE:.0%} tied rows (S={S} D={Dm} E={E} k={k})")


def tables_ref(ids, E, BM, P):
    """counts [E], offs [E + 1] (each expert padded to BM), gather [P] (-1 = padding and every row past offs[E]), inv [S, k] from the ids alone:
    inside an expert the rows are in ascending token order."""
    S, k = ids.shape
    flat = ids.reshape(-1)
    counts = torch.bincount(flat, minlength=E)
    pad = (counts + BM - 1) // BM * BM
    offs = torch.zeros(E + 1, dtype=torch.int64)
    offs[1:] = pad.cumsum(0)
    order = torch.argsort(flat, stable=True)                          # (token, slot) pairs by expert, ascending token inside an expert
    start = torch.zeros(E + 1, dtype=torch.int64)
    start[1:] = counts.cumsum(0)
    e_sorted = flat[order]
    rows = offs[e_sorted] + (torch.arange(S * k) - start[e_sorted])
    gather = torch.full((P,), -1, dtype=torch.int64)
    gather[rows] = order // k
    inv = torch.empty(S * k, dtype=torch.int64)
    inv[order] = rows
    assert int(offs[E]) <= P
    return counts.int(), offs.int(), gather.int(), inv.view(S, k).int()


# entry: route (vl2_moe_route, row tile 128, xg / rn), rows (vl2_moe_route_rows, compact tables), gemv (vl2_moe_route_gemv, one token)
# mode: want (random table) | counts (arg = the count vector) | ties (arg = kind) | free (arg = D)
RRow = namedtuple("RRow", "entry S E k mode arg", defaults=(None,))

ROUTE_S = (1, 3, 4, 5,          # four tokens per router workgroup: part of one, a full one, one token into the second
           63, 64, 65,          # the scan's 64-token ballot chunks: a partial chunk, a full one, one token into the second
           1023, 1025)          # the scan's 1024-thread staging loop `for (i = tid; i < S * k; i += 1024)` (k = 1: one short of a trip, one past)
ROUTE_E = (1, 2, 8,             # one expert (k = 1 only); the smallest choice; Mixtral's
           16, 17,              # the scan's 16 waves `for (e = wave; e < E; e += 16)`: one trip each, wave 0 takes a second
           63, 64)              # lane 63 holds a logit / lane 63 is idle in the router; MOE_MAX_E
ROUTE_K = (1, 2, 3, 4)          # MOE_MAX_K = 4; k = 1 and 3 never ran before
FREE_D = (8,                    # one vector: lane 0 alone
          504, 512, 520,        # 63, 64, 65 vectors: a partial wave trip, a full one, lane 0's second trip
          4096)                 # Mixtral's D: 8 trips


def _count_vectors():
    """name -> (counts, k): S = sum / k.  The planted count vectors of the 128-row tile and of the compact tables."""
    v = {
        "one_first": ((130, 0, 0, 0, 0, 0, 0, 0), 1), "one_middle": ((0, 0, 0, 130, 0, 0, 0, 0), 1), "one_last": ((0, 0, 0, 0, 0, 0, 0, 130), 1),
        # empty first and last expert around counts of exactly 1, 127, 128, 129, 256 and 257: every distance to the row tile
        "tile_edges": ((0, 1, 127, 128, 129, 256, 257, 0), 2),
        "empty_first": ((0, 129, 1, 128, 127, 257, 2, 256), 2), "empty_last": ((257, 128, 1, 129, 127, 256, 2, 0), 2),
        "tile_edges_k4": ((257, 1, 127, 128, 129, 256, 0, 258), 4),
    }
    return v


COUNT_VECTORS = _count_vectors()
# the compact tables (row tile 1: offs[e + 1] - offs[e] = counts[e], offs[E] = S k): the same vectors, and the batched decode's own sizes
COUNT_VECTORS_ROWS = dict(COUNT_VECTORS, small_first=((5, 0, 0, 0, 0, 0, 0, 0), 1), small_last=((0, 0, 0, 0, 0, 0, 0, 64), 1),
                          small_mixed=((0, 1, 15, 16, 17, 33, 46, 0), 2))


def route_table():
    rows, i = [], 0
    for entry in ("route", "rows"):
        # every S with E and k rotating, the modes rotating
        for S in ROUTE_S:
            E = ROUTE_E[1 + i % 6]
            k = 1 + i % min(4, E)
            mode = ("want", "ties", "free")[i % 3] if E > k else "want"
            arg = TIES[i % 4] if mode == "ties" else (FREE_D[i % 3 + 1] if mode == "free" else None)
            if mode == "ties" and arg == "pair" and k == 1:
                arg = "rest"
            rows.append(RRow(entry, S, E, k, mode, arg))
            i += 1
        # every E with every k <= E at S = 65
        for E in ROUTE_E:
            for k in ROUTE_K:
                if k <= E:
                    mode = ("ties", "want")[i % 2] if E > k else "want"
                    rows.append(RRow(entry, 65, E, k, mode, TIES[(i // 2) % 4] if mode == "ties" and k > 1 else ("rest" if mode == "ties" else None)))
                    i += 1
        # every kind of tie at k = 2 and 4 (the exact 1 / k weights), and at k = 3
        for kind in TIES:
            for k in (2, 3, 4):
                rows.append(RRow(entry, 33, 8, k, "ties", kind))
        # the D edges of the vector loops in the free mode
        for Dm in FREE_D:
            rows.append(RRow(entry, 37, 8, 2, "free", Dm))
        rows.append(RRow(entry, 9, 64, 4, "free", 520))
        # the planted count vectors
        for name, (_, k) in (COUNT_VECTORS if entry == "route" else COUNT_VECTORS_ROWS).items():
            vec = (COUNT_VECTORS if entry == "route" else COUNT_VECTORS_ROWS)[name][0]
            rows.append(RRow(entry, sum(vec) // k, len(vec), k, "counts", name))
        # S * k == MOE_SCAN_MAX exactly: the last id the scan stages
        rows.append(RRow(entry, 8192, 8, 2, "want"))
        rows.append(RRow(entry, 4096, 16, 4, "ties", "rest"))
    for E, k, mode, arg in ((1, 1, "want", None), (2, 1, "ties", "rest"), (8, 2, "ties", "chosen"), (8, 2, "free", 4096), (8, 3, "free", 504),
                            (17, 4, "ties", "pair"), (64, 4, "want", None), (64, 1, "free", 520), (63, 2, "ties", "all"), (16, 4, "ties", "chosen")):
        rows.append(RRow("gemv", 1, E, k, mode, arg))
    return list(dict.fromkeys(rows))


# the calls that must be refused with the documented error and leave every sentinel alone: (why, entry, S, E, k, P (None = ops.moe_rows), message)
ROUTE_REFUSALS = (
    ("S * k > 16384", "route", 8193, 8, 2, None, "S * k <="), ("S * k > 16384", "rows", 4097, 8, 4, None, "S * k <="),
    ("k > E", "route", 5, 2, 3, None, "need E <="), ("k > E", "rows", 5, 2, 3, None, "need E <="), ("k > E", "gemv", 1, 2, 3, None, "need E <="),
    ("E > 64", "route", 5, 65, 2, None, "need E <="), ("E > 64", "rows", 5, 65, 2, None, "need E <="), ("E > 64", "gemv", 1, 65, 2, None, "need E <="),
    ("k > 4", "route", 5, 8, 5, None, "need E <="),
    ("P too small", "route", 5, 8, 2, "small", "must be a multiple of"), ("P not a multiple of 128", "route", 5, 8, 2, "odd", "must be a multiple of"),
)


class RouteCase:
    """One router call on exact inputs: the storages, the int64 scores, THE ids and every reference table."""

    def __init__(self, row, seed=0):
        self.row = row
        entry, S, E, k, mode, arg = row
        self.S, self.E, self.k = S, E, k
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * S + 31 * E + k + sum(map(ord, entry + mode + str(arg))))
        if mode == "free":
            x, wr, sc = free(S, arg, E, k, seed)
        else:
            if mode == "want":
                want, lv, rest = want_random(S, E, k, g), LEVELS, REST
            elif mode == "counts":
                vec = (COUNT_VECTORS_ROWS if entry == "rows" else COUNT_VECTORS)[arg][0]
                want, lv, rest = want_from_counts(vec, S, k), LEVELS, REST
            else:
                lv, rest = tie_levels(arg, k)
                want = want_tied(S, E, k, g, lv, rest)
            x, wr, sc = planted(want, E, g, lv, rest)
            self.want = want
        self.D = Dm = x.shape[1]
        self.x, self.wr, self.sc = x, wr, sc
        # the guards, in integer arithmetic: every score and every sum of squares is exact in fp32 in any order, and no __expf underflows
        assert int((x.abs() @ wr.abs().T).max()) < 2 ** 24 and 16 * Dm < 2 ** 24
        self.spread = int((sc.max(1).values - sc.min(1).values).max())
        assert self.spread <= 64, f"logit spread {self.spread / 4} > 16"
        self.ids = ids_from_scores(sc, k)
        top = sc.sort(1, descending=True).values
        self.tied_rows = float((top[:, k - 1] == top[:, k]).double().mean()) if E > k else 0.0
        self.chosen_tie = (sc.gather(1, self.ids) == sc.gather(1, self.ids[:, :1])).all(1)      # rows whose k chosen scores all tie
        self.BM = MOE_BM if entry == "route" else 1
        self.P = moe_rows(S, k, E) if entry == "route" else S * k
        self.counts, self.offs, self.gather, self.inv = tables_ref(self.ids, E, self.BM, self.P)
        # fp64 references
        self.rstd64 = (16.0 + EPS) ** -0.5
        self.rstd32 = torch.tensor(self.rstd64, dtype=torch.float64).float()
        self.logits_ref = (sc.float().double() * self.rstd32.double()).float()          # fl32(score) * fl32(rstd_ref), rounded once
        p = torch.softmax(sc.double() * self.rstd64, dim=1).gather(1, self.ids)
        self.wts_ref = p / p.sum(1, keepdim=True)
        self.store = dict(x=_padded(x.double(), 8), wr=_padded(wr.double(), 0))          # wr has no row stride in the ABI: one NaN row behind it

    def coords(self):
        r = self.row
        return f"{r.entry} S={r.S} E={r.E} k={r.k} D={self.D} {r.mode}{'' if r.arg is None else ':' + str(r.arg)}"


def _route_buffers(entry, S, E, k, Dm, P, dev, with_logits=True):
    """Every output of a router entry in its sentinel frame -> {name: (storage, view, fill)}."""
    i32, f32 = torch.int32, torch.float32
    b = {"ids": framed((S, k), i32, dev, ISENT) + (ISENT,), "wts": framed((S, k), f32, dev) + (SENTINEL,)}
    if with_logits:
        b["logits"] = framed((S, E), f32, dev) + (SENTINEL,)
    if entry in ("route", "rows"):
        b.update(counts=framed((E,), i32, dev, ISENT) + (ISENT,), offs=framed((E + 1,), i32, dev, ISENT) + (ISENT,),
                 gather=framed((P,), i32, dev, ISENT) + (ISENT,), inv=framed((S, k), i32, dev, ISENT) + (ISENT,))
    if entry == "route":
        b.update(rstd=framed((S,), f32, dev) + (SENTINEL,), xg=framed((P, Dm), elem_dtype(), dev) + (SENTINEL,),
                 rn=framed((P, 2), f32, dev) + (SENTINEL,))
    return b


def _call_route(ops, entry, x2, wr, S, Dm, E, k, P, b):
    from videollama2_amd import _lib
    p = lambda n: ops._p(b[n][1]) if n in b else None
    if entry == "route":
        _lib.call("vl2_moe_route", ops._p(x2), x2.stride(0), ops._p(wr), S, Dm, E, k, EPS, p("ids"), p("wts"), p("rstd"), p("logits"), p("counts"),
                  p("offs"), p("gather"), p("inv"), P, p("xg"), p("rn"), ops._stream())
    elif entry == "rows":
        _lib.call("vl2_moe_route_rows", ops._p(x2), x2.stride(0), ops._p(wr), S, Dm, E, k, EPS, p("ids"), p("wts"), p("logits"), p("counts"),
                  p("offs"), p("gather"), p("inv"), ops._stream())
    else:
        _lib.call("vl2_moe_route_gemv", ops._p(x2[0]), ops._p(wr), Dm, E, k, EPS, p("ids"), p("wts"), p("logits"), ops._stream())


def run_route(ops, c, dev):
    """Run the case through its entry point with buffers of the test's own -> {name: whole storage (CPU)}."""
    S, E, k, Dm = c.S, c.E, c.k, c.D
    x_st = c.store["x"].to(elem_dtype()).to(dev)
    wr_st = c.store["wr"].to(dev)
    b = _route_buffers(c.row.entry, S, E, k, Dm, c.P, dev)
    _call_route(ops, c.row.entry, x_st[:S, :Dm], wr_st[:E], S, Dm, E, k, c.P, b)
    return {n: st.cpu() for n, (st, _, _) in b.items()}


def run_route_refusal(ops, ref, dev):
    """One row of ROUTE_REFUSALS: the call must raise with the documented message and write nothing.  -> error or None."""
    from videollama2_amd import _lib
    why, entry, S, E, k, P, msg = ref
    Dm = 8
    full = moe_rows(S, k, E)
    P = full if P is None else full - MOE_BM if P == "small" else full + 64
    x = torch.zeros((S + 1, Dm + 8), dtype=elem_dtype(), device=dev)
    wr = torch.zeros((E + 1, Dm), dtype=torch.float32, device=dev)
    b = _route_buffers(entry, S, E, k, Dm, max(P, full), dev)
    try:
        _call_route(ops, entry, x[:S, :Dm], wr[:E], S, Dm, E, k, P, b)
    except _lib.Vl2HipError as e:
        if msg not in str(e):
            return f"{entry}: {why}: refused with another message: {e}"
    else:
        return f"{entry}: {why}: accepted"
    if dev != "cpu":
        torch.cuda.synchronize()
    for n, (st, _, fill) in b.items():
        if not bool((st == fill).all()):
            return f"{entry}: {why}: {n} was written by a refused call"
    return None


def check_route(c, out):
    """-> (errors, figures): ids, counts, offs, gather, inv equal to the reference tables; logits within LOGIT_ULPS of fl32(score) * fl32(rstd_ref)
    (both factors are exact or once rounded, and the kernel rounds their product once: at most one step unless the kernel's rstd is not the
    correctly rounded one, which RSTD_ULPS bounds separately); wts within WTS_TOL of the fp64 softmax / top-k / renormalise, exactly 1.0 at k = 1
    and exactly 1 / k where the k chosen scores tie (k in {2, 4}); rstd within RSTD_ULPS of fp64 rsqrt(16 + eps); xg / rn live rows equal to the
    bits of x[gather[p]] and (0, rstd[gather[p]]), every padding row untouched; every frame intact."""
    S, E, k, Dm, P = c.S, c.E, c.k, c.D, c.P
    errs, fig = [], dict(wts=0.0, rstd_ulps=0, logit_ulps=0)
    who = c.coords()
    fills = {n: (ISENT if st.dtype == torch.int32 else SENTINEL) for n, st in out.items()}
    sizes = dict(ids=S * k, wts=S * k, logits=S * E, counts=E, offs=E + 1, gather=P, inv=S * k, rstd=S, xg=P * Dm, rn=2 * P)
    for n, st in out.items():
        if not frame_intact(st, sizes[n], fills[n]):
            errs.append(f"{who}: the frame of {n} was overwritten")
    v = {n: st[8:8 + sizes[n]] for n, st in out.items()}
    ids = v["ids"].view(S, k).long()
    if not torch.equal(ids, c.ids):
        t = torch.nonzero((ids != c.ids).any(1))[0].item()
        errs.append(f"{who}: ids differ on {int((ids != c.ids).any(1).sum())} of {S} rows, first token {t}: got {ids[t].tolist()}, "
                    f"determined {c.ids[t].tolist()} (scores {c.sc[t].tolist()[:16]})")
        return errs, fig
    wts = v["wts"].view(S, k)
    if bool(wts.isnan().any()):
        errs.append(f"{who}: NaN in wts (a poisoned pad was read)")
        return errs, fig
    fig["wts"] = float((wts.double() - c.wts_ref).abs().max())
    if fig["wts"] > WTS_TOL:
        errs.append(f"{who}: wts {fig['wts']:.3e} from the fp64 reference, bound {WTS_TOL}")
    if k == 1 and not bool((wts == 1.0).all()):
        errs.append(f"{who}: k = 1 and a weight is not exactly 1.0")
    if k in (2, 4) and bool(c.chosen_tie.any()) and not bool((wts[c.chosen_tie] == 1.0 / k).all()):
        errs.append(f"{who}: the k chosen scores tie and a weight is not exactly 1 / {k}")
    if "logits" in v:
        lg = v["logits"].view(S, E)
        d = ulp32(lg, c.logits_ref)
        d = torch.where(c.sc == 0, (lg != 0).long() * 99, d)                # a zero score gives a zero logit exactly
        fig["logit_ulps"] = int(d.max())
        if fig["logit_ulps"] > LOGIT_ULPS:
            t, e = torch.nonzero(d > LOGIT_ULPS)[0].tolist()
            errs.append(f"{who}: logit [{t}, {e}] is {int(d[t, e])} fp32 steps from fl32(score) * fl32(rstd): got {lg[t, e].item()!r}, "
                        f"reference {c.logits_ref[t, e].item()!r}")
    if "rstd" in v:
        d = ulp32(v["rstd"], c.rstd32.expand(S).contiguous())
        fig["rstd_ulps"] = int(d.max())
        if fig["rstd_ulps"] > RSTD_ULPS:
            errs.append(f"{who}: rstd {fig['rstd_ulps']} fp32 steps from rsqrt(16 + eps), bound {RSTD_ULPS}")
    if "counts" in v:
        for n, ref in (("counts", c.counts), ("offs", c.offs), ("gather", c.gather), ("inv", c.inv.reshape(-1))):
            if not torch.equal(v[n], ref):
                i = torch.nonzero(v[n] != ref)[0].item()
                errs.append(f"{who}: {n}[{i}] is {int(v[n][i])}, reference {int(ref[i])} ({int((v[n] != ref).sum())} entries differ)")
        if c.row.entry == "rows" and int(c.offs[E]) != S * k:
            errs.append(f"{who}: the compact reference tables do not end at S * k")
    if "xg" in v:
        xg, rn = v["xg"].view(P, Dm), v["rn"].view(P, 2)
        live = c.gather >= 0
        src = c.gather[live].long()
        x_el = c.x.double().to(xg.dtype)
        if not torch.equal(xg[live].view(torch.int16), x_el[src].view(torch.int16)):
            errs.append(f"{who}: a live row of xg is not the bits of x[gather[p]]")
        if not bool((xg[~live] == SENTINEL).all()) or not bool((rn[~live] == SENTINEL).all()):
            errs.append(f"{who}: a padding row of xg / rn was written")
        if not (bool((rn[live][:, 0] == 0).all()) and torch.equal(rn[live][:, 1], v["rstd"][src])):
            errs.append(f"{who}: a live row of rn is not (0, rstd[gather[p]])")
    return errs, fig


def reference_alone_route(c):
    """The references alone in torch fp32 on the CPU (softmax, top-k by THE ids, renormalise; rsqrt(mean + eps)) against every bound check_route
    applies -> (largest wts deviation, rstd steps, logit steps)."""
    x32 = c.x.float()
    rstd = torch.rsqrt((x32 * x32).mean(1) + EPS)
    lg = (x32 @ c.wr.float().T) * rstd[:, None]
    p = torch.softmax(lg, 1).gather(1, c.ids)
    w = p / p.sum(1, keepdim=True)
    return (float((w.double() - c.wts_ref).abs().max()), int(ulp32(rstd, c.rstd32.expand(c.S).contiguous()).max()),
            int(torch.where(c.sc == 0, torch.zeros((), dtype=torch.int64), ulp32(lg, c.logits_ref)).max()))


# ================================================================================================================ the grouped GEMMs
def _epilogue(acc, rs, swiglu, dt):
    """gemm_exact.Case.epilogue's contract for the epilogues vl2_moe_gemm builds (plain, swiglu, swiglu_rms): v = acc; RMSNorm v = v * rstd_m;
    SwiGLU v = silu(g) * u on the 32 gate | 32 up columns of every 64-column block."""
    v = acc.to(dt)
    if rs is not None:
        v = v * rs.to(dt)[:, None]
    if swiglu:
        y = v.reshape(v.shape[0], -1, 2, 32)
        v = (torch.nn.functional.silu(y[:, :, 0]) * y[:, :, 1]).reshape(v.shape[0], -1)
    return v


MOE_EPIS = ("plain", "swiglu", "swiglu_rms")       # the only epilogues the entry point builds
GEMM_COUNTS = (0, 1, 31, 32, 33,    # an idle expert; one row; the 32-row wave slabs of gemm_l8_16_body's empty-wave skip: 31, 32, 33 live rows
               127, 128, 129,       # the row tile: a ragged tile, a full one, a second tile of one row
               257)                 # three tiles, the last of one row
GRow = namedtuple("GRow", "E counts N K epi shrink", defaults=(None,))


def gemm_table():
    """Per-expert counts from GEMM_COUNTS, rotated so that each count is the first, a middle and the last expert, over E in {2, 8, 64}; N = one,
    two and three column tiles; K from gemm_exact.K_ALL; the epilogue rotating.  Grids (P / 128 row tiles x N / 128 column tiles) that are and
    are not multiples of 8 both occur (xcd_remap): tests/test_moe_edges_host.py asserts it."""
    rows, i, c = [], 0, GEMM_COUNTS
    for E in (2, 8, 64):
        for r in range(len(c)):
            counts = tuple(c[(r + 4 * j) % 9] for j in range(2)) if E == 2 else tuple(c[(r + j) % 9] for j in range(E))
            K = G.K_ALL[i % len(G.K_ALL)] if E < 64 else G.K_ALL[i % 3]
            rows.append(GRow(E, counts, (128, 256, 384)[i % 3] if E < 64 else (128, 256)[i % 2], K, MOE_EPIS[i % 3]))
            i += 1
    # counts smaller than the padded range (the rows left over keep the sentinel), for every epilogue
    for epi in MOE_EPIS:
        rows.append(GRow(8, (129, 40, 0, 128, 1, 257, 33, 127), 256, 192, epi, ((0, 30), (1, 16), (3, 127), (5, 0), (7, 1))))
    return rows


class GemmCase:
    """One vl2_moe_gemm call: the device tables are the case's own (independent of the router).  `given` = the counts the kernel is told,
    `alloc` = the counts the offsets were laid out for (shrink: given < alloc for some experts)."""

    def __init__(self, row, seed=0, wide=False):
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
        self.P = P = moe_rows(S, k, E)
        offs = [0]
        for cnt in alloc:
            offs.append(offs[-1] + (cnt + MOE_BM - 1) // MOE_BM * MOE_BM)
        assert offs[-1] <= P
        self.counts, self.offs = torch.tensor(given, dtype=torch.int32), torch.tensor(offs, dtype=torch.int32)
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + E + sum(alloc) + sum(map(ord, epi)))
        ra, rw = (8, 15) if not wide else (2 ** 9, 2 ** 7)
        wi = _ints(g, (E, N, K), -rw, rw).double()
        a = torch.full((P, K), NAN, dtype=torch.float64)
        live = torch.zeros(P, dtype=torch.bool)
        owner = torch.full((P,), -1, dtype=torch.int64)
        for e in range(E):
            a[offs[e]:offs[e] + alloc[e]] = _ints(g, (alloc[e], K), -ra, ra).double()      # the leftover rows of a shrunk expert hold numbers too
            live[offs[e]:offs[e] + given[e]] = True
            owner[offs[e]:offs[e] + given[e]] = e
        self.live, self.owner = live, owner
        rs = torch.exp2(-((torch.arange(P) * 5 + seed) % 4).double()) if self.rms else None      # 1, 1/2, 1/4, 1/8: neighbours differ
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
        if self.swiglu and len(rows):           # A carries a power of two that brings the gate values to about +-8 (gemm_exact's rule)
            pre = _epilogue(acc, rs_live, False, torch.float64).reshape(len(rows), -1, 2, 32)[:, :, 0]
            sa = 2.0 ** -max(0, math.ceil(math.log2(max(float(pre.abs().max()), 8.0) / 8.0)))
        self.quantum = q = sa * (0.125 if self.rms else 1.0)
        # the guard: gemm_exact.guard_case's rule with the row-norm term
        assert q >= 2.0 ** -20 and math.frexp(q)[0] == 0.5, f"quantum {q} is not a power of two >= 2^-20"
        pre = _epilogue(acc * sa, rs_live, False, torch.float64)
        assert G._multiple(pre, q), "a pre-activation value is not a multiple of the quantum"
        tot = mag * sa * (rs_live[:, None] if rs_live is not None else 1.0)
        self.bound = float((tot / q).max()) if len(rows) else 0.0
        assert self.bound < 2.0 ** 24, f"exactness guard: sum of magnitudes / quantum = {self.bound:.0f} >= 2^24"
        self.a64, self.w64, self.acc, self.rs_live, self.rows = a * sa, wi, acc * sa, rs_live, rows
        self.ref = _epilogue(self.acc, rs_live, self.swiglu, torch.float64)
        self.R = len(rows)                                                   # decode_exact.swiglu_cap reads c.R and c.n_out
        # storages: A [P + 1, K + 8]; the expert stack [E, N + 1, K + 8] (ldw > K, w_stride > N ldw: a NaN row between two experts); rn [P + 1, 2]
        ast = torch.full((P + 1, K + 8), NAN, dtype=torch.float32)
        ast[:P, :K] = (a * sa).float()
        wst = torch.full((E, N + 1, K + 8), NAN, dtype=torch.float32)
        wst[:, :N, :K] = wi.float()
        self.store = dict(a=ast, w=wst)
        if self.rms:
            rn = torch.full((P + 1, 2), NAN, dtype=torch.float32)
            rn[rows, 0], rn[rows, 1] = 0.0, rs_live.float()                  # NaN in every padding row
            self.store["rn"] = rn
        self.out_shape = (P + 2, n_out + 8)
        self.grid = (P // MOE_BM) * (N // 128)

    def coords(self):
        r = self.row
        c = r.counts if len(r.counts) <= 8 else r.counts[:4] + ("...",) + r.counts[-2:]
        return f"moe_gemm E={r.E} counts={c} N={r.N} K={r.K} {r.epi}{' shrink' if r.shrink else ''}"

    def expected(self, ref=None):
        return (self.ref if ref is None else ref).float().to(elem_dtype())

    def rounding_share(self):
        r64 = self.ref
        inexact = r64.float().bfloat16().double() != r64
        step = torch.exp2(torch.floor(torch.log2(r64.abs().clamp(min=1e-30))) - 7)
        return float(inexact.double().mean()), int((inexact & (((r64 / step) % 1.0) == 0.5)).sum())


def run_gemm(ops, c, dev):
    el = elem_dtype()
    a, w = c.store["a"].to(el).to(dev), c.store["w"].to(el).to(dev)
    rn = c.store["rn"].to(dev) if c.rms else None
    out = torch.full(c.out_shape, SENTINEL, dtype=el, device=dev)
    route = dict(counts=c.counts.to(dev), offs=c.offs.to(dev))
    ops.moe_gemm(a[:c.P, :c.K], w[:, :c.N, :c.K], route, c.S, c.k, swiglu=c.swiglu, row_norm=None if rn is None else rn[:c.P], eps=EPS,
                 out=out[1:c.P + 1, :c.n_out])
    return out.cpu()


def _check_rows(c, y, exp, approx, who, cap_outputs):
    """y, exp [rows, n] of the element type -> (error or None, outputs that differ)."""
    if not approx:
        if torch.equal(y, exp):
            return None, 0
        diff = torch.nonzero((y != exp) | y.isnan())
        r, n = diff[0].tolist()
        return f"{who}: {len(diff)} of {y.numel()} outputs differ, first at live row {r} column {n}: got {y[r, n].item()!r}, exact {exp[r, n].item()!r}", len(diff)
    if bool(y.isnan().any()):
        return f"{who}: NaN in the output (a poisoned pad was read)", int(y.isnan().sum())
    d = ulp_distance(y, exp)
    nd = int((d > 0).sum()) if d.numel() else 0
    if d.numel() and int(d.max()) > 1:
        r, n = torch.nonzero(d > 1)[0].tolist()
        return f"{who}: live row {r} column {n} is {int(d[r, n])} steps from RNE of the fp64 value: got {y[r, n].item()!r}, exact {exp[r, n].item()!r}", nd
    cap = max(1, cap_outputs // 100)
    if nd > cap:
        return f"{who}: {nd} outputs differ from RNE of the fp64 value by one step, cap {cap}", nd
    return None, nd


def check_gemm(c, out):
    """-> (error or None, outputs that differ by one step [SwiGLU only]).  Every padding row of C, every row at or past offs[E], the leftover
    rows of a shrunk expert and the frame keep the sentinel."""
    mask = torch.zeros(c.out_shape, dtype=torch.bool)
    mask[1 + c.rows, :c.n_out] = True
    if not bool((out[~mask] == SENTINEL).all()):
        bad = torch.nonzero((out != SENTINEL) & ~mask)
        return f"{c.coords()}: a row nobody owns was written at {[tuple(i) for i in bad[:4].tolist()]} of the framed output {tuple(out.shape)}", 0
    return _check_rows(c, out[1 + c.rows, :c.n_out], c.expected(), c.swiglu, c.coords(), c.R * c.n_out)


# ---- the grouped skinny-M GEMM
SKINNY_S = (5, 16, 17, 33, 64)          # moe_gemv_batched's last size + 1; MT = 1 full, MT = 2 by one row, MT = 4 by one row, the most
SRow = namedtuple("SRow", "S k counts N K rowmap swiglu shrink", defaults=(None,))


def skinny_table():
    """Counts from {0, 1, 15, 16, 17, 33, 64} (an idle expert, one row, the 16-row MFMA groups +- 1, three groups by one row, every token) that
    sum to S k; with and without rowmap; K = 1184 (37 steps, a prime: no split) and K that split (96 -> 3, 2368 -> 2, 512 -> 16 at N = 1024)."""
    vecs = {5: (2, (0, 1, 5, 4, 0, 0, 0, 0)), 16: (4, (16, 15, 1, 0, 16, 16, 0, 0)), 17: (2, (17, 16, 1, 0, 0, 0, 0, 0)),
            33: (3, (33, 17, 16, 15, 1, 0, 17, 0)), 64: (2, (0, 1, 15, 16, 17, 33, 46, 0))}
    nk = ((128, 1184), (128, 96), (128, 2368), (1024, 512))
    rows, i = [], 0
    for S in SKINNY_S:
        k, counts = vecs[S]
        for j, (N, K) in enumerate(nk):
            rows.append(SRow(S, k, counts, N, K, bool((i + j) % 2), (i + j) % 3 == 1))
        i += 1
    rows.append(SRow(64, 1, (64,) + (0,) * 7, 128, 1184, True, False))                     # every token on one expert
    rows.append(SRow(64, 1, (0,) * 63 + (64,), 128, 96, False, True))                      # E = 64, the last expert alone
    rows.append(SRow(33, 3, (33, 17, 16, 15, 1, 0, 17, 0), 128, 96, True, False, ((0, 16), (1, 0), (6, 1))))      # rows owned by nobody
    return rows


class SkinnyCase:
    def __init__(self, row, seed=0):
        self.row = row
        S, k, alloc, N, K, rowmap, sw, shrink = row
        self.S, self.k, self.E, self.N, self.K, self.swiglu = S, k, len(alloc), N, K, sw
        E, R = self.E, S * k
        self.Rp = R
        self.n_out = n_out = N // 2 if sw else N
        given = list(alloc)
        for e, cnt in (shrink or ()):
            given[e] = cnt
        want = want_from_counts(alloc, S, k)
        cnts, offs, gather, _ = tables_ref(want, E, 1, R)
        assert cnts.tolist() == list(alloc) and int(offs[E]) == R
        self.counts, self.offs = torch.tensor(given, dtype=torch.int32), offs
        self.rowmap = gather if rowmap else None
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + S + 17 * k)
        a_rows = S if rowmap else R
        a = _ints(g, (a_rows, K), -8, 8).double()
        wi = _ints(g, (E, N, K), -15, 15).double()
        live = torch.zeros(R, dtype=torch.bool)
        owner = torch.full((R,), -1, dtype=torch.int64)
        for e in range(E):
            live[int(offs[e]):int(offs[e]) + given[e]] = True
            owner[int(offs[e]):int(offs[e]) + given[e]] = e
        self.live, self.rows = live, torch.nonzero(live).flatten()
        src = gather.long() if rowmap else torch.arange(R)
        ap = a[src[self.rows]]
        acc = torch.stack([ap[i] @ wi[owner[r]].T for i, r in enumerate(self.rows.tolist())]) if len(self.rows) else torch.zeros((0, N), dtype=torch.float64)
        sa = 1.0
        if sw:
            gate = acc.reshape(len(self.rows), -1, 2, 32)[:, :, 0]
            sa = 2.0 ** -max(0, math.ceil(math.log2(max(float(gate.abs().max()), 8.0) / 8.0)))
        self.quantum = sa
        for e in range(E):
            m = owner[self.rows] == e
            if bool(m.any()):
                D.guard(wi[e], ap[m] * sa, None, None, 1.0, sa)
        self.acc = acc * sa
        self.ref = _epilogue(self.acc, None, sw, torch.float64)
        self.R = len(self.rows)
        wst = torch.full((E, N + 1, K + 8), NAN, dtype=torch.float32)
        wst[:, :N, :K] = wi.float()
        self.store = dict(a=_padded(a * sa, 8), w=wst)
        self.a_rows = a_rows
        self.ks = D.skinny_plan(S, N, K)["ks"]
        self.out_shape = (R + 2, n_out + 4)

    def coords(self):
        r = self.row
        return f"moe_gemm_skinny S={r.S} k={r.k} counts={r.counts if len(r.counts) <= 8 else '...'} N={r.N} K={r.K}{' rowmap' if r.rowmap else ''}{' swiglu' if r.swiglu else ''}{' shrink' if r.shrink else ''}"

    def expected(self):
        return self.ref.float().to(elem_dtype())


def run_skinny(ops, c, dev):
    el = elem_dtype()
    a, w = c.store["a"].to(el).to(dev), c.store["w"].to(el).to(dev)
    out = torch.full(c.out_shape, SENTINEL, dtype=el, device=dev)
    need = ops.moe_skinny_part_bytes(c.S, c.k, c.N, c.K) // 4
    assert need == c.ks * c.Rp * c.N, (need, c.ks, c.Rp, c.N)
    part_st, part = framed((need,), torch.float32, dev, fill=NAN)          # NaN, not the sentinel: a partial sum may be any integer
    tables = dict(counts=c.counts.to(dev), offs=c.offs.to(dev))
    ops.moe_gemm_skinny(a[:c.a_rows, :c.K], w[:, :c.N, :c.K], tables, c.S, c.k, part, rowmap=None if c.rowmap is None else c.rowmap.to(dev),
                        swiglu=c.swiglu, out=out[1:c.Rp + 1, :c.n_out])
    return out.cpu(), part_st.cpu()


def check_skinny(c, out, part_st):
    """Owned rows against the reference; the frame of C; the frame of the partial sums and every partial row owned by nobody keep their poison.
    (An unowned row of C itself is reduced from that poison: its content is not part of the contract, its neighbours are.)"""
    n = c.ks * c.Rp * c.N
    if not (bool(part_st[:8].isnan().all()) and bool(part_st[8 + n:].isnan().all())):
        return f"{c.coords()}: the frame of the partial sums was overwritten", 0
    part = part_st[8:8 + n].view(c.ks, c.Rp, c.N)
    if not bool(part[:, ~c.live].isnan().all()):
        return f"{c.coords()}: a partial row owned by nobody was written", 0
    if bool(part[:, c.live].isnan().any()):
        return f"{c.coords()}: a partial sum of an owned row was not written (or a poisoned pad was read)", 0
    mask = torch.zeros(c.out_shape, dtype=torch.bool)
    mask[1:c.Rp + 1, :c.n_out] = True
    if not bool((out[~mask] == SENTINEL).all()):
        return f"{c.coords()}: the frame of C was overwritten", 0
    return _check_rows(c, out[1 + c.rows, :c.n_out], c.expected(), c.swiglu, c.coords(), c.R * c.n_out)


# ================================================================================================================ the decode GEMVs
DYADIC = {1: ((1.0,),), 2: ((0.5, 0.5), (0.25, 0.75)), 3: ((0.25, 0.25, 0.5), (0.5, 0.125, 0.375)), 4: ((0.125, 0.125, 0.25, 0.5), (0.25, 0.25, 0.25, 0.25))}
DOWN_K = (8, 72, 520,       # 1, 9, 65 vectors: one lane, part of one slot, lane 0's second slot
          4096, 4104)       # 512 vectors: the last one-pass K; 513: a second pass of one vector
DOWN_N = (1, 3, 4, 5, 41)   # one row per wave, four per workgroup: part of a workgroup, a full one, one row into the second, eleven
DOWN_K_LDS = 20480          # K k 2 = 160 KiB exactly at k = 4: the whole LDS; 20488 must be refused
# gate/up: (E, k, N, K): k in {1, 2, 4} from E in {4, 64}; the ids always include 0 and E - 1 where k allows
GU_CASES = ((4, 1, 64, 8), (4, 2, 64, 520), (4, 4, 192, 4096), (4, 2, 192, 4104), (64, 1, 64, 72), (64, 2, 64, 520), (64, 4, 64, 520), (4, 4, 64, 2056))
GU_BATCHED = ((1, 4, 2, 64, 520), (2, 4, 4, 64, 72), (5, 64, 2, 64, 520), (5, 4, 1, 192, 4104))      # (S, E, k, N, K)
DRow = namedtuple("DRow", "S E k N K res batched", defaults=(False,))


def _ids_for(S, E, k, g):
    """ids [S, k]: distinct per token, the first token holds expert E - 1 first and expert 0 last (out of ascending order)."""
    ids = want_random(S, E, k, g)
    if E >= 2 and k >= 2:
        ids[0, 0], ids[0, k - 1] = E - 1, 0
        for j in range(1, k - 1):
            ids[0, j] = j
    elif k == 1:
        ids[0, 0] = E - 1
    return ids


def down_table():
    rows, i = [], 0
    for K in DOWN_K:
        for N in DOWN_N:
            rows.append(DRow(1, (4, 8)[i % 2], 1 + i % 4, N, K, i % 2 == 0))
            i += 1
    for k in (1, 2, 3, 4):                  # every KS at both pass counts, with and without the residual
        for K in (520, 4104):
            rows.append(DRow(1, 4, k, 5, K, k % 2 == 1))
            rows.append(DRow(1, 4, k, 5, K, k % 2 == 0))
    rows.append(DRow(1, 64, 4, 41, 72, True))
    rows.append(DRow(1, 4, 4, 5, DOWN_K_LDS, True))
    for S in (1, 2, 5):                     # batched: every token its own ids, weights and residual row; ldy / ldres > N
        for k, N, K in ((2, 5, 520), (4, 41, 72), (3, 3, 4104), (1, 4, 8)):
            rows.append(DRow(S, 8, k, N, K, (S + k) % 2 == 0, True))
    rows.append(DRow(2, 4, 4, 5, DOWN_K_LDS, True, True))
    return list(dict.fromkeys(rows))


class DownCase:
    """vl2_moe_gemv / vl2_moe_gemv_batched, flags 0: y[t] = bf16(res[t] + sum_j w_tj W_{ids[t][j]} a[t k + j]) on the test's own ids and DYADIC
    weights (every fma of the slot-order chain is then exact: all terms are multiples of q = 2^-3 below 2^24 q)."""

    def __init__(self, row, seed=0, wide=False):
        self.row = row
        S, E, k, N, K, has_res, batched = row
        self.S, self.E, self.k, self.N, self.K, self.batched = S, E, k, N, K, batched
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + 5 * S + k + E)
        self.ids = _ids_for(S, E, k, g)
        self.wts = torch.tensor([DYADIC[k][(t + seed) % len(DYADIC[k])] for t in range(S)], dtype=torch.float64)
        ra = 64 if wide else 8 if K <= 8192 else 2                            # 8 * 15 * K / 2^-3 < 2^24 needs K <= 17476
        a = _ints(g, (S * k, K), -ra, ra).double()
        wi = _ints(g, (E, N, K), -15, 15).double()
        res = _ints(g, (S, N), -64, 64).double() if has_res else None
        self._finish(a, wi, res, 0.125)

    def _finish(self, a, wi, res, q, guarded=True):
        S, k, N, K, E = self.S, self.k, self.N, self.K, self.E
        self.quantum = q
        dots = torch.stack([torch.stack([wi[self.ids[t, j]] @ a[t * k + j] for j in range(k)]) for t in range(S)])       # [S, k, N]
        mags = torch.stack([torch.stack([wi[self.ids[t, j]].abs() @ a[t * k + j].abs() for j in range(k)]) for t in range(S)])
        tot = (mags * self.wts[:, :, None].abs()).sum(1) + (res.abs() if res is not None else 0.0)
        self.ref = (dots * self.wts[:, :, None]).sum(1) + (res if res is not None else 0.0)                               # exact in fp64
        assert G._multiple(self.ref, q) and G._multiple(dots * self.wts[:, :, None], q), "a term is not a multiple of the quantum"
        self.bound = float((tot / q).max())
        assert not guarded or self.bound < 2.0 ** 24, f"exactness guard: sum of magnitudes / quantum = {self.bound:.0f} >= 2^24"
        self.dots = dots
        wst = torch.full((E, N + 1, K + 8), NAN, dtype=torch.float32)
        wst[:, :N, :K] = wi.float()
        assert torch.equal(wst[:, :N, :K].double(), wi)
        self.store = dict(a=_padded(a, 0), w=wst)                             # the SwiGLU rows have no row stride in the ABI: one NaN row behind
        if res is not None:
            self.store["res"] = _padded(res, 3)
        self.res = res

    @classmethod
    def order_case(cls):
        """The one input on which the ORDER of the slots shows.  Slot 0: w = 1, dot = A = -1024 + 3 * 2^-10 (exact).  Slot 1: w = 1 + 2^-20,
        dot = 1025: B = w dot = 1025 + 2^-10 + 2^-20 needs 31 bits.  In slot order o = fma(1, A, 0) = A exactly, then fma(w1, 1025, A) rounds the
        EXACT sum A + B = 1.00390625 + 2^-20 once: representable, just above the midpoint of 1.0 and 1.0078125, so the stored value is 1.0078125
        = RNE of the exact value.  In the reverse order fl(B) = 1025 + 2^-10 loses the 2^-20, A + fl(B) = 1.00390625 is the midpoint itself and the
        store rounds it to even: 1.0.  (bf16 only: the numbers are chosen for an 8-bit significand.)"""
        c = cls.__new__(cls)
        c.row = DRow(1, 4, 2, 3, 8, False)
        c.S, c.E, c.k, c.N, c.K, c.batched = 1, 4, 2, 3, 8, False
        c.ids = torch.tensor([[3, 0]])
        c.wts = torch.tensor([[1.0, 1.0 + 2.0 ** -20]], dtype=torch.float64)
        a = torch.zeros((2, 8), dtype=torch.float64)
        a[0, :3], a[1, :2] = 1.0, 1.0
        wi = torch.zeros((4, 3, 8), dtype=torch.float64)
        wi[3, :, 0], wi[3, :, 1], wi[3, :, 2] = -1024.0, 2.0 ** -9, 2.0 ** -10
        wi[0, :, 0], wi[0, :, 1] = 1024.0, 1.0
        c._finish(a, wi, None, 2.0 ** -20, guarded=False)      # not exact in any order -- that is the point; every step is worked out above
        assert c.ref.float().bfloat16().tolist() == [[1.0078125] * 3]
        return c

    def coords(self):
        r = self.row
        return f"moe_gemv{'_batched' if r.batched else ''} down S={r.S} E={r.E} k={r.k} N={r.N} K={r.K}{' res' if r.res else ''}"

    def expected(self):
        return self.ref.float().to(elem_dtype())

    def rounding_share(self):
        r64 = self.ref
        inexact = r64.float().bfloat16().double() != r64
        step = torch.exp2(torch.floor(torch.log2(r64.abs().clamp(min=1e-30))) - 7)
        return float(inexact.double().mean()), int((inexact & (((r64 / step) % 1.0) == 0.5)).sum())


def run_down(ops, c, dev):
    """-> the whole output storage (CPU): flat [8 + N + 8] for the single-token entry, [S + 1, N + 5] for the batched one."""
    el = elem_dtype()
    S, k, N, K = c.S, c.k, c.N, c.K
    a, w = c.store["a"].to(el).to(dev), c.store["w"].to(el).to(dev)
    ids, wts = c.ids.int().to(dev), c.wts.float().to(dev)
    res = c.store["res"].to(el).to(dev) if c.res is not None else None
    if not c.batched:
        st, y = framed((N,), el, dev)
        ops.moe_gemv(w[:, :N, :K], a[:k], ids[0].contiguous(), wts=wts[0].contiguous(), res=None if res is None else res[0, :N], out=y)
        return st.cpu()
    out = torch.full((S + 1, N + 5), SENTINEL, dtype=el, device=dev)
    ops.moe_gemv_batched(w[:, :N, :K], a[:S * k], ids, wts=wts, res=None if res is None else res[:S, :N], out=out[:S, :N])
    return out.cpu()


def check_down(c, st):
    if not c.batched:
        if not frame_intact(st, c.N):
            return f"{c.coords()}: the frame of y was overwritten"
        y = st[8:8 + c.N][None, :]
    else:
        m = torch.zeros(st.shape, dtype=torch.bool)
        m[:c.S, :c.N] = True
        if not bool((st[~m] == SENTINEL).all()):
            return f"{c.coords()}: the frame of y was overwritten"
        y = st[:c.S, :c.N]
    return _check_rows(c, y, c.expected(), False, c.coords(), 0)[0]


class GateUpCase:
    """vl2_moe_gemv / vl2_moe_gemv_batched with VL2_GEMM_SWIGLU: decode_exact's SwiGLU rule on RMSNorm(+-4 rows) -- the staged x is +-1 exactly --
    for the k experts of the test's own ids; the power of two that keeps the gate sums inside +-8 rides in the weights."""

    def __init__(self, S, E, k, N, K, batched, seed=0):
        self.S, self.E, self.k, self.N, self.K, self.batched = S, E, k, N, K, batched
        self.n_out = N // 2
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * N + 5 * S + k + E)
        self.ids = _ids_for(S, E, k, g)
        sign = _ints(g, (S, K), 0, 1).double() * 2 - 1
        wi = _ints(g, (E, N, K), -15, 15).double()
        y = torch.stack([wi[self.ids[t, j]] @ sign[t] for t in range(S) for j in range(k)])                            # [S k, N]: row t k + j
        p = max(0, math.ceil(math.log2(max(float(y.reshape(S * k, -1, 2, 32)[:, :, 0].abs().max()), 8.0) / 8.0)))
        self.quantum = f = 2.0 ** -p
        for t in range(S):
            for j in range(k):
                D.guard(wi[self.ids[t, j]] * f, sign[t:t + 1], None, None, f, 1.0)
        self.acc = y * f
        self.ref = _epilogue(self.acc, None, True, torch.float64)
        self.R = S * k
        wst = torch.full((E, N + 1, K + 8), NAN, dtype=torch.float32)
        wst[:, :N, :K] = (wi * f).float()
        self.store = dict(x=_padded(sign * 4.0, 8), w=wst)

    def coords(self):
        return f"moe_gemv{'_batched' if self.batched else ''} gate/up S={self.S} E={self.E} k={self.k} N={self.N} K={self.K}"

    def expected(self):
        return self.ref.float().to(elem_dtype())


def run_gate_up(ops, c, dev):
    """-> the output storage (CPU): [1 + k + 1, N / 2] (slot j in row 1 + j) resp. [S k + 1, N / 2 + 8] for the batched entry."""
    el = elem_dtype()
    S, k, N, K = c.S, c.k, c.N, c.K
    x, w = c.store["x"].to(el).to(dev), c.store["w"].to(el).to(dev)
    ids = c.ids.int().to(dev)
    if not c.batched:
        out = torch.full((k + 2, N // 2), SENTINEL, dtype=el, device=dev)
        ops.moe_gemv(w[:, :N, :K], x[0, :K], ids[0].contiguous(), swiglu=True, eps=EPS, out=out[1:k + 1])
        return out.cpu()
    out = torch.full((S * k + 1, N // 2 + 8), SENTINEL, dtype=el, device=dev)
    ops.moe_gemv_batched(w[:, :N, :K], x[:S, :K], ids, swiglu=True, eps=EPS, out=out[:S * k, :N // 2])
    return out.cpu()


def check_gate_up(c, out):
    """Slot j's output lands in row j (row t k + j of the batched entry); rows >= k and the frame keep the sentinel."""
    m = torch.zeros(out.shape, dtype=torch.bool)
    if c.batched:
        m[:c.R, :c.n_out] = True
    else:
        m[1:c.k + 1] = True
    if not bool((out[~m] == SENTINEL).all()):
        return f"{c.coords()}: a row past the k slots (or the frame) was written", 0
    y = out[:c.R, :c.n_out] if c.batched else out[1:c.k + 1]
    return _check_rows(c, y, c.expected(), True, c.coords(), c.R * c.n_out)


DOWN_REFUSALS = (("one vector past the LDS", False, 1, 4, 20488, "must fit the LDS"), ("one vector past the LDS", True, 2, 4, 20488, "must fit the LDS"))


def run_down_refusal(ops, ref, dev):
    from videollama2_amd import _lib
    why, batched, S, k, K, msg = ref
    el, E, N = elem_dtype(), 4, 5
    w = torch.zeros((E, N, K), dtype=el, device=dev)
    a = torch.zeros((S * k, K), dtype=el, device=dev)
    ids = torch.arange(k, dtype=torch.int32, device=dev).repeat(S, 1)
    wts = torch.full((S, k), 0.25, dtype=torch.float32, device=dev)
    out = torch.full((S + 1, N + 3), SENTINEL, dtype=el, device=dev)
    try:
        if batched:
            ops.moe_gemv_batched(w, a, ids, wts=wts, out=out[:S, :N])
        else:
            ops.moe_gemv(w, a, ids[0].contiguous(), wts=wts[0].contiguous(), out=out[0, :N])
    except _lib.Vl2HipError as e:
        if msg not in str(e):
            return f"down K={K}: {why}: refused with another message: {e}"
    else:
        return f"down K={K}: {why}: accepted"
    if dev != "cpu":
        torch.cuda.synchronize()
    return None if bool((out == SENTINEL).all()) else f"down K={K}: {why}: y was written by a refused call"


# ================================================================================================================ the combine
COMBINE_D = (8,                     # one vector
             2040, 2048, 2056,      # 255, 256, 257 vectors around the 256-thread loop `for (v = tid; v < D / 8; v += 256)`
             4096)                  # Mixtral's D: two full trips
CRow = namedtuple("CRow", "S k D alias")
COMBINE_LARGE = 32                  # columns of a row that carry large values (|out| up to about 100 with eighths: the store must round)


def combine_table():
    rows, i = [], 0
    for Dm in COMBINE_D:
        for k in (1, 2, 3, 4):
            rows.append(CRow((1, 5)[i % 2], k, Dm, i % 3 == 0))
            i += 1
    rows += [CRow(5, 2, 2056, True), CRow(1, 4, 8, True), CRow(5, 4, 4096, False)]
    return list(dict.fromkeys(rows))


class CombineCase:
    """vl2_moe_combine on the test's own inv and DYADIC wts: inv is a random injection of the (token, slot) pairs into P = S k + 3 rows of y --
    slots of one token on rows in and out of ascending order.  Most columns hold small integers (|.| <= 2), COMBINE_LARGE random columns per
    row (the last vector and the vector at the 256-thread boundary among them) large ones -- y up to +-63, x1 eighths below 16 -- so that a good number of outputs need the rounding at
    the store while the sum of the STORED row's squares stays exact in fp32 (multiples of 2^-6 below 2^24 2^-6: the second guard), which is
    what bounds rstd by RSTD_ULPS as in the router."""

    def __init__(self, row, seed=0):
        self.row = row
        S, k, Dm, alias = row
        self.S, self.k, self.D, self.alias = S, k, Dm, alias
        self.P = P = S * k + 3
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * Dm + 31 * S + k)
        self.inv = torch.randperm(P, generator=g)[:S * k].view(S, k)
        self.wts = torch.tensor([DYADIC[k][(t + seed) % len(DYADIC[k])] for t in range(S)], dtype=torch.float64)
        y = _ints(g, (P, Dm), -2, 2).double()
        x1 = _ints(g, (S, Dm), -2, 2).double()
        for t in range(S):
            cols = {Dm - 1 - int(torch.randint(0, 8, (1,), generator=g))}
            if Dm >= 2056:
                cols.add(2048 + int(torch.randint(0, 8, (1,), generator=g)))
            while len(cols) < min(COMBINE_LARGE, Dm):
                cols.add(int(torch.randint(0, Dm, (1,), generator=g)))
            cols = torch.tensor(sorted(cols))
            for j in range(k):
                y[self.inv[t, j], cols] = _ints(g, (len(cols),), -63, 63).double()
            x1[t, cols] = _ints(g, (len(cols),), -127, 127).double() / 8.0     # eighths below 16: with any weights the sum has bits to round
        acc = torch.stack([(y[self.inv[t]] * self.wts[t][:, None]).sum(0) for t in range(S)])        # exact: multiples of 2^-3
        self.acc = acc
        self.ref = x1 + acc
        q = 0.125
        assert G._multiple(self.ref, q)
        tot = torch.stack([(y[self.inv[t]].abs() * self.wts[t][:, None]).sum(0) for t in range(S)]) + x1.abs()
        assert float((tot / q).max()) < 2.0 ** 24
        stored = self.ref.float().bfloat16().double()
        assert G._multiple(stored, q)
        self.ss_bound = float(((stored * stored).sum(1) / (q * q)).max())
        assert self.ss_bound < 2.0 ** 24, f"statistics guard: sum of squares / quantum^2 = {self.ss_bound:.0f} >= 2^24"
        self.store = dict(y=_padded(y, 8), x1=_padded(x1, 8))
        self.x1, self.y = x1, y

    def coords(self):
        r = self.row
        return f"moe_combine S={r.S} k={r.k} D={r.D}{' in place' if r.alias else ''}"

    def expected(self):
        return self.ref.float().to(elem_dtype())

    def rstd_ref(self):
        st = self.expected().double()
        return torch.rsqrt((st * st).mean(1) + EPS).float()

    def rounding_count(self):
        return int((self.ref.float().bfloat16().double() != self.ref).sum())


def run_combine(ops, c, dev):
    """-> (out storage [S + 1, D + 8], rn storage) on the CPU; alias: out is x1's own storage (the strided view, pads and extra row poisoned)."""
    el = elem_dtype()
    S, k, Dm = c.S, c.k, c.D
    y, x1 = c.store["y"].to(el).to(dev), c.store["x1"].to(el).to(dev)
    route = dict(inv=c.inv.int().to(dev), wts=c.wts.float().to(dev))
    rn_st, rn = framed((S, 2), torch.float32, dev)
    if c.alias:
        out = x1
    else:
        out = torch.full((S + 1, Dm + 8), SENTINEL, dtype=el, device=dev)
    ops.moe_combine(x1[:S, :Dm], y[:c.P, :Dm], route, EPS, out=out[:S, :Dm], row_norm=rn)
    return out.cpu(), rn_st.cpu()


def check_combine(c, out, rn_st):
    """-> (error or None, rstd steps).  out = RNE(fp64) with torch.equal; the frame of out (in place: x1's NaN pads and extra row) and of rn
    intact; rn[t] = (0, rstd) with rstd within RSTD_ULPS of fp64 rsqrt(mean of the STORED row's squares + eps): the sum of squares is exact
    (second guard), so the roundings are the division by D (D a power of two or not: <= 0.5 ulp), the + eps (<= 0.5 ulp, halved by the root),
    rsqrtf (<= 1 ulp) and the reference's own rounding (0.5 ulp): 2.5 ulps at most."""
    S, Dm = c.S, c.D
    m = torch.zeros(out.shape, dtype=torch.bool)
    m[:S, :Dm] = True
    rest = out[~m]
    if not bool((rest.isnan() if c.alias else rest == SENTINEL).all()):
        return f"{c.coords()}: the frame of out was overwritten", 0
    if not frame_intact(rn_st, 2 * S):
        return f"{c.coords()}: the frame of rn was overwritten", 0
    err, _ = _check_rows(c, out[:S, :Dm], c.expected(), False, c.coords(), 0)
    if err:
        return err, 0
    rn = rn_st[8:8 + 2 * S].view(S, 2)
    if not bool((rn[:, 0] == 0).all()):
        return f"{c.coords()}: rn[t][0] is not 0", 0
    d = int(ulp32(rn[:, 1].contiguous(), c.rstd_ref()).max())
    if d > RSTD_ULPS:
        return f"{c.coords()}: rstd of the stored row is {d} fp32 steps from the fp64 value, bound {RSTD_ULPS}", d
    return None, d
