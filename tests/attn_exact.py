"""TEST INFRASTRUCTURE ONLY -- exact key-selecting inputs for the split-KV attention family (vl2_attn_decode, _batched, _kv8, _kv8_batched,
_shared, vl2_attn_append and the lab form vl2_attn_decode_fused): generators, the exactness guard, the fp64 reference and the case tables of
tests/test_gpu_attn_edges.py, tests/test_attn_edges_emu.py and the fused cases of tests/test_gpu_lab.py.

THE RULE.  Softmax attention is an exact gather when every score is either the row maximum or far below it.  K row j encodes its position:
head_dim 128 = 4 digits base 32 of j, digit i one-hot (value 1) in dims 32 i .. 32 i + 31 (rotated by a salt per kv head and request, so that
a neighbour's rows never answer).  A query holds -2048 everywhere except 0 at the wanted digit values; a digit whose 32 dims are all 0 is a
wildcard.  The score of a key is -2048 x (mismatched digits), times the product's scale 128^-1/2 x log2(e): 0 for a selected key, at most
-261 in the exp2 domain for every other.  exp2(0) = 1 and exp2(x <= -200) = 0 in fp32 under any implementation, so every slice or tile
without a selected key gets combine weight 0, every other weight 1, and the output is (sum of the selected V rows) / (their count).  With V
integers in [-15, 15] times a per-row power of two (quantum 2^-2) and a power-of-two count, every partial sum and the product with 1 / L are
exact in fp32 in every association order, on the scalar slices, on the MFMA tiles (P is 0 or 1) and through the online-softmax rescales
(factor 0 or 1).  The fp64 softmax over the visible keys, rounded ONCE to the element type, is then THE answer: `torch.equal`, no tolerance.

THE GUARD (`guard`, asserted for every head of every case before the launch): the maximum score is exactly 0, every other score is
<= -200 in the exp2 domain, the number of selected keys is a power of two, sum |V| / quantum over them is below 2^24, and every V element is
a multiple of the quantum.  The fp8 caches add the round trip: quantise -> dequantise of the rows returns them unchanged (`kv8_of`).

RoPE stays in the test: cos/sin row p holds, per frequency d, one of the four exact rotations (cos, sin) in {(1,0), (0,1), (-1,0), (0,-1)},
number (p + d) % 4; the un-roped q and k_new of `qkv` are the inverse rotation of the wanted pattern, and the reference ropes them itself.
A kernel that reads table row pos +- 1, or column d +- 1, rotates wrongly and selects garbage.

Poison: NaN in the partial workspace (guard bands on both sides that must survive), NaN in every cache row past `pos` -- the slot at `pos`
too, the kernel's own append overwrites it --, in the padding of strided operands and in one extra slot before and after a batch; 0x7F codes
and NaN scales in the fp8 caches; outputs pre-filled with a sentinel that must survive outside the written range.  After the call the
caches must hold their bits everywhere except row `pos`, which must hold the roped k_new and v_new.

Nothing under videollama2_amd/ imports this file."""
import torch

HD, HALF = 128, 64
SCALE = HD ** -0.5                      # the product's softmax scale
LOG2E = 1.4426950408889634
NEG = -2048.0                           # a mismatched digit: -2048 * SCALE * LOG2E = -261.2 in the exp2 domain
GAP = -200.0                            # the guard's bound on every non-selected score (exp2 domain)
V_QUANTUM = 0.25                        # V = integers in [-15, 15] * 2^e, e in -2 .. 2
SENTINEL = -777.0
BAND = 520                              # floats of NaN guard band on either side of the partial workspace (a multiple of 2: 8-byte stores)
N_WORLD = 16448 + 576                   # keys of the longest context any table reaches, and the shared-prefix own rows on top


# ---------------------------------------------------------------------------------------------------------------- the case tables
# vl2_attn_decode / _kv8 / _fused: position of the new token (context = pos + 1), why -- from attn_decode_kernel (64-key slices, four waves of
# 16 keys) and attn_combine_head (k_decode.h: early <= 32 slices; 64 slices per max/sum pass; 256 weights per LDS chunk; 8-wide loop + tail)
DECODE_POS = (
    0,                  # one key: the appended row alone
    15, 16,             # the last key of wave 0 / the first of wave 1; context 16 cuts a 32-key block to 16
    63, 64,             # 1 -> 2 slices
    71,                 # context 72: the block 64 .. 95 cut to 8
    2047, 2048,         # 32 -> 33 slices: the last early combine, the first general one (one pass, 33 = 4 * 8 + 1: the tail loop runs once)
    2063,               # context 2064: 33 slices, the last block cut to 16
    4095, 4096,         # 64 -> 65 slices: the second 64-slice max/sum pass holds one slice
    4159, 4160,         # 65 -> 66 slices
    16383, 16384,       # 256 -> 257 slices: the second weight chunk holds one slice (its 8-wide loop does not run, the tail does)
    16447, 16448,       # 257 -> 258 slices
)
DECODE_GROUPS = ((4, 2), (7, 2), (8, 2), (1, 4))    # (group, nkv): one head block; blocks of 4 + 3; 4 + 4; one head (lanes 16 .. 63 idle)
REGIME_POS = (64, 2048, 4160, 16448)                # one position per combine regime: the fp16 build, the graded weights, the fused lab form
# vl2_attn_decode_batched / _kv8_batched: B = 5 requests of different regimes in one launch; a second mix reaches the weight chunks
BATCH_POS = ((0, 64, 2048, 4160, 63), (16448, 15, 4095, 2047, 16383))
# vl2_attn_decode_shared: (P, own_cap, nb, own lengths = pos - P per request (cycled)), from attn_shared_split (vl2_abi.hip)
SHARED_CASES = (
    (1, 64, 1, (0,)),                       # one prefix key: one split, one ragged tile
    (127, 64, 5, (0, 63, 1, 5, 62)),        # one split of two tiles, the second ragged
    (128, 64, 5, (0, 63, 7, 33, 1)),        # ... full
    (129, 128, 5, (0, 63, 64, 1, 127)),     # the second split holds one key; own rows in two slices
    (1000, 64, 33, (0, 63, 31)),            # ragged P between: 16 tiles, 8 splits; 33 requests x group rows = more than one 128-row block
    (3072, 512, 5, (0, 63, 64, 511, 448)),  # 48 tiles -> 24 splits of 2; own_cap 512: up to 32 slices, the last early combine
    (3072, 576, 5, (575, 512, 0, 64, 63)),  # ... 33 slices: the general combine
    (3073, 576, 5, (0, 575, 64, 63, 513)),  # 49 tiles -> splits of 3: 17 splits
    (3073, 64, 33, (0, 63, 32)),
)
SHARED_GROUPS = ((4, 2), (7, 2))
# vl2_attn_append: (P, n, group, nkv), from attn_append_split (vl2_abi.hip) and attn_append_kernel (128 rows = n * group per block)
APPEND_CASES = (
    (0, 1, 4, 2),           # pure causal, one row, one key
    (0, 40, 4, 2),          # pure causal: 160 rows = two row blocks
    (100, 1, 4, 2),         # n = 1: two tiles, one split
    (300, 32, 4, 2),        # n * group = 128 rows: one full block
    (300, 33, 4, 2),        # 132: a second block of four rows (a wave with four live lanes, three idle waves)
    (300, 18, 7, 2),        # 126 rows, group 7
    (300, 19, 7, 2),        # 133
    (60, 8, 4, 2),          # P + n = 68 crosses the 64-key tile edge inside the new rows
    (90, 64, 4, 2),         # 256 rows = two blocks, two splits of 128 keys: the first block's rows end at key 121, so its workgroup of split 1
                            # returns early and the combine must not read that partial
    (1000, 64, 4, 2),       # 17 tiles in 9 splits of 2, the last split one tile
    (3990, 43, 4, 1),       # P + n = 4033: 64 tiles, nkv * row blocks = 2 -> the maximum of 32 splits
    (4000, 64, 8, 1),       # group 8: four row blocks, 64 tiles in 32 splits
)


# ---------------------------------------------------------------------------------------------------------------- inputs
def salt(b, hk):
    """Rotation of the one-hot digit positions for (request b, kv head hk): another request's or another kv head's K rows never match."""
    return (5 * hk + 11 * b) % 32


def k_rows(nkv, b, keys):
    """K rows [nkv, len(keys), 128] (fp32 zeros and ones) of the absolute positions `keys` for request b."""
    keys = torch.as_tensor(keys, dtype=torch.int64)
    out = torch.zeros((nkv, keys.numel(), HD), dtype=torch.float32)
    r = torch.arange(keys.numel())
    for hk in range(nkv):
        for i in range(4):
            out[hk, r, 32 * i + (((keys >> (5 * i)) & 31) + salt(b, hk)) % 32] = 1.0
    return out


class World:
    """The V rows of every key, computed once and left unchanged: integers in [-15, 15] times a per-row power of two.  Request b reads them
    rolled by 131 b keys, so that no two requests share a row."""

    def __init__(self, nkv=4, n=N_WORLD, seed=0):
        g = torch.Generator().manual_seed(seed)
        ints = torch.randint(-15, 16, (nkv, n, HD), generator=g)
        exps = torch.randint(-2, 3, (nkv, n, 1), generator=g)
        self.V = (ints.double() * torch.exp2(exps.double())).float()
        self.n = n

    def v_rows(self, nkv, b, keys):
        keys = torch.as_tensor(keys, dtype=torch.int64)
        return self.V[:nkv, (keys + 131 * b) % self.n]


_WORLD = None


def world():
    global _WORLD
    if _WORLD is None:
        _WORLD = World()
    return _WORLD


def rope_tables(rows):
    """cos / sin fp32 [rows, 64]: entry (p, d) is exact rotation number (p + d) % 4 of (1,0), (0,1), (-1,0), (0,-1)."""
    k = (torch.arange(rows)[:, None] + torch.arange(HALF)[None, :]) % 4
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[k]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[k]
    return cos.contiguous(), sin.contiguous()


def rope(x, cos, sin):
    """rotate-half RoPE of x [.., 128] by one table row (HF apply_rotary_pos_emb), in the dtype of x."""
    x1, x2 = x[..., :HALF], x[..., HALF:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1)


def unrope(w, cos, sin):
    """The inverse rotation; + 0.0 turns a -0 into +0."""
    w1, w2 = w[..., :HALF], w[..., HALF:]
    return torch.cat([w1 * cos + w2 * sin, w2 * cos - w1 * sin], -1) + 0.0


def q_pattern(sel, s):
    """The roped query [128] of selector `sel` = 4 digits (None = wildcard) against K rows of salt `s`."""
    q = torch.full((HD,), NEG, dtype=torch.float64)
    for i, d in enumerate(sel):
        if d is None:
            q[32 * i:32 * i + 32] = 0.0
        else:
            q[32 * i + (d + s) % 32] = 0.0
    return q


def digits(j):
    return tuple((j >> (5 * i)) & 31 for i in range(4))


def matches(sel, keys):
    """bool [len(keys)]: the keys a selector selects."""
    keys = torch.as_tensor(keys, dtype=torch.int64)
    m = torch.ones(keys.shape, dtype=torch.bool)
    for i, d in enumerate(sel):
        if d is not None:
            m &= ((keys >> (5 * i)) & 31) == d
    return m


def _pow2(n):
    return n >= 1 and n & (n - 1) == 0


def _wild(j, *which):
    return tuple(None if i in which else d for i, d in enumerate(digits(j)))


def selectors(last, first=0):
    """The selectors of a query that sees the keys first .. last (decode: last = pos = the appended key; append row i: last = P + i), each with
    a power-of-two number of visible keys by construction:
      single keys   : key 0 (`first`), the appended / diagonal key, the one before it, the last key of a slice and the first of the next
                      (at the end of the context and at 63 | 64), the wave edge 15 | 16, a key in the middle of the last, ragged slice;
      wildcard sets : digit 0 = 32 consecutive keys (one slice, two waves), the block the context ends in when the context cuts it to a power
                      of two, else the last full one; digit 1 = 32 keys 32 apart (16 slices of equal weight), cut by the context where a
                      residue gives a power of two; digits 0 and 1 = 1024 keys; digit 2 = keys 1024 apart (across the 64-slice passes and
                      the 256-slice chunks of the combine), the residue chosen for a power of two; digits 0 and 2 = 32-key blocks 1024 apart."""
    ctx = last + 1
    keys = torch.arange(first, ctx)
    out = []

    def add(sel):
        n = int(matches(sel, keys).sum())
        if _pow2(n) and sel not in out:
            out.append(sel)
            return True
        return False

    s = last // 64 * 64
    for j in (first, last, last - 1, s - 1, s, 63, 64, 15, 16, s + (last - s) // 2, first + (last - first) // 2):
        if first <= j <= last:
            add(digits(j))
    b = last // 32
    add(_wild(32 * b, 0))                                                    # the context's last block, where the cut is a power of two
    if b >= 1:
        add(_wild(32 * (b - 1), 0))                                          # the last full block
    add(_wild(0, 0))
    hi = last // 1024 * 1024
    for base in (hi, 0):                                                     # 32 apart: the first residue with a power-of-two count, a cut one first
        cands = sorted({last % 32, ctx % 32, 0, 31}, key=lambda d0: int(matches(_wild(base + d0, 1), keys).sum()) == 32)
        any(add(_wild(base + d0, 1)) for d0 in cands)
    add(_wild(hi, 0, 1))                                                     # what the context leaves of its last 1024 keys
    add(_wild(0, 0, 1))                                                      # 1024 keys
    any(add(_wild(lo, 2)) for lo in (last % 1024, ctx % 1024, 64, 0, 63, 1023) if lo <= last)     # 1024 apart
    any(add(_wild(lo, 0, 2)) for lo in (last % 1024 // 32 * 32, 64, 0, 992))                      # blocks 1024 apart
    assert out
    return out


_KEYS64 = (None, None, None)


class Request:
    """One new token of one request: its selectors per q head, its un-roped qkv row, the fp64 reference, the guard.
    keys [first_abs .. pos] are visible; `b` salts K and rolls V."""

    def __init__(self, group, nkv, pos, b=0, rnd=0, sels=None):
        self.group, self.nkv, self.nh, self.pos, self.b = group, nkv, group * nkv, pos, b
        pats = sels if sels is not None else selectors(pos)
        nh = self.nh
        self.sel = [pats[(rnd * nh + h + 3 * b) % len(pats)] for h in range(nh)]
        self.rounds = (len(pats) + nh - 1) // nh
        k4 = (pos + torch.arange(HALF)) % 4                      # row `pos` of rope_tables
        self.cos, self.sin = torch.tensor([1.0, 0.0, -1.0, 0.0])[k4].double(), torch.tensor([0.0, 1.0, 0.0, -1.0])[k4].double()
        qw = torch.stack([q_pattern(self.sel[h], salt(b, h // group)) for h in range(nh)])
        kw = k_rows(nkv, b, [pos])[:, 0].double()
        self.v_new = world().v_rows(nkv, b, [pos])[:, 0].double()
        self.qkv64 = torch.cat([unrope(qw, self.cos, self.sin).reshape(-1), unrope(kw, self.cos, self.sin).reshape(-1), self.v_new.reshape(-1)])
        # what the kernel must compute from the un-roped row: the reference ropes it itself
        self.q = rope(self.qkv64[:nh * HD].view(nh, HD), self.cos, self.sin)
        self.k_new = rope(self.qkv64[nh * HD:(nh + nkv) * HD].view(nkv, HD), self.cos, self.sin)
        assert torch.equal(self.q, qw) and torch.equal(self.k_new, kw)

    def qkv(self, elem):
        t = self.qkv64.to(elem)
        assert torch.equal(t.double(), self.qkv64), "qkv is not exact in the element type"
        return t

    def keys64(self):
        """(K, V) fp64 [nkv, pos + 1, 128] of the visible keys: the resident rows and the appended one."""
        global _KEYS64
        key = (self.nkv, self.b, self.pos)
        if _KEYS64[0] != key:                        # the last one is kept: the launches of one case share it
            r = torch.arange(self.pos)
            K = torch.cat([k_rows(self.nkv, self.b, r).double(), self.k_new[:, None]], 1)
            V = torch.cat([world().v_rows(self.nkv, self.b, r).double(), self.v_new[:, None]], 1)
            _KEYS64 = (key, K, V)
        return _KEYS64[1], _KEYS64[2]

    def reference(self, K=None, V=None):
        """(fp64 softmax attention [nh * 128] over the visible keys, the guard's figures).  Asserts the guard."""
        if K is None:
            K, V = self.keys64()
        return softmax_reference(self.q, K, V, self.group), guard(self.q, K, V, self.group, f"pos {self.pos} request {self.b}")

    def coords(self):
        return f"group {self.group} nkv {self.nkv} pos {self.pos} request {self.b}"


def softmax_reference(q, K, V, group, limits=None):
    """Plain softmax attention in fp64: q [nh, 128] (roped), K / V [nkv, keys, 128], the product's scale -> [nh * 128].  limits [nh]: head h sees
    the keys 0 .. limits[h] only (append)."""
    out = []
    for h in range(q.shape[0]):
        n = K.shape[1] if limits is None else limits[h] + 1
        p = torch.softmax((K[h // group, :n] @ q[h]) * SCALE, 0)
        out.append(p @ V[h // group, :n])
    return torch.cat(out)


def guard(q, K, V, group, what="", limits=None):
    """THE GUARD, in fp64, for every head: max score == 0, every other score <= GAP (exp2 domain), a power-of-two number of selected keys,
    sum |V| / quantum < 2^24 over them, V on the quantum.  -> [selected keys per head]."""
    assert bool(((V / V_QUANTUM) == (V / V_QUANTUM).round()).all()), f"{what}: V is not a multiple of the quantum"
    counts = []
    for h in range(q.shape[0]):
        n = K.shape[1] if limits is None else limits[h] + 1
        s = (K[h // group, :n] @ q[h]) * (SCALE * LOG2E)
        hit = s == 0.0
        cnt = int(hit.sum())
        assert float(s.max()) == 0.0 and cnt >= 1, f"{what} head {h}: the maximum score is {float(s.max())}, not 0"
        assert cnt == n or float(s[~hit].max()) <= GAP, f"{what} head {h}: a non-selected key scores {float(s[~hit].max())} > {GAP}"
        assert _pow2(cnt), f"{what} head {h}: {cnt} selected keys is not a power of two"
        mag = float(V[h // group, :n][hit].abs().sum(0).max()) / V_QUANTUM
        assert mag < 2.0 ** 24, f"{what} head {h}: sum |V| / quantum = {mag} >= 2^24"
        counts.append(cnt)
    return counts


def poisoned_cache(req, smax, elem, resident=None):
    """(k, v) [nkv, smax, 128] in `elem`: rows 0 .. pos - 1 resident (exact), every row from `pos` on NaN."""
    k = torch.full((req.nkv, smax, HD), float("nan"), dtype=elem)
    v = torch.full((req.nkv, smax, HD), float("nan"), dtype=elem)
    r = torch.arange(req.pos)
    k[:, :req.pos] = k_rows(req.nkv, req.b, r).to(elem)
    vr = world().v_rows(req.nkv, req.b, r)
    v[:, :req.pos] = vr.to(elem)
    assert torch.equal(v[:, :req.pos].float(), vr), "V is not exact in the element type"
    return k, v


def kv8_of(k16, v16, pos):
    """The fp8 cache (k8, v8, ks, vs) of a poisoned 16-bit cache: rows below pos through the definition's quantiser (tests/fp8kv_oracle.py),
    which must return them unchanged (the round trip, asserted); rows from pos on 0x7F codes and NaN scales."""
    from tests import fp8kv_oracle as KV
    nkv, smax, _ = k16.shape
    k8 = torch.full((nkv, smax, HD), 0x7F, dtype=torch.uint8)
    v8 = torch.full((nkv, smax, HD), 0x7F, dtype=torch.uint8)
    ks = torch.full((nkv, smax), float("nan"), dtype=torch.float32)
    vs = torch.full((nkv, smax), float("nan"), dtype=torch.float32)
    if pos:
        (k8[:, :pos], ks[:, :pos]), (v8[:, :pos], vs[:, :pos]) = KV.quant_cache_rows(k16[:, :pos]), KV.quant_cache_rows(v16[:, :pos])
        assert torch.equal(KV.dequant_cache(k8[:, :pos], ks[:, :pos]), k16[:, :pos].float()), "fp8 round trip of K"
        assert torch.equal(KV.dequant_cache(v8[:, :pos], vs[:, :pos]), v16[:, :pos].float()), "fp8 round trip of V"
    return k8, v8, ks, vs


def partial_ws(floats, dev):
    """(storage, view): a NaN workspace of `floats` floats between two NaN guard bands."""
    st = torch.full((floats + 2 * BAND,), float("nan"), dtype=torch.float32, device=dev)
    return st, st[BAND:BAND + floats]


def bands_intact(st):
    return bool(st[:BAND].isnan().all()) and bool(st[-BAND:].isnan().all())


def bits(t):
    """The storage bits of a 16-bit, fp32 or uint8 tensor: NaN poison compares equal to itself."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def expected(ref64, elem):
    """THE answer: the fp64 value rounded once to the element type."""
    return ref64.to(elem)


def first_bad(y, exp):
    """Indices of the flat outputs that differ from the exact ones (a NaN differs from everything)."""
    return torch.nonzero((y != exp) | y.isnan()).flatten()


def first_diff(y, exp, hd=HD):
    bad = first_bad(y, exp)
    i = int(bad[0])
    return f"{bad.numel()} of {y.numel()} outputs differ, first at head {i // hd} dim {i % hd}: got {y[i].item()!r}, exact {exp[i].item()!r}"


# ---------------------------------------------------------------------------------------------------------------- vl2_attn_decode
DECODE_FORMS = ("static", "cap_pos1", "cap_64", "cap_smax")     # pos by value; *pos_dev with ctx_cap = pos + 1, the next multiple of 64, smax


def smax_for(pos):
    """Cache rows of a case: a slice of poisoned rows past the one the context ends in."""
    return (pos + 64) // 64 * 64 + 64


def ctx_cap_of(form, pos, smax):
    return {"static": 0, "cap_pos1": pos + 1, "cap_64": (pos + 64) // 64 * 64, "cap_smax": smax}[form]


class DecodeState:
    """Device state of one (group, nkv, pos) case, shared by its launches: the poisoned caches (16-bit or fp8) and their pristine copies."""

    def __init__(self, group, nkv, pos, elem, dev, kv8=False):
        self.group, self.nkv, self.pos, self.elem, self.dev, self.kv8 = group, nkv, pos, elem, dev, kv8
        self.smax = smax_for(pos)
        req = Request(group, nkv, pos)
        self.rounds = req.rounds
        k, v = poisoned_cache(req, self.smax, elem)
        host = kv8_of(k, v, pos) if kv8 else (k, v)
        self.pristine = tuple(t.to(dev) for t in host)
        self.cache = tuple(t.clone() for t in self.pristine)
        cos, sin = rope_tables(self.smax)
        self.cos, self.sin = cos.to(dev), sin.to(dev)


def take_row(cache, pristine, pos):
    """Row `pos` of every tensor of a cache [nkv, smax, ..] (CPU copies); the row is put back to its pristine bits."""
    row = [c[:, pos].clone().cpu() for c in cache]
    for c, p in zip(cache, pristine):
        c[:, pos] = p[:, pos]
    return row


def new_row_error(req, row, elem, kv8, what):
    """The appended row holds the roped k_new and v_new (kv8: their quantisation by the definition -- codes up to the sign of a zero -- and
    scales, and it dequantises to them).  -> error or None."""
    if not kv8:
        if not (torch.equal(row[0].double(), req.k_new) and torch.equal(row[1].double(), req.v_new)):
            return f"{what}: cache row {req.pos} is not the roped k_new / v_new"
        return None
    from tests import fp8kv_oracle as KV
    nz = lambda c: torch.where((c & 0x7F) == 0, torch.zeros_like(c), c)
    for name, codes, sc, want in (("K", row[0], row[2], req.k_new), ("V", row[1], row[3], req.v_new)):
        q, s = KV.quant_cache_rows(want.to(elem)[:, None])
        if not (torch.equal(nz(codes), nz(q[:, 0])) and torch.equal(sc, s[:, 0])):
            return f"{what}: fp8 {name} row {req.pos} is not the definition's quantisation of the new row"
        if not torch.equal(KV.dequant_cache(codes[:, None], sc[:, None])[:, 0].double(), want):
            return f"{what}: fp8 {name} row {req.pos} does not dequantise to the new row"
    return None


def run_decode(ops, st, form, rnd, fused_cnt=None):
    """One launch of vl2_attn_decode (or _kv8; fused_cnt: vl2_attn_decode_fused) on state `st` in `form` with the selectors of round `rnd`.
    -> error or None."""
    req = Request(st.group, st.nkv, st.pos, rnd=rnd)
    ref, _ = req.reference()
    exp = expected(ref, st.elem)
    nh, pos, dev = req.nh, st.pos, st.dev
    cap = ctx_cap_of(form, pos, st.smax)
    nsplit = (st.smax + 63) // 64 if fused_cnt is not None else ((cap if cap else pos + 1) + 63) // 64
    pst, partial = partial_ws(nh * nsplit * 130, dev)
    out_st = torch.full((nh * HD + 256,), SENTINEL, dtype=st.elem, device=dev)
    out = out_st[128:128 + nh * HD]
    qkv = req.qkv(st.elem).to(dev)
    pos_dev = None if form == "static" else torch.tensor([pos], dtype=torch.int32, device=dev)
    what = f"{req.coords()} {form} round {rnd}{' kv8' if st.kv8 else ''}{' fused' if fused_cnt is not None else ''}"
    if fused_cnt is not None:
        fused_cnt.zero_()
        ops.attn_decode_fused(qkv, st.cache[0], st.cache[1], st.cos, st.sin, partial, out, nh, st.nkv, pos_dev, SCALE, fused_cnt)
    elif st.kv8:
        ops.attn_decode_kv8(qkv, st.cache, st.cos, st.sin, partial, out, nh, st.nkv, pos, SCALE, pos_dev=pos_dev, ctx_cap=cap)
    else:
        ops.attn_decode(qkv, st.cache[0], st.cache[1], st.cos, st.sin, partial, out, nh, st.nkv, pos, SCALE, pos_dev=pos_dev, ctx_cap=cap)
    o = out_st.cpu()
    err = new_row_error(req, take_row(st.cache, st.pristine, pos), st.elem, st.kv8, what)
    if err:
        return err
    if not all(torch.equal(bits(c), bits(p)) for c, p in zip(st.cache, st.pristine)):
        return f"{what}: a cache row other than {pos} changed"
    if not (bool((o[:128] == SENTINEL).all()) and bool((o[128 + nh * HD:] == SENTINEL).all())):
        return f"{what}: the sentinel around the output was overwritten"
    if not bands_intact(pst.cpu()):
        return f"{what}: a guard band of the partial workspace was written"
    y = o[128:128 + nh * HD]
    if not torch.equal(y, exp):
        return f"{what}: {first_diff(y, exp)}"
    return None


def decode_launches(rounds, every_round=False):
    """[(form, round)]: every form once, each with another round of selectors; every_round: and every round of selectors once.  (With fewer
    than 8 heads four rounds do not reach every selector of a position; the other groups do.)"""
    return [(DECODE_FORMS[i % 4], i % rounds) for i in range(max(4, rounds) if every_round else 4)]


# ---------------------------------------------------------------------------------------------------------------- vl2_attn_decode_batched
class Batch:
    """B requests in one launch, every operand strided and poisoned: qkv rows of width + 24 in B + 2 rows, cache slots of nkv * smax * 128 +
    128 elements in B + 2 slots (kv8: codes likewise, scales + 4), out rows of width + 8 in B + 2 rows pre-filled with the sentinel.
    dead = indices of requests whose position is moved to smax + (0 | 3): they must write nothing (their output is unspecified)."""

    def __init__(self, group, nkv, positions, elem, dev, kv8=False, dead=()):
        self.group, self.nkv, self.nh, self.elem, self.dev, self.kv8, self.dead = group, nkv, group * nkv, elem, dev, kv8, tuple(dead)
        B = self.B = len(positions)
        self.smax = smax_for(max(positions))
        self.reqs = [Request(group, nkv, p, b=b, rnd=b) for b, p in enumerate(positions)]
        nan = float("nan")
        w = (self.nh + 2 * nkv) * HD
        qst = torch.full((B + 2, w + 24), nan, dtype=elem)
        for b, r in enumerate(self.reqs):
            qst[b + 1, :w] = r.qkv(elem)
        self.qkv_st = qst.to(dev)
        self.qkv = self.qkv_st[1:B + 1, :w]
        slot = nkv * self.smax * HD
        caches = [poisoned_cache(r, self.smax, elem) for r in self.reqs]
        if kv8:
            parts = [kv8_of(k, v, r.pos) for (k, v), r in zip(caches, self.reqs)]
            fill = (0x7F, 0x7F, nan, nan)
            sizes = (slot, slot, nkv * self.smax, nkv * self.smax)
            pads = (128, 128, 4, 4)
        else:
            parts, fill, sizes, pads = caches, (nan, nan), (slot, slot), (128, 128)
        self.cache_st, self.cache = [], []
        for i, (f, n, pad) in enumerate(zip(fill, sizes, pads)):
            stg = torch.full((B + 2, n + pad), f, dtype=parts[0][i].dtype)
            for b in range(B):
                stg[b + 1, :n] = parts[b][i].reshape(-1)
            stg = stg.to(dev)
            self.cache_st.append(stg)
            self.cache.append(stg[1:B + 1, :n].view((B, nkv, self.smax, HD) if n == slot else (B, nkv, self.smax)))
        self.pristine = [s.clone() for s in self.cache_st]
        cos, sin = rope_tables(self.smax + 8)
        self.cos, self.sin = cos.to(dev), sin.to(dev)
        pos = [self.smax + 3 * (b % 2) if b in self.dead else r.pos for b, r in enumerate(self.reqs)]
        self.pos_dev = torch.tensor(pos, dtype=torch.int32, device=dev)

    def run(self, ops, ctx_cap):
        """-> (error or None, out [B, nh * 128] CPU)."""
        B, nh, dev = self.B, self.nh, self.dev
        nsplit = (ctx_cap + 63) // 64
        pst, partial = partial_ws(B * nh * nsplit * 130, dev)
        out_st = torch.full((B + 2, nh * HD + 8), SENTINEL, dtype=self.elem, device=dev)
        out = out_st[1:B + 1, :nh * HD]
        if self.kv8:
            ops.attn_decode_kv8_batched(self.qkv, tuple(self.cache), self.cos, self.sin, partial, out, nh, self.nkv, self.pos_dev, ctx_cap, SCALE)
        else:
            ops.attn_decode_batched(self.qkv, self.cache[0], self.cache[1], self.cos, self.sin, partial, out, nh, self.nkv, self.pos_dev, ctx_cap, SCALE)
        o = out_st.cpu()
        what = f"batched group {self.group} positions {[r.pos for r in self.reqs]} dead {self.dead} ctx_cap {ctx_cap}{' kv8' if self.kv8 else ''}"
        keep = torch.ones(o.shape, dtype=torch.bool)
        keep[1:B + 1, :nh * HD] = False
        if not bool((o[keep] == SENTINEL).all()):
            return f"{what}: the sentinel around the outputs was overwritten", None
        if not bands_intact(pst.cpu()):
            return f"{what}: a guard band of the partial workspace was written", None
        errs = []
        for b, r in enumerate(self.reqs):
            if b in self.dead:
                continue
            exp = expected(r.reference()[0], self.elem)
            if not torch.equal(o[b + 1, :nh * HD], exp):
                errs.append(f"{what} request {b} (pos {r.pos}): {first_diff(o[b + 1, :nh * HD], exp)}")
        # the caches: slot b row pos holds the new row; everything else -- pads, the extra slots, a dead request's whole slot -- keeps its bits
        for b, r in enumerate(self.reqs):
            if b in self.dead:
                continue
            pr = [p[b + 1, :c[b].numel()].view(c[b].shape) for p, c in zip(self.pristine, self.cache)]
            e = new_row_error(r, take_row([c[b] for c in self.cache], pr, r.pos), self.elem, self.kv8, f"{what} request {b}")
            if e:
                errs.append(e)
        for s, p in zip(self.cache_st, self.pristine):
            if not torch.equal(bits(s), bits(p)):
                errs.append(f"{what}: cache bits outside the appended rows changed (a pad, an extra slot, a dead request or another row)")
                s.copy_(p)
        return ("\n".join(errs) or None), o[1:B + 1, :nh * HD].clone()


def batched_errors(ops, group, nkv, positions, elem, dev, kv8=False):
    """The batched entry on one mix of positions: ctx_cap = the longest context, the next multiple of 64 and smax; row stability (a request
    alone, on its own slot, gives the bits it has in the batch); and a launch in which requests 1 and 4 sit at or past the cache end -- they
    must write nothing and leave their neighbours exact.  -> [errors]."""
    errs = []
    bt = Batch(group, nkv, positions, elem, dev, kv8=kv8)
    top = max(positions) + 1
    first = None
    for cap in sorted({top, (top + 63) // 64 * 64, bt.smax}):
        err, o = bt.run(ops, cap)
        if err:
            return errs + [err]
        first = o if first is None else first
    nh = group * nkv
    for b, r in enumerate(bt.reqs):
        one = torch.full((nh * HD,), SENTINEL, dtype=elem, device=dev)
        _, partial = partial_ws(nh * ((r.pos + 64) // 64) * 130, dev)
        qkv = bt.qkv[b].contiguous()
        if kv8:
            ops.attn_decode_kv8(qkv, tuple(c[b] for c in bt.cache), bt.cos, bt.sin, partial, one, nh, nkv, r.pos, SCALE)
        else:
            ops.attn_decode(qkv, bt.cache[0][b], bt.cache[1][b], bt.cos, bt.sin, partial, one, nh, nkv, r.pos, SCALE)
        if not torch.equal(one.cpu(), first[b]):
            errs.append(f"batched group {group} positions {positions}: request {b} alone differs from its row in the batch")
    dead = Batch(group, nkv, positions, elem, dev, kv8=kv8, dead=(1, 4))
    err, _ = dead.run(ops, dead.smax)
    return errs + ([err] if err else [])


# ---------------------------------------------------------------------------------------------------------------- graded weights
def random_decode_inputs(group, nkv, pos, elem, seed=0):
    """General random inputs (weights of every size, not only 0 and 1): qkv, poisoned caches [nkv, smax, 128] and real cos/sin tables, with the
    fp64 softmax reference of the kernel's definition (q and k_new roped in fp64 and rounded to the element type as the kernel rounds them)."""
    g = torch.Generator().manual_seed(1000 * group + pos + seed)
    nh, smax = group * nkv, smax_for(pos)
    qkv = (torch.randn((nh + 2 * nkv) * HD, generator=g) * 1.5).to(elem)
    k = torch.full((nkv, smax, HD), float("nan"), dtype=elem)
    v = torch.full((nkv, smax, HD), float("nan"), dtype=elem)
    k[:, :pos] = torch.randn(nkv, pos, HD, generator=g).to(elem)
    v[:, :pos] = torch.randn(nkv, pos, HD, generator=g).to(elem)
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.int64).float() / HD))
    fr = torch.arange(smax, dtype=torch.float32)[:, None] * inv[None, :]
    cos, sin = fr.cos().contiguous(), fr.sin().contiguous()
    c, s = cos[pos].double(), sin[pos].double()
    q = rope(qkv[:nh * HD].double().view(nh, HD), c, s).to(elem).double()
    kn = rope(qkv[nh * HD:(nh + nkv) * HD].double().view(nkv, HD), c, s).to(elem).double()
    vn = qkv[(nh + nkv) * HD:].double().view(nkv, HD)
    K = torch.cat([k[:, :pos].double(), kn[:, None]], 1)
    V = torch.cat([v[:, :pos].double(), vn[:, None]], 1)
    return dict(qkv=qkv, k=k, v=v, cos=cos, sin=sin, ref=softmax_reference(q, K, V, group), smax=smax, nh=nh)


# ---------------------------------------------------------------------------------------------------------------- vl2_attn_decode_shared
def shared_splits(P):
    """attn_shared_split (vl2_abi.hip) restated: (keys per split, splits)."""
    chunk = max(((P + 63) // 64 + 23) // 24, 2) * 64
    return chunk, (P + chunk - 1) // chunk


class SharedCase:
    """nb requests over a shared prefix of P keys (request 0's K / V world: salt and roll 0 for every request) and own rows P .. pos (the same
    world: a request's own rows continue the prefix, so one selector can straddle the boundary).  Selectors of request b: `selectors(pos)`
    -- they aim into the prefix, into the own rows, at the new row and at sets across P -- plus the keys P - 1 and P."""

    def __init__(self, P, own_cap, nb, owns, group, nkv, elem, dev):
        self.P, self.own_cap, self.nb, self.group, self.nkv, self.nh, self.elem, self.dev = P, own_cap, nb, group, nkv, group * nkv, elem, dev
        nan = float("nan")
        self.psmax = (P + 63) // 64 * 64 + 64
        self.reqs = []
        for b in range(nb):
            pos = P + owns[b % len(owns)]
            sels = selectors(pos)
            for j in (P - 1, P, P - 64, P + 63):
                if 0 <= j <= pos and digits(j) not in sels:
                    sels.insert(1, digits(j))
            r = Request(group, nkv, pos, b=0, rnd=0, sels=sels[b % len(sels):] + sels[:b % len(sels)])
            self.reqs.append(r)
        r0 = Request(group, nkv, P, b=0)
        kp, vp = poisoned_cache(r0, self.psmax, elem)                      # rows 0 .. P - 1, NaN from P on
        self.kprefix, self.vprefix = kp.to(dev), vp.to(dev)
        ko = torch.full((nb + 2, nkv, own_cap, HD), nan, dtype=elem)
        vo = torch.full((nb + 2, nkv, own_cap, HD), nan, dtype=elem)
        for b, r in enumerate(self.reqs):
            keys = torch.arange(P, r.pos)
            ko[b + 1, :, :r.pos - P] = k_rows(nkv, 0, keys).to(elem)
            vo[b + 1, :, :r.pos - P] = world().v_rows(nkv, b + 1, keys).to(elem)         # the own V rows are the request's alone
        self.kown_st, self.vown_st = ko.to(dev), vo.to(dev)
        self.pristine = (self.kown_st.clone(), self.vown_st.clone(), self.kprefix.clone(), self.vprefix.clone())
        w = (self.nh + 2 * nkv) * HD
        qst = torch.full((nb + 2, w + 24), nan, dtype=elem)
        for b, r in enumerate(self.reqs):
            qst[b + 1, :w] = r.qkv(elem)
        self.qkv_st = qst.to(dev)
        cos, sin = rope_tables(P + own_cap)
        self.cos, self.sin = cos.to(dev), sin.to(dev)
        self.pos_dev = torch.tensor([r.pos for r in self.reqs], dtype=torch.int32, device=dev)

    def run(self, ops):
        nb, nh, nkv, P, dev = self.nb, self.nh, self.nkv, self.P, self.dev
        w = (nh + 2 * nkv) * HD
        per = ops.shared_partial_floats(P, self.own_cap, nh)
        assert per == nh * (shared_splits(P)[1] + self.own_cap // 64) * 130
        pst, partial = partial_ws(nb * per, dev)
        out_st = torch.full((nb + 2, nh * HD + 8), SENTINEL, dtype=self.elem, device=dev)
        ops.attn_decode_shared(self.qkv_st[1:nb + 1, :w], self.kprefix, self.vprefix, self.kown_st[1:nb + 1], self.vown_st[1:nb + 1], self.cos,
                               self.sin, partial, out_st[1:nb + 1, :nh * HD], nh, nkv, P, self.pos_dev, SCALE)
        o = out_st.cpu()
        what = f"shared P {P} own_cap {self.own_cap} nb {nb} group {self.group}"
        keep = torch.ones(o.shape, dtype=torch.bool)
        keep[1:nb + 1, :nh * HD] = False
        if not bool((o[keep] == SENTINEL).all()):
            return f"{what}: the sentinel around the outputs was overwritten"
        if not bands_intact(pst.cpu()):
            return f"{what}: a guard band of the partial workspace was written"
        errs = []
        ko, vo = self.kown_st.cpu(), self.vown_st.cpu()
        pk, pv = self.pristine[0].cpu(), self.pristine[1].cpu()
        Kp, Vp = k_rows(nkv, 0, torch.arange(P)).double(), world().v_rows(nkv, 0, torch.arange(P)).double()
        for b, r in enumerate(self.reqs):
            keys = torch.arange(P, r.pos)
            K = torch.cat([Kp, k_rows(nkv, 0, keys).double(), r.k_new[:, None]], 1)
            V = torch.cat([Vp, world().v_rows(nkv, b + 1, keys).double(), r.v_new[:, None]], 1)
            exp = expected(r.reference(K, V)[0], self.elem)
            if not torch.equal(o[b + 1, :nh * HD], exp):
                errs.append(f"{what} request {b} (pos {r.pos}): {first_diff(o[b + 1, :nh * HD], exp)}")
            own = r.pos - P
            if not (torch.equal(ko[b + 1, :, own].double(), r.k_new) and torch.equal(vo[b + 1, :, own].double(), r.v_new)):
                errs.append(f"{what} request {b}: private row {own} is not the roped k_new / v_new")
            pk[b + 1, :, own], pv[b + 1, :, own] = ko[b + 1, :, own], vo[b + 1, :, own]
        if not (torch.equal(bits(ko), bits(pk)) and torch.equal(bits(vo), bits(pv))):
            errs.append(f"{what}: private cache bits outside the appended rows changed")
        if not (torch.equal(bits(self.kprefix), bits(self.pristine[2])) and torch.equal(bits(self.vprefix), bits(self.pristine[3]))):
            errs.append(f"{what}: the prefix cache changed")
        return "\n".join(errs) or None


# ---------------------------------------------------------------------------------------------------------------- vl2_attn_append
def append_splits(P, n, group, nkv):
    """attn_append_split (vl2_abi.hip) restated: (keys per split, splits)."""
    T, rb = (P + n + 63) // 64, (n * group + 127) // 128
    want = max(1, min((256 + nkv * rb - 1) // (nkv * rb), (T + 1) // 2, 32))
    tps = (T + want - 1) // want
    return tps * 64, (T + tps - 1) // tps


class AppendCase:
    """n roped query rows at positions P .. P + n - 1 over a cache that already holds the keys 0 .. P + n - 1 (NaN past them); row i sees the
    keys 0 .. P + i.  Head h of row i takes selector (i + h) of `selectors(P + i)`: its own key (the diagonal), P + i - 1, key 0, slice
    edges, and wildcard sets that the causal limit cuts to a power of two."""

    def __init__(self, P, n, group, nkv, elem, dev):
        self.P, self.n, self.group, self.nkv, self.nh, self.elem, self.dev = P, n, group, nkv, group * nkv, elem, dev
        nh = self.nh
        self.smax = (P + n + 63) // 64 * 64 + 64
        keys = torch.arange(P + n)
        K, V = k_rows(nkv, 0, keys), world().v_rows(nkv, 0, keys)
        k = torch.full((nkv, self.smax, HD), float("nan"), dtype=elem)
        v = torch.full((nkv, self.smax, HD), float("nan"), dtype=elem)
        k[:, :P + n], v[:, :P + n] = K.to(elem), V.to(elem)
        assert torch.equal(v[:, :P + n].float(), V)
        self.k, self.v = k.to(dev), v.to(dev)
        qst = torch.full((n + 2, nh * HD + 8), float("nan"), dtype=elem)
        ref = []
        K64, V64 = K.double(), V.double()
        for i in range(n):
            sels = selectors(P + i)
            q = torch.stack([q_pattern(sels[(i + h) % len(sels)], salt(0, h // group)) for h in range(nh)])
            lim = [P + i] * nh
            guard(q, K64, V64, group, f"append P {P} row {i}", limits=lim)
            ref.append(softmax_reference(q, K64, V64, group, limits=lim))
            qst[i + 1, :nh * HD] = q.reshape(-1).to(elem)
        self.ref = torch.stack(ref)
        self.q_st = qst.to(dev)

    def run(self, ops):
        P, n, nh, dev = self.P, self.n, self.nh, self.dev
        T = (P + n + 63) // 64
        need = nh * n * min(T, 32) * 130
        assert append_splits(P, n, self.group, self.nkv)[1] <= min(T, 32)
        pst, ws = partial_ws(need, dev)
        out_st = torch.full((n + 2, nh * HD + 8), SENTINEL, dtype=self.elem, device=dev)
        k0, v0 = self.k.clone(), self.v.clone()
        ops.attn_append(self.q_st[1:n + 1, :nh * HD], self.k, self.v, out_st[1:n + 1, :nh * HD], P, nh, self.nkv, SCALE, ws=ws)
        o = out_st.cpu()
        what = f"append P {P} n {n} group {self.group} nkv {self.nkv}"
        keep = torch.ones(o.shape, dtype=torch.bool)
        keep[1:n + 1, :nh * HD] = False
        if not bool((o[keep] == SENTINEL).all()):
            return f"{what}: the sentinel around the outputs was overwritten"
        if not bands_intact(pst.cpu()):
            return f"{what}: a guard band of the workspace was written"
        if not (torch.equal(bits(self.k), bits(k0)) and torch.equal(bits(self.v), bits(v0))):
            return f"{what}: the caches changed"
        y, exp = o[1:n + 1, :nh * HD], expected(self.ref, self.elem)
        if not torch.equal(y, exp):
            bad = torch.nonzero(((y != exp) | y.isnan()).any(1)).flatten()
            i = int(bad[0])
            return f"{what}: {bad.numel()} of {n} rows differ, first row {i}: {first_diff(y[i], exp[i])}"
        return None
