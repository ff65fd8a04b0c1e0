"""TEST INFRASTRUCTURE ONLY -- exact key-selecting inputs for vl2_attn_fwd (prefill, extend beyond 64 rows, both vision towers): the 16 kernel
instances of csrc/k_attn.h and csrc/k_attn2.h.  Generators, the guard, the fp64 reference and the case tables of
tests/test_gpu_attn_fwd_edges.py, tests/test_attn_fwd_edges_emu.py and the variant-5 cases of tests/test_gpu_lab.py.

THE RULE is that of tests/attn_exact.py (section 18), for head_dim D: K row j is D / 32 base-32 digits of j, digit i one-hot in dims 32 i ..
32 i + 31, rotated by `salt(request, kv head)`; D = 128: 4 digits, D = 64: 2 digits (1024 keys), D = 96 as the SigLIP tower uses it: 2 digits,
dims 64 .. 71 carry -2048 in q against 0 in k, dims 72 .. 95 are zero in q, k and v and the scale is 72^-1/2 (one case uses all 96 dims: 3
digits, scale 96^-1/2).  A query holds -2048 except 0 at the wanted digit values: a digit is a 32-bit MASK of wanted values -- one bit = one
value, all bits = a wildcard, two bits = the trap below, every fourth bit = keys 128 apart.  A selected key scores exactly 0, every other
visible key at most -2048 * scale * log2(e) = -261 (D 128), -301 (96), -348 (72), -369 (64) in the exp2 domain: `guard` asserts <= -200 for
every row, it is not assumed.  exp2(0) = 1 and exp2(x <= -200) = 0 in fp32, so P is 0 or 1 and every online-softmax rescale factor
exp2(m_old - 0), m_old <= -200 or -1e30, is 0 -- as are the factors of the NG = 2 and NS = 2 merges and of the class key's initial state
(m = its score, l = 1, O = V[0]: kept when the class key is selected, multiplied by 0 when a tile brings the first selected key).  What a row
accumulates before its first selected key arrives (P = exp2(rounding residue) ~ 1 for the best keys so far) is finite and is multiplied by 0.
With V integers in [-15, 15] times a per-row power of two (quantum 2^-2) and a power-of-two count, (sum of the selected V rows) * (1 / count)
is exact in fp32 in every order.  THE answer is the plain fp64 softmax over the visible keys rounded ONCE to the element type: `torch.equal`.

THE TRAP.  Every row's list holds a selector whose digit 0 wants the two values {d, d + 1} of its last visible key `last`: it matches `last`
and `last + 1`, and only `last` is visible (count 1) -- a mask that lets one more key in gives count 2 and the mean of two rows.  Where d = 31
the two values are {31, 0}: a product of digit masks that holds `last` and `last + 1` (the next block's first key) cannot leave out
`last - 31`, so there the visible count is 2 (`last - 31` and `last`) and one more key gives three.  In the full-attention cases the same
selector covers keys nk - 1 and nk.  A key at or past nk is never READ: the buffer resource ends at nk, it arrives as zeros, and a zero K row
scores 0 for EVERY query -- it traps by itself, which is why an unmasked out-of-range key always shows (with the V row zero: every output
of the row is scaled by count / (count + 1)).

THE GUARD (`guard`, asserted for every (request, head, row) of every case before the launch, never used to filter a case): the maximum
visible score is exactly 0, every other visible score is <= -200, the number of selected keys is a power of two, sum |V| / quantum over them
is below 2^24, V is on the quantum; `Inputs.operands` asserts that every operand is exact in the element type.  The selectors of a row are
CHOSEN with a power-of-two visible count (`row_lists`); the guard then checks the tensors that are launched.

Poison and frames: NaN in every K / V row from nk to the capacity (>= 128 rows past it), in the row padding of the padded caches
(k_rs = v_rs = D + 8), in the q rows from nq on, in one whole request slot before and after the batch; the output sits in a sentinel frame
(a row before and after each request, o_rs = H D + 8 with the padding holding the sentinel) that must survive, and q, k, v must keep their bits.

Nothing under videollama2_amd/ imports this file."""
import collections
import functools

import torch

from tests.attn_exact import GAP, LOG2E, NEG, SENTINEL, V_QUANTUM, World, bits, expected, first_bad, first_diff, salt

ALL = 0xFFFFFFFF
NAN = float("nan")

Case = collections.namedtuple("Case", "table name D causal B H nkv nq nk off layout rpad used ndig")
# layout: "fused"   = the towers' buffer [B, rows, 3 H D]: q, k, v are column blocks of one row, equal strides (needs nq == nk, nkv == H);
#         "decoder" = q [S, H D] with q_bs = 0 and a cache [nkv, smax, D] with k_bs = v_bs = 0 (B = 1);
#         "batch"   = B requests with their own q and their own cache (q_bs, k_bs != 0), q rows padded by 8.
# rpad: elements of NaN padding behind every K / V row (fused: behind every row of the buffer).


def _case(table, D, causal, nq, nk=None, off=0, B=1, H=2, nkv=1, layout=None, rpad=0, used=None, ndig=None):
    nk = nq + off if nk is None else nk
    layout = layout or ("decoder" if causal and B == 1 else "batch" if causal else "fused")
    used = used or D
    ndig = ndig or (2 if D == 96 else D // 32)
    name = f"{table}:D{D}{'c' if causal else 'f'}_B{B}_H{H}_kv{nkv}_nq{nq}_nk{nk}_off{off}_{layout}{'_pad' if rpad else ''}{'_all96' if D == 96 and used == 96 else ''}"
    return Case(table, name, D, bool(causal), B, H, nkv, nq, nk, off, layout, rpad, used, ndig)


# ---------------------------------------------------------------------------------------------------------------- the case tables
# The smallest shapes that reach each edge (query blocks of 128 rows = four waves of 32; key tiles of 64; NG / NS = 2: the second group or
# stream takes the odd tiles), not the workload's.
CAUSAL_S = (                    # D = 128, off = 0, nk = S
    1,                          # one row, one key: three dead waves, 31 dead lanes
    31, 32, 33,                 # one wave's rows: the last row of wave 0 / the first of wave 1
    63, 64, 65,                 # 1 -> 2 tiles: at 64 the odd stream (second group) has no tile at all, at 65 one tile holding one key
    127, 128, 129,              # the query-block edge, 2 -> 3 tiles: the second group / stream is one tile short of the first
    200,                        # two query blocks, a ragged last tile (200 = 3 * 64 + 8)
    330,                        # three query blocks; rows 0 .. 63 of a block: their first odd-stream tile is wholly masked (m stays -1e30 -> -1e28 floor)
)
CAUSAL_GROUPS = (               # (H, nkv, B) at S = 130 (two query blocks, three tiles): h / group picks the kv head
    (8, 2, 1),                  # group 4 (Mistral)
    (14, 2, 1),                 # group 7 (Qwen2)
    (2, 2, 1),                  # group 1
    (4, 1, 1),                  # one kv head
    (8, 2, 3),                  # group 4 in a batch of three: b = g / heads, own q and cache per request, padded cache rows
)
EXTEND = (                      # (nq, off): nk = nq + off, key j visible to row i iff j <= i + off
    (1, 700),                   # one row over 11 tiles (700 = 10 * 64 + 60): the longest chain, the merge of 6 + 5 tiles
    (70, 260),                  # limit 388: off is no multiple of 64 or 32; padded cache rows
    (200, 260),                 # the first block's key limit q0 + 128 + off = 388 ends 4 keys into tile 6; the second block's is nk = 460
    (64, 64),                   # off = one tile: every row's diagonal sits in tile 1
    (130, 1),                   # off = 1: the diagonal one key past the row
    (128, 63),                  # off = 63: a wave's last row reaches the last key of the next tile
)
CAUSAL_NK_SHORT = (             # (nq, nk), off = 0: nk below the diagonal's reach -- the rows from nk on see nk keys, the last tile is cut by nk
    (200, 150),                 # nk = 22 mod 64
    (200, 191),                 # nk = 63 mod 64
    (200, 129),                 # nk = 1 mod 64: the last tile holds one key
)
CAUSAL_GRID = (1, 4, 6)         # B at H = 32, nkv = 8, S = 300 (nqb = 3): G = 32 -> nfirst >= nqb; G = 128 -> nfirst = 2, the n2 / alone order of
                                # variant 3, and 384 > 256 -> plain longest-first for variant 4; G = 192: 576 > 512 -> plain longest-first for variant 3
FULL_64_N = (                   # D = 64, nq = nk = N, group 1, the towers' fused buffer
    1, 63, 64, 65,              # one key; one ragged tile; one full tile; 65 = 1 + 64: class-token shape, 64 patch rows -> the class query in dead wave 2
    127, 128, 129,              # 129 = 1 + 128: class-token shape with a FULL last block -> the extra workgroup for the class query (cls_rem == 0)
    150, 191,                   # ragged, no class-token shape: 150 = 2 * 64 + 22, 191 = 3 * 64 - 1
    193,                        # 1 + 192: cls_rem = 64 -> dead wave 2 of block 1
    257,                        # 1 + 256: cls_rem == 0 -> the extra workgroup, two full patch blocks
    577,                        # the CLIP tower's: cls_rem = 64, nine peeled tiles
)
FULL_64_NQ_NK = ((100, 300), (300, 100))    # nq != nk: own q and caches per request (B = 3)
FULL_128_N = (64, 130, 191)     # D = 128 full attention: one tile; two blocks, three tiles; a tile short of three by one key
FULL_96_N = (63, 64, 65, 129, 200)          # D = 96 (k_attn.h only): one ragged tile, one full, the second tile with one key, block edge + 1, two blocks
CAUSAL_64_S = (65, 130, 200)    # D = 64 causal: built, unused by the product; variants 1, 3, 4
CAUSAL_AUTO_H = (176, 177)      # variant 0 only, S = 129 (nqb = 2): nqb * H = 352 -> two streams (variant 4), 354 -> one stream (variant 3)


def is_cls_shape(c):
    """vl2_attn_fwd's class-token shapes (csrc/vl2_abi.hip `cls_shape`): variants 0 and 4 peel the class token there."""
    return c.D == 64 and not c.causal and c.nq == c.nk and c.nk > 64 and (c.nk - 1) % 64 == 0 and c.H == c.nkv


def all_cases():
    out = [_case("CAUSAL_S", 128, True, S, rpad=8 if S == 129 else 0) for S in CAUSAL_S]
    out += [_case("CAUSAL_GROUPS", 128, True, 130, B=B, H=H, nkv=nkv, rpad=8 if B > 1 else 0) for H, nkv, B in CAUSAL_GROUPS]
    out += [_case("EXTEND", 128, True, nq, off=off, H=4, nkv=2, rpad=8 if (nq, off) == (70, 260) else 0) for nq, off in EXTEND]
    out += [_case("CAUSAL_NK_SHORT", 128, True, nq, nk=nk) for nq, nk in CAUSAL_NK_SHORT]
    out += [_case("CAUSAL_GRID", 128, True, 300, B=B, H=32, nkv=8) for B in CAUSAL_GRID]
    out += [_case("FULL_64", 64, False, N, B=2, H=2, nkv=2, rpad=8 if N in (150, 257) else 0) for N in FULL_64_N]
    out += [_case("FULL_64", 64, False, nq, nk=nk, B=3, H=2, nkv=2, layout="batch", rpad=8 if nq == 300 else 0) for nq, nk in FULL_64_NQ_NK]
    out += [_case("FULL_64", 64, False, 129, B=1, H=2, nkv=1, layout="decoder")]     # group 2 at a class-token N: the plain tiling under variant 0
    out += [_case("FULL_128", 128, False, N, B=2 if N == 130 else 1, H=2, nkv=2, rpad=8 if N == 191 else 0) for N in FULL_128_N]
    out += [_case("FULL_128", 128, False, 130, B=3, H=4, nkv=2, layout="batch", rpad=8)]
    out += [_case("FULL_96", 96, False, N, B=2, H=2, nkv=2, used=72, rpad=8 if N == 65 else 0) for N in FULL_96_N]
    out += [_case("FULL_96", 96, False, 129, B=1, H=2, nkv=2, used=96, ndig=3)]
    out += [_case("FULL_96", 96, False, 100, B=3, H=4, nkv=2, layout="batch", used=72, rpad=8)]
    out += [_case("CAUSAL_64", 64, True, S, rpad=8 if S == 130 else 0) for S in CAUSAL_64_S]
    out += [_case("CAUSAL_64", 64, True, 130, B=3, H=4, nkv=2, rpad=8)]
    out += [_case("CAUSAL_AUTO", 128, True, 129, H=H, nkv=1) for H in CAUSAL_AUTO_H]
    return out


def fp16_cases():
    """The fp16 build's share: one row per table edge class (one wave / tile edge / block edge / ragged / nk short / each grid order / each
    class-token path / nq != nk / each layout / padded rows) such that every kernel instance runs (asserted in tests/test_attn_fwd_edges_emu.py)."""
    keep = {"CAUSAL_S": (33, 65, 129, 330), "EXTEND": (1, 200), "CAUSAL_NK_SHORT": (200,), "FULL_64": (1, 65, 129, 150, 577, 100, 300),
            "FULL_128": (130, 191), "FULL_96": (65, 129, 100), "CAUSAL_64": (130, 200), "CAUSAL_AUTO": (129,)}
    out = []
    for c in all_cases():
        if c.table == "CAUSAL_GROUPS":
            ok = c.B == 3 or c.H == 14
        elif c.table == "CAUSAL_GRID":
            ok = c.B in (4, 6)
        elif c.table == "CAUSAL_NK_SHORT":
            ok = c.nk == 129
        else:
            ok = c.nq in keep[c.table]
        if ok:
            out.append(c)
    return out


def variants_of(c):
    """The vl2_attn_fwd variants that serve a case: 1 = attn_fwd_kernel<D, .>, 2 = attn_fwd_kernel<128, true, 2>, 3 = attn2_fwd_kernel on one
    stream with the plain tiling, 4 = two streams (and the class-token peel at the class-token shapes), 0 = the automatic choice: the one-stream
    peel with its (H, B, qb) grid, 4 or 3 by nqb * H <= 352, the D = 96 route."""
    if c.D == 96:
        return (0, 1)
    if c.table == "CAUSAL_AUTO":
        return (0,)
    if c.D == 64 and c.causal:
        return (1, 3, 4)
    return (0, 1, 2, 3, 4) if c.D == 128 and c.causal else (0, 1, 3, 4)


def instance(c, variant):
    """The kernel instance vl2_attn_fwd launches for a case under a variant: the launcher's plan (csrc/vl2_abi.hip) restated.  The tables must
    reach all 16 (tests/test_attn_fwd_edges_emu.py); the source lines this restates are pinned there."""
    form = f"{c.D}{'c' if c.causal else 'f'}"
    cls = is_cls_shape(c)
    if variant == 0 and c.D == 128 and c.causal and (c.nq + 127) // 128 * c.H <= 352:
        variant = 4
    elif variant == 0 and c.D in (64, 128):
        return f"attn2<{form}{',CLS' if cls else ''},NS1>"
    if variant == 4:
        return f"attn2<{form}{',CLS' if cls else ''},NS2>"
    if variant == 3:
        return f"attn2<{form},NS1>"
    return f"attn<{form}{',NG2' if variant == 2 and c.D == 128 and c.causal else ''}>"


def scale_of(c):
    return c.used ** -0.5


@functools.lru_cache(maxsize=None)
def rounds_of(c):
    """Launches of a case, each shifting every row's walk through its selector list by one step: the smallest number after which, in EVERY
    request, every kind that is in some row's list has been launched (`launched`) -- one round where rows x heads cover the lists, more at
    the short cases -- and, at the class-token shapes and the one-row cases, row 0 has run its whole list in every request."""
    _, _, order, n = row_lists(c)
    want = set(order[torch.arange(len(KINDS))[None, :] < n[:, None]].tolist())
    row0 = set(order[0, :n[0]].tolist()) if is_cls_shape(c) or c.nq == 1 else set()
    ran = [set() for _ in range(c.B)]
    ran0 = [set() for _ in range(c.B)]
    for rnd in range(64):
        p = picks(c, rnd)
        for b in range(c.B):
            ran[b] |= set(p[b].unique().tolist())
            ran0[b] |= set(p[b, :, 0].tolist())
        if all(r == want for r in ran) and all(row0 <= r for r in ran0):
            return rnd + 1
    raise AssertionError(f"{c.name}: the walk does not reach every selector in 64 rounds")


def launched(c):
    """[set of kinds launched in request b over all rounds of the case]."""
    out = [set() for _ in range(c.B)]
    for rnd in range(rounds_of(c)):
        p = picks(c, rnd)
        for b in range(c.B):
            out[b] |= set(p[b].unique().tolist())
    return out


# ---------------------------------------------------------------------------------------------------------------- selectors
def last_visible(c):
    """int64 [nq]: the last visible key of every query row."""
    r = torch.arange(c.nq)
    return torch.clamp(r + c.off, max=c.nk - 1) if c.causal else torch.full((c.nq,), c.nk - 1, dtype=torch.int64)


def _single(j, ndig):
    """masks [n, ndig] that select the one key j [n] (j clamped into the digits' range; the caller decides whether j is visible)."""
    j = j.clamp(0, 32 ** ndig - 1)
    return torch.stack([torch.ones_like(j) << ((j >> (5 * i)) & 31) for i in range(ndig)], 1)


def _low(j, ndig, d1=None, d0=None):
    """masks of key (j mod 1024) with digits 2.. = 0; d0 / d1: another mask for digit 0 / 1."""
    m = _single(j % 1024, ndig)
    if d1 is not None and ndig >= 2:
        m[:, 1] = d1
    if d0 is not None:
        m[:, 0] = d0
    return m


def _spaced(last, d0, step, phase, ndig):
    """(masks, wanted) of the keys d0 + 32 (phase + step k), k = 0, 1, .. below 1024: of those a row sees, the LAST 2^m (the largest power of
    two there is) -- the set ends at the row's last tiles and its count is a power of two by construction."""
    top = (last - d0) // 32                                                      # digit 1 of the last visible member of d0 + 32 v
    n = torch.where((last >= d0) & (top >= phase), (torch.clamp(top, max=31) - phase) // step + 1, 0)
    m = torch.ones_like(n)
    for _ in range(5):
        m = torch.where(2 * m <= n, 2 * m, m)
    mask = torch.zeros_like(n)
    for k in range(32 // step):
        mask |= ((k >= n - m) & (k < n)).long() << (phase + step * k)
    return _low(d0, ndig, d1=mask), n >= 1


KINDS = (
    "key0", "last", "last-1", "tile_first", "prev_tile_last", "key31", "key32", "key63", "key64",      # single keys
    "trap",                                                                                              # last and last + 1
    "block_last", "block_prev", "block0",                                                                # 32 consecutive keys: cut by the diagonal / nk; whole; keys 0 .. 31
    "apart32", "apart32_next",                                                                           # 32 apart: two keys in every tile, both streams and groups
    "apart64",                                                                                           # 64 apart: one key in every tile
    "even_tiles", "even_tiles_hi", "odd_tiles", "odd_tiles_hi",                                          # 128 apart: every selected key in ONE stream / group
    "apart1024",                                                                                         # D = 128: digit 2 free
)


def kind_masks(c):
    """{kind: (masks int64 [nq, ndig], wanted bool [nq])} for every row of a case; `wanted` = the kind applies (its defining key is visible)."""
    last, nd = last_visible(c), c.ndig
    yes = torch.ones(c.nq, dtype=torch.bool)
    const = lambda j: torch.full((c.nq,), j, dtype=torch.int64)
    T = last // 64 * 64
    out = {}
    for name, j in (("key0", const(0)), ("last", last), ("last-1", last - 1), ("tile_first", T), ("prev_tile_last", T - 1),
                    ("key31", const(31)), ("key32", const(32)), ("key63", const(63)), ("key64", const(64))):
        out[name] = (_single(j, nd), (j >= 0) & (j <= last))
    trap = _single(last, nd)
    trap[:, 0] |= torch.ones_like(last) << ((last + 1) & 31)
    if nd >= 2:                                                 # digit 0 = 31: last + 1 is the next block's first key (the tables stay below key 1023)
        trap[:, 1] |= torch.where((last & 31) == 31, torch.ones_like(last) << (((last >> 5) + 1) & 31), 0)
    out["trap"] = (trap, yes)
    blk = _single(last, nd)
    blk[:, 0] = ALL
    out["block_last"] = (blk, yes)
    blk = _single(last - 32, nd)
    blk[:, 0] = ALL
    out["block_prev"] = (blk, last >= 32)
    blk = _single(const(0), nd)
    blk[:, 0] = ALL
    out["block0"] = (blk, yes)
    d0 = last & 31
    out["apart32"] = _spaced(last, d0, 1, 0, nd)
    out["apart32_next"] = _spaced(last, (last + 1) & 31, 1, 0, nd)      # ends at key last + 1 - 32: the step after it is the hidden key last + 1
    out["apart64"] = _spaced(last, d0, 2, 0, nd)
    out["even_tiles"] = _spaced(last, d0, 4, 0, nd)
    out["even_tiles_hi"] = _spaced(last, d0, 4, 1, nd)
    out["odd_tiles"] = _spaced(last, d0, 4, 2, nd)
    out["odd_tiles_hi"] = _spaced(last, d0, 4, 3, nd)
    if nd >= 3:
        far = _single(last % 1024, nd)
        far[:, 2] = ALL
        out["apart1024"] = (far, yes)
    else:
        out["apart1024"] = (_single(last, nd), ~yes)
    return out


def matches(masks, nkeys, ndig):
    """bool [.., nkeys]: the keys 0 .. nkeys - 1 that masks [.., ndig] select."""
    keys = torch.arange(nkeys)
    ok = torch.ones(masks.shape[:-1] + (nkeys,), dtype=torch.bool)
    for i in range(ndig):
        ok &= ((masks[..., i, None] >> ((keys >> (5 * i)) & 31)) & 1).bool()
    for i in range(ndig, 4):
        ok &= ((keys >> (5 * i)) & 31) == 0
    return ok


@functools.lru_cache(maxsize=4)
def row_lists(c):
    """(masks [nq, K, ndig], count [nq, K], order [nq, K], n [nq]): every kind's masks and visible count per row; a kind is IN a row's list
    iff it applies and its visible count is a power of two (by construction for most; the cut blocks and the spaced sets where the cut
    leaves one); order[r, :n[r]] = the row's list as indices into KINDS."""
    km = kind_masks(c)
    masks = torch.stack([km[k][0] for k in KINDS], 1)
    wanted = torch.stack([km[k][1] for k in KINDS], 1)
    last = last_visible(c)
    vis = torch.arange(c.nk)[None, :] <= last[:, None]
    count = (matches(masks, c.nk, c.ndig) & vis[:, None, :]).sum(-1)
    valid = wanted & (count >= 1) & ((count & (count - 1)) == 0)
    order = torch.argsort((~valid).to(torch.int8), dim=1, stable=True)
    return masks, count, order, valid.sum(1)


def picks(c, rnd=0):
    """int64 [B, H, nq]: the kind every (request, head, row) runs.  The walking heads of a row (all H in full attention; in the causal cases
    head (row + round) % H runs THE TRAP, so that every causal row has it in one head of every launch, and the other H - 1 walk) take
    CONSECUTIVE entries of the row's list, starting where the row before stopped: entry ((row + round) * walkers + j + 7 * request) % n.  A
    swapped row, head or request is then another answer, rows x heads of ONE request reach every entry of a list of n <= nq * walkers entries
    in one launch, and row 0 reaches its whole list over ceil(n / walkers) rounds (`rounds_of` counts what is needed)."""
    _, _, order, n = row_lists(c)
    b, h, r = torch.arange(c.B)[:, None, None], torch.arange(c.H)[None, :, None], torch.arange(c.nq)[None, None, :]
    if not c.causal:
        idx = ((r + rnd) * c.H + h + 7 * b) % n[None, None, :]
        return order[r.expand_as(idx), idx]
    t = (r + rnd) % c.H
    j = (h - t - 1) % c.H                                                             # 0 .. H - 2 on the heads that walk the list
    idx = ((r + rnd) * (c.H - 1) + j + 7 * b) % n[None, None, :]
    return torch.where(h == t, KINDS.index("trap"), order[r.expand_as(idx), idx])


# ---------------------------------------------------------------------------------------------------------------- inputs
_WORLD = None


def world():
    global _WORLD
    if _WORLD is None:
        _WORLD = World(nkv=8, n=1543, seed=18)
    return _WORLD


def _salts(B, n, group=1):
    return torch.tensor([[salt(b, h // group) for h in range(n)] for b in range(B)])


def k_rows(c):
    """K fp32 [B, nkv, nk, D] of zeros and ones."""
    keys = torch.arange(c.nk)
    K = torch.zeros((c.B, c.nkv, c.nk, c.D))
    s = _salts(c.B, c.nkv)[:, :, None]
    for i in range(c.ndig):
        K.scatter_(3, (32 * i + (((keys >> (5 * i)) & 31)[None, None, :] + s) % 32)[..., None], 1.0)
    return K


def v_rows(c):
    """V fp32 [B, nkv, nk, D]: the world's rows (request b rolled by 131 b keys), dims from `used` on zero."""
    V = torch.zeros((c.B, c.nkv, c.nk, c.D))
    for b in range(c.B):
        V[b, :, :, :c.used] = world().v_rows(c.nkv, b, torch.arange(c.nk))[..., :c.used]
    return V


def q_rows(c, sel):
    """q fp32 [B, H, nq, D] of the masks sel [B, H, nq, ndig]: 0 at the wanted digit values (rotated by the kv head's salt), -2048 elsewhere
    below `used`, 0 from `used` on."""
    want = ((sel[..., None] >> torch.arange(32)) & 1).bool()                        # [B, H, nq, ndig, 32] by digit value
    s = _salts(c.B, c.H, c.H // c.nkv)[:, :, None, None, None]
    src = ((torch.arange(32) - s) % 32).expand(want.shape)                          # position p holds value (p - salt) % 32
    q = torch.zeros((c.B, c.H, c.nq, c.D))
    q[..., :c.used] = NEG
    q[..., :32 * c.ndig] = torch.where(torch.gather(want, 4, src), 0.0, NEG).flatten(3)
    return q


def softmax_reference(q, K, V, vis, scale):
    """Plain softmax attention in fp64: q [H, nq, D], K / V [H, nk, D] (the kv head of every q head), vis bool [nq, nk] -> [H, nq, D]."""
    s = (q @ K.transpose(1, 2)) * scale
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
    return p @ V


def guard(q, K, V, vis, scale, what=""):
    """THE GUARD in fp64 for every (head, row) of one request: q [H, nq, D], K / V [H, nk, D], vis [nq, nk].  -> selected keys [H, nq]."""
    assert bool(((V / V_QUANTUM) == (V / V_QUANTUM).round()).all()), f"{what}: V is not a multiple of the quantum"
    s = (q @ K.transpose(1, 2)) * (scale * LOG2E)
    top = s.masked_fill(~vis, float("-inf")).amax(-1)
    where = lambda bad: "head %d row %d" % tuple(torch.nonzero(bad)[0].tolist())
    assert bool((top == 0.0).all()), f"{what} {where(top != 0.0)}: the maximum score is not 0"
    hit = (s == 0.0) & vis
    rest = s.masked_fill(hit | ~vis, float("-inf")).amax(-1)
    assert bool((rest <= GAP).all()), f"{what} {where(rest > GAP)}: a non-selected key scores {float(rest.max())} > {GAP}"
    cnt = hit.sum(-1)
    assert bool(((cnt & (cnt - 1)) == 0).all()), f"{what} {where((cnt & (cnt - 1)) != 0)}: the number of selected keys is not a power of two"
    mag = (hit.double() @ V.abs()).amax(-1) / V_QUANTUM
    assert bool((mag < 2.0 ** 24).all()), f"{what} {where(mag >= 2.0 ** 24)}: sum |V| / quantum >= 2^24"
    return cnt


class Inputs:
    """One round of one case on the CPU: q, K, V (fp32, exact), the guard asserted for every row, the fp64 reference [B, H, nq, D]."""

    def __init__(self, c, rnd=0):
        self.c, self.rnd = c, rnd
        masks, _, _, _ = row_lists(c)
        self.kind = picks(c, rnd)
        r = torch.arange(c.nq)[None, None, :].expand_as(self.kind)
        self.q, self.K, self.V = q_rows(c, masks[r, self.kind]), k_rows(c), v_rows(c)
        self.vis = torch.arange(c.nk)[None, :] <= last_visible(c)[:, None]
        g, sc = c.H // c.nkv, scale_of(c)
        ref, cnt = [], []
        for b in range(c.B):
            q64 = self.q[b].double()
            K64, V64 = (t[b].double().repeat_interleave(g, 0) for t in (self.K, self.V))
            cnt.append(guard(q64, K64, V64, self.vis, sc, f"{c.name} round {rnd} request {b}"))
            ref.append(softmax_reference(q64, K64, V64, self.vis, sc))
        self.ref, self.count = torch.stack(ref), torch.stack(cnt)

    def operands(self, elem):
        out = []
        for t in (self.q, self.K, self.V):
            e = t.to(elem)
            assert torch.equal(e.float(), t), "an operand is not exact in the element type"
            out.append(e)
        return out


@functools.lru_cache(maxsize=2)
def inputs(c, rnd=0):
    return Inputs(c, rnd)


# ---------------------------------------------------------------------------------------------------------------- layouts, poison, the launch
def _strided(st, shape, strides, off):
    return torch.as_strided(st.view(-1), shape, strides, off)


def cap_of(c):
    return (c.nk + 63) // 64 * 64 + 128


class Operands:
    """The device operands of one case in its layout, poisoned: storages, element offsets of (request 0, head 0, row 0) and strides."""

    def __init__(self, c, q, K, V, elem, dev):
        B, H, nkv, D, nq, nk = c.B, c.H, c.nkv, c.D, c.nq, c.nk
        cap = cap_of(c)
        if c.layout == "fused":
            assert nq == nk and nkv == H
            W = 3 * H * D + c.rpad
            st = torch.full((B + 2, cap, W), NAN, dtype=elem)
            self.q_str = self.k_str = self.v_str = (cap * W, D, W)
            self.off = [cap * W, cap * W + H * D, cap * W + 2 * H * D]
            self.st = [st, st, st]
        else:
            Wq = H * D + (8 if c.layout == "batch" else 0)
            Wk = D + c.rpad
            self.st = [torch.full((B + 2, nq + 3, Wq), NAN, dtype=elem), torch.full((B + 2, nkv, cap, Wk), NAN, dtype=elem),
                       torch.full((B + 2, nkv, cap, Wk), NAN, dtype=elem)]
            self.q_str, self.k_str = ((nq + 3) * Wq, D, Wq), (nkv * cap * Wk, cap * Wk, Wk)
            self.v_str = self.k_str
            self.off = [(nq + 3) * Wq, nkv * cap * Wk, nkv * cap * Wk]
        for st, off, strd, t, n in zip(self.st, self.off, (self.q_str, self.k_str, self.v_str), (q, K, V), (nq, nk, nk)):
            _strided(st, t.shape, strd + (1,), off).copy_(t)
        if c.layout == "decoder":                                  # one request: the batch strides are 0, as the decoders pass them
            assert B == 1
            self.q_str, self.k_str, self.v_str = ((0,) + s[1:] for s in (self.q_str, self.k_str, self.v_str))
        Wo = H * D + 8
        self.o_str, self.o_off = ((nq + 2) * Wo, D, Wo), Wo
        self.o_host = torch.full((B, nq + 2, Wo), SENTINEL, dtype=elem)
        uniq = [self.st[0]] if c.layout == "fused" else self.st
        self.pristine = [s.to(dev) for s in uniq]
        self.dev_st = [s.clone() for s in self.pristine]
        self.dev = [self.dev_st[0 if c.layout == "fused" else i].view(-1)[self.off[i]:] for i in range(3)]

    def intact(self):
        return all(torch.equal(bits(a), bits(b)) for a, b in zip(self.dev_st, self.pristine))


def launch(ops, c, opnd, variant, dev):
    """One vl2_attn_fwd call of a case under `variant` -> the output storage [B, nq + 2, H D + 8] on the CPU."""
    o_st = opnd.o_host.to(dev)
    ops.set_attn_kv_groups(variant)
    try:
        ops.attn_fwd(opnd.dev[0], opnd.dev[1], opnd.dev[2], o_st.view(-1)[opnd.o_off:], opnd.q_str, opnd.k_str, opnd.v_str, opnd.o_str,
                     c.B, c.H, c.nq, c.nk, c.H // c.nkv, scale_of(c), c.causal, c.off, c.D)
    finally:
        ops.set_attn_kv_groups(0)
    return o_st.cpu()


def describe(c, variant, rnd, o, want):
    """The coordinates of the first wrong output: request, head, row, element, expected and received bits."""
    Wo = c.H * c.D + 8
    y, e = (_strided(t, (c.B, c.H, c.nq, c.D), ((c.nq + 2) * Wo, c.D, Wo, 1), Wo) for t in (o, want))
    bad = torch.nonzero(((y != e) | y.isnan()).any(-1))          # (a NaN differs from everything; -0.0 == 0.0: the fp64 mean of zeros is -1e-76)
    head = f"{c.name} variant {variant} round {rnd}"
    if not bad.numel():
        return f"{head}: the sentinel frame or the row padding of the output was written"
    b, h, r = bad[0].tolist()
    d = int(first_bad(y[b, h, r], e[b, h, r])[0])
    inp = inputs(c, rnd)
    return (f"{head}: {bad.shape[0]} of {c.B * c.H * c.nq} (request, head, row) differ, first request {b} head {h} row {r} (selector "
            f"{KINDS[int(inp.kind[b, h, r])]}, {int(inp.count[b, h, r])} keys): {first_diff(y[b, h, r], e[b, h, r], c.D)}; bits expected "
            f"{int(bits(e[b, h, r])[d]) & 0xFFFF:#06x}, got {int(bits(y[b, h, r])[d]) & 0xFFFF:#06x}")


def run_case(ops, c, elem, dev, variants=None, rounds=None):
    """Every round of a case under every variant that serves it -> [errors].  The expected output storage is the sentinel frame with the
    fp64 reference rounded once inside: one torch.equal checks the rows, the frame and the row padding."""
    errs = []
    Wo = c.H * c.D + 8
    for rnd in range(rounds_of(c)) if rounds is None else rounds:
        inp = inputs(c, rnd)
        opnd = Operands(c, *inp.operands(elem), elem, dev)
        want = opnd.o_host.clone()
        _strided(want, (c.B, c.H, c.nq, c.D), ((c.nq + 2) * Wo, c.D, Wo, 1), Wo).copy_(expected(inp.ref, elem))
        for v in variants_of(c) if variants is None else variants:
            o = launch(ops, c, opnd, v, dev)
            if not torch.equal(o, want):
                errs.append(describe(c, v, rnd, o, want))
            if not opnd.intact():
                errs.append(f"{c.name} variant {v} round {rnd}: q, k or v changed")
                for s, p in zip(opnd.dev_st, opnd.pristine):
                    s.copy_(p)
    return errs


# ---------------------------------------------------------------------------------------------------------------- the causal grid order
def causal_qb(x, nqb, G, NS, file=2, skip=True):
    """The query block of workgroup blockIdx.x = x of a causal launch, restated from the kernels: file 1 = k_attn.h (the first nfirst ranks the
    longest blocks descending, then ascending), file 2 = k_attn2.h with NS streams (plain longest-first when nqb * G exceeds what the chip
    holds, else k_attn.h's order, else -- one stream, nqb > nfirst -- the n2 blocks that get a partner first)."""
    r = x // G
    nfirst = min((256 + G - 1) // G, nqb)
    pair = nqb - 1 - r if r < nfirst else r - nfirst
    if file == 1:
        return pair
    qb = nqb - 1 - r if skip and nqb * G > (256 if NS == 2 else 512) else pair
    if skip and NS == 1 and nqb * G <= 512 and nqb > nfirst:
        n2 = nqb - nfirst
        alone = nfirst - n2
        qb = nqb - 1 - alone - r if r < n2 else nqb - 1 - (r - n2) if r < nfirst else r - nfirst
    return qb


def causal_order(nqb, G, NS):
    """Which of k_attn2.h's three orders a launch takes."""
    nfirst = min((256 + G - 1) // G, nqb)
    if NS == 1 and nqb * G <= 512 and nqb > nfirst:
        return "partnered_first"
    return "longest_first" if nqb * G > (256 if NS == 2 else 512) else "long_then_ascending"


# ---------------------------------------------------------------------------------------------------------------- graded weights
GRADED_MARGIN = 1.5     # the kernel's largest per-row rel-L2 over the rounding model's: see tests/test_gpu_attn_fwd_edges.py
GRADED = (      # one random-input case per kernel instance: (D, causal, B, H, nkv, N, used)
    (128, True, 1, 8, 2, 330, 128),     # causal S = 330, group 4: variants 1, 2, 3, 4
    (64, False, 2, 2, 2, 193, 64),      # class-token shape with a dead wave: variants 0 (peel, one stream), 1, 3, 4 (peel, two streams)
    (64, False, 2, 2, 2, 150, 64),      # plain D = 64: variants 1, 3, 4
    (128, False, 1, 2, 2, 130, 128),    # variants 1, 3, 4
    (96, False, 2, 2, 2, 129, 72),      # variant 1
    (64, True, 1, 2, 1, 200, 64),       # D = 64 causal: variants 1, 3, 4
)


def graded_case(D, causal, B, H, nkv, N, used):
    return _case("GRADED", D, causal, N, B=B, H=H, nkv=nkv, used=used, rpad=8)


def graded_inputs(c, elem, seed=0):
    """Random q, K, V (weights of every size) in the element type, dims from `used` on zero -> (q, K, V) as Inputs.operands gives them."""
    g = torch.Generator().manual_seed(1000 * c.D + c.nq + seed)
    mk = lambda *s: torch.randn(*s, generator=g)
    q, K, V = mk(c.B, c.H, c.nq, c.D) * 1.5, mk(c.B, c.nkv, c.nk, c.D), mk(c.B, c.nkv, c.nk, c.D)
    for t in (q, K, V):
        t[..., c.used:] = 0
    return q.to(elem), K.to(elem), V.to(elem)


def row_rel(y, ref):
    """rel-L2 per (request, head, row) over the `used` dims: [B, H, nq]."""
    return ((y.double() - ref).norm(dim=-1) / ref.norm(dim=-1))


def graded_reference(c, q, K, V, elem):
    """(fp64 softmax [B, H, nq, D], the rounding model's output in `elem`): the model is the reference's arithmetic at the kernel's precision
    -- fp32 scores and softmax weights, P rounded to the element type before it meets V, the denominator from the unrounded weights, the
    result rounded once -- computed from the reference's inputs alone."""
    g, sc = c.H // c.nkv, scale_of(c)
    vis = torch.arange(c.nk)[None, :] <= last_visible(c)[:, None]
    Kh, Vh = K.repeat_interleave(g, 1), V.repeat_interleave(g, 1)
    ref = torch.stack([softmax_reference(q[b].double(), Kh[b].double(), Vh[b].double(), vis, sc) for b in range(c.B)])
    s = (q.float() @ Kh.float().transpose(2, 3)) * torch.tensor(sc, dtype=torch.float32)
    s = s.masked_fill(~vis, float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    model = ((p.to(elem).float() @ Vh.float()) / p.sum(-1, keepdim=True)).to(elem)
    return ref, model
