"""The paged KV cache in fp8 on MI355X (include/vl2hip.h vl2_attn_decode_kv8_paged / vl2_kv_page_quant, csrc/k_attn_paged_kv8.h, DESIGN.md
section 21).  Paging moves codes and scales and changes no sum, so EVERY comparison here is torch.equal (on the storage bits where NaN poison
is involved): there is no tolerance in this file.  Kernels at nkv = 2, 256 positions (4 pages per sequence), both builds: the page quantiser
writes what vl2_kv_quant writes (and what tests/fp8kv_oracle.py defines) and touches nothing else; the attention equals
vl2_attn_decode_kv8_batched on contiguous copies of the same codes and scales in `out`, in the live slices of `partial` and in the appended
rows, and selects the right keys on the exact inputs of tests/attn_exact.py; a request without a page or past the table writes nothing; a
replayed graph crosses a page boundary like the eager contiguous steps.  Decoder and serving on the small golden config: generate_batch, the
continuous batcher and ModelBatcher on fp8 pages give the tokens and logits of the contiguous fp8-KV slots."""
import gc

import pytest
import torch

from oracle import vl2_oracle as O
from tests import attn_exact as AX
from tests import fp8kv_oracle as KV

pytestmark = pytest.mark.gpu
DEV = "cuda"
NKV, HD, SMAX = 2, 128, 256
PPS = SMAX // 64                                  # pages per sequence
SCALE = HD ** -0.5
POSITIONS = (0, 15, 63, 64, 65, 200)
CODE_K, CODE_V = 0xAB, 0xCD                       # the code pools' bytes before a page quantisation
SCALE_K, SCALE_V = 0x5A5B5C5D, 0x5A5B5C5E         # the scale pools' bit patterns before it (finite floats, no power of two)
POISON_CODE = 0x7F                                # e4m3fn NaN; with a NaN scale: whoever reads such a row has NaN in its output


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib, ops as o
    _lib.load()
    return o


@pytest.fixture(params=["bf16", "fp16"])
def elem(request, ops):
    """Both builds: libvl2hip.so (bf16 elements) and libvl2hip_f16.so."""
    from videollama2_amd import _lib
    _lib.set_elem(request.param)
    try:
        yield torch.bfloat16 if request.param == "bf16" else torch.float16
    finally:
        _lib.set_elem("bf16")


def bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def all_same_bits(xs, ys):
    return len(xs) == len(ys) and all(same_bits(x, y) for x, y in zip(xs, ys))


def _tables(rows=SMAX):
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.int64).float() / HD))
    fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().contiguous().to(DEV), fr.sin().contiguous().to(DEV)


def deal_pages(needs, n_pages, seed, pps=PPS):
    """Page ids 1 .. n_pages - 1 shuffled and dealt to the requests (needs[b] pages each): non-monotone rows, interleaved across requests.
    -> (table rows as lists of pps entries, -1 behind a request's pages; the ids nobody got)."""
    perm = (torch.randperm(n_pages - 1, generator=torch.Generator().manual_seed(seed)) + 1).tolist()
    rows = []
    for n in needs:
        rows.append(perm[:n] + [-1] * (pps - n))
        perm = perm[n:]
    return rows, perm


def interleaved(rows):
    """Two requests' pages interleave: some page of one lies between two pages of another."""
    own = [[p for p in r if p >= 0] for r in rows]
    return any(min(a) < p < max(a) for i, a in enumerate(own) for j, b in enumerate(own) if i != j and a for p in b)


def paginate(kv8, rows, n_pages):
    """The four pools that hold the contiguous fp8 caches kv8 = (k8, v8, ks, vs) (codes [B, nkv, S, 128], scales [B, nkv, S]) under the table
    `rows`; poison (code 0x7F, NaN scale) in every page nobody owns, page 0 included."""
    pools = []
    for t in kv8:
        codes = t.dim() == 4
        pool = torch.full((n_pages, t.shape[1], 64) + ((HD,) if codes else ()), POISON_CODE if codes else float("nan"), dtype=t.dtype, device=t.device)
        for b, row in enumerate(rows):
            for j, page in enumerate(row):
                if 0 <= page < n_pages:
                    pool[page] = t[b, :, 64 * j:64 * j + 64]
        pools.append(pool)
    return tuple(pools)


def _qkv(nh, seed, elem, rows):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((rows, (nh + 2 * NKV) * HD), generator=g) * 1.5).to(elem).to(DEV)


def _random_rows(g, elem, *lead):
    """[*lead, NKV, SMAX, 128] with row magnitudes spread over 2^-8 .. 2^8, so that the rows' scales differ."""
    x = torch.randn(*lead, NKV, SMAX, HD, generator=g) * torch.exp2(torch.randint(-8, 9, (*lead, NKV, SMAX, 1), generator=g).float())
    return x.to(elem)


def _caches8(positions, elem, seed):
    """Contiguous fp8 caches (k8, v8, ks, vs) [B, NKV, SMAX, ..] on the device: below each request's position the definition's quantisation
    of random 16-bit rows, poison from it on."""
    g = torch.Generator().manual_seed(seed)
    B = len(positions)
    out = []
    for _ in range(2):
        q, s = KV.quant_cache_rows(_random_rows(g, elem, B).view(B * NKV, SMAX, HD))
        q, s = q.view(B, NKV, SMAX, HD).clone(), s.view(B, NKV, SMAX).clone()
        for b, p in enumerate(positions):
            q[b, :, p:] = POISON_CODE
            s[b, :, p:] = float("nan")
        out.append((q, s))
    return tuple(t.to(DEV) for t in (out[0][0], out[1][0], out[0][1], out[1][1]))


def _nan_partial(B, nh, nsplit=PPS):
    return torch.full((B * nh * nsplit * 130,), float("nan"), dtype=torch.float32, device=DEV)


def _out(B, nh, elem):
    return torch.zeros((B, nh * HD), dtype=elem, device=DEV)


def clone_all(ts):
    return tuple(t.clone() for t in ts)


# ---------------------------------------------------------------------------------------------------------------- 1. the page quantiser
def _sentinel_pools(n_pages):
    k8 = torch.full((n_pages, NKV, 64, HD), CODE_K, dtype=torch.uint8, device=DEV)
    v8 = torch.full((n_pages, NKV, 64, HD), CODE_V, dtype=torch.uint8, device=DEV)
    ks = torch.full((n_pages, NKV, 64), SCALE_K, dtype=torch.int32, device=DEV).view(torch.float32)
    vs = torch.full((n_pages, NKV, 64), SCALE_V, dtype=torch.int32, device=DEV).view(torch.float32)
    return k8, v8, ks, vs


@pytest.mark.parametrize("p0,p1", [(0, 1), (0, 64), (63, 66), (0, 200)])
def test_page_quant_writes_what_kv_quant_writes_and_nothing_else(ops, elem, p0, p1):
    """(0, 1): the workgroup with dead rows (4 live rows of 16).  (63, 66) crosses a page edge."""
    n_pages = 12
    g = torch.Generator().manual_seed(100 + p1)
    k16, v16 = _random_rows(g, elem), _random_rows(g, elem)
    k16[0, p0], v16[1, p1 - 1] = 0, 0                          # an all-zero row: scale 1
    # the contiguous fp8 cache vl2_kv_quant fills at those rows, and the definition's quantisation of them
    cont = (torch.full((NKV, SMAX, HD), CODE_K, dtype=torch.uint8, device=DEV), torch.full((NKV, SMAX, HD), CODE_V, dtype=torch.uint8, device=DEV),
            torch.full((NKV, SMAX), -7.0, dtype=torch.float32, device=DEV), torch.full((NKV, SMAX), -9.0, dtype=torch.float32, device=DEV))
    ops.kv_quant(k16.to(DEV), v16.to(DEV), cont, p0, p1)
    (qk, sk), (qv, sv) = KV.quant_cache_rows(k16[:, p0:p1]), KV.quant_cache_rows(v16[:, p0:p1])
    for got, want in zip(cont, (qk, qv, sk, sv)):
        assert torch.equal(got[:, p0:p1].cpu(), want)
    assert sk[0, 0].item() == 1.0 and sv[1, -1].item() == 1.0
    k16, v16 = k16.to(DEV), v16.to(DEV)
    mine, other = [7, 2, 9, 4], [3, 8, 1, 6]                  # non-monotone, interleaved with another request's pages
    assert interleaved([mine, other]) and any(mine[j] > mine[j + 1] for j in range(PPS - 1))
    for row in (mine, [7, -1, 9, 4], [7, n_pages, 9, n_pages + 5], [-1, -1, -1, -1]):
        pools = _sentinel_pools(n_pages)
        exp = clone_all(pools)
        p = torch.arange(p0, p1)
        page = torch.tensor(row)[p // 64]
        has = (page >= 0) & (page < n_pages)
        for e, c in zip(exp, cont):
            e[page[has].to(DEV), :, (p % 64)[has].to(DEV)] = c[:, p[has].to(DEV)].transpose(0, 1)
        table = torch.tensor([other, row], dtype=torch.int32, device=DEV)
        ops.kv_page_quant(k16, v16, pools, table[1], p0, p1)
        torch.cuda.synchronize()
        # the rows read back through the table are vl2_kv_quant's codes and scales; every other byte of the four pools keeps its sentinel (the
        # other request's pages, the pages nobody owns, the rows of this request's pages outside [p0, p1), a row without a page)
        assert all_same_bits(pools, exp), row
        if row is mine:
            for pool, c, want in zip(pools, cont, (qk, qv, sk, sv)):
                back = torch.cat([pool[pg] for pg in row], 1)[:, p0:p1]
                assert same_bits(back, c[:, p0:p1]) and torch.equal(back.cpu(), want)
            untouched = torch.ones(n_pages, dtype=torch.bool, device=DEV)
            untouched[row] = False
            for pool, s in zip(pools, (CODE_K, CODE_V, SCALE_K, SCALE_V)):
                assert bool((bits(pool)[untouched] == s).all())


# ---------------------------------------------------------------------------------------------------------------- 2. the operator
class Case:
    """B = 6 requests at POSITIONS in one launch, computed once per (group, element type): random contiguous fp8 caches with poison from `pos`
    on, their pages shuffled across the requests with poison in every page nobody owns, and vl2_attn_decode_kv8_batched's results on the
    contiguous copies -- `out`, `partial` (NaN outside the slices it wrote) and the caches after the append."""

    def __init__(self, ops, group, elem, positions=POSITIONS, seed=0):
        self.nh, self.elem, self.positions = NKV * group, elem, positions
        B = self.B = len(positions)
        self.cos, self.sin = _tables()
        self.qkv = _qkv(self.nh, 10 * group + seed, elem, B)
        self.c0 = _caches8(positions, elem, 20 * group + seed)
        needs = [p // 64 + 1 for p in positions]
        self.n_pages = 1 + sum(needs) + 3
        self.rows, self.spare = deal_pages(needs, self.n_pages, 30 * group + seed)
        self.pos = torch.tensor(positions, dtype=torch.int32, device=DEV)
        self.c1 = clone_all(self.c0)
        self.partial = _nan_partial(B, self.nh)
        self.out = _out(B, self.nh, elem)
        ops.attn_decode_kv8_batched(self.qkv, self.c1, self.cos, self.sin, self.partial, self.out, self.nh, NKV, self.pos, SMAX, SCALE)
        torch.cuda.synchronize()
        assert not bool(self.out.isnan().any())

    def table(self, rows=None):
        return torch.tensor(self.rows if rows is None else rows, dtype=torch.int32, device=DEV)

    def pools(self, rows=None):
        return paginate(self.c0, self.rows if rows is None else rows, self.n_pages)


_CASES = {}


def case(ops, group, elem):
    key = (group, elem)
    if key not in _CASES:
        _CASES[key] = Case(ops, group, elem)
    return _CASES[key]


@pytest.mark.parametrize("group", [4, 7], ids=["group4_mistral", "group7_qwen2"])
def test_paged_attention_equals_the_contiguous_fp8_call_bit_for_bit(ops, elem, group):
    c = case(ops, group, elem)
    pools = c.pools()
    # the pages really are shuffled: some request's row is not ascending, and two requests' pages interleave
    assert any(r[j] > r[j + 1] >= 0 for r in c.rows for j in range(PPS - 1)) and interleaved(c.rows)
    # the poison is where it should be: page 0, the spare pages, the rows at and past `pos` of owned pages
    for page in [0] + c.spare:
        assert bool((pools[0][page] == POISON_CODE).all()) and bool(pools[2][page].isnan().all()) and bool(pools[3][page].isnan().all())
    for b, pos in enumerate(c.positions):
        page = c.rows[b][pos // 64]
        assert bool((pools[1][page, :, pos % 64:] == POISON_CODE).all()) and bool(pools[3][page, :, pos % 64:].isnan().all())
    partial, out = _nan_partial(c.B, c.nh), _out(c.B, c.nh, elem)
    ops.attn_decode_kv8_paged(c.qkv, pools, c.table(), c.cos, c.sin, partial, out, c.nh, NKV, c.pos, SMAX, SCALE)
    torch.cuda.synchronize()
    assert torch.equal(out, c.out), int((out != c.out).sum())
    # partial [B][nh][4][130]: the live slices hold the contiguous call's bits, the others were not written (both still NaN)
    assert same_bits(partial, c.partial)
    p4, live = partial.view(c.B, c.nh, PPS, 130), 0
    for b, pos in enumerate(c.positions):
        n = pos // 64 + 1
        live += n
        assert not bool(p4[b, :, :n].isnan().any()) and bool(p4[b, :, n:].isnan().all()), b
    assert live == 11
    # the four pools after the step = the contiguous caches after theirs, page by page: the appended row's codes and scales byte for byte,
    # every other row (the poison past `pos`, the pages nobody owns, page 0) untouched
    assert all_same_bits(pools, paginate(c.c1, c.rows, c.n_pages))
    for b, pos in enumerate(c.positions):
        page = c.rows[b][pos // 64]
        for pool, cont in zip(pools, c.c1):
            assert same_bits(pool[page, :, pos % 64], cont[b, :, pos]), b
        assert not bool(pools[2][page, :, pos % 64].isnan().any()) and not bool(pools[3][page, :, pos % 64].isnan().any()), b
    # a smaller launch capacity (ctx_cap = the longest context): the same outputs and the same pools
    out2, pools2 = _out(c.B, c.nh, elem), c.pools()
    ops.attn_decode_kv8_paged(c.qkv, pools2, c.table(), c.cos, c.sin, _nan_partial(c.B, c.nh), out2, c.nh, NKV, c.pos, max(c.positions) + 1, SCALE)
    torch.cuda.synchronize()
    assert torch.equal(out2, c.out) and all_same_bits(pools2, pools)


# ---------------------------------------------------------------------------------------------------------------- 3. key-selecting inputs
@pytest.mark.parametrize("group", [4, 7], ids=["group4_mistral", "group7_qwen2"])
def test_a_wrong_page_would_select_a_wrong_key(ops, group):
    """tests/attn_exact.py's key-selecting inputs (every K row encodes its own position, every query selects a power-of-two set of keys, the
    fp64 softmax rounded once is THE answer) on the fp8 cache, which holds them exactly: the strided, poisoned batch of its batched kv8
    cases, its rows moved into shuffled pages.  bf16 elements, as the exact kv8 cases of tests/test_gpu_attn_edges.py."""
    elem = torch.bfloat16
    bt = AX.Batch(group, NKV, POSITIONS, elem, DEV, kv8=True)
    assert bt.smax % 64 == 0
    pps = bt.smax // 64
    needs = [p // 64 + 1 for p in POSITIONS]
    n_pages = 1 + sum(needs) + 2
    rows, _ = deal_pages(needs, n_pages, group, pps)
    assert any(r[j] > r[j + 1] >= 0 for r in rows for j in range(pps - 1)) and interleaved(rows)
    nh = bt.nh

    def launch(table_rows):
        pools = paginate(tuple(bt.cache), rows, n_pages)             # the rows live where `rows` says, whatever table the launch is given
        pst, partial = AX.partial_ws(bt.B * nh * pps * 130, DEV)
        out_st = torch.full((bt.B + 2, nh * HD + 8), AX.SENTINEL, dtype=elem, device=DEV)
        ops.attn_decode_kv8_paged(bt.qkv, pools, torch.tensor(table_rows, dtype=torch.int32, device=DEV), bt.cos, bt.sin, partial,
                                  out_st[1:bt.B + 1, :nh * HD], nh, NKV, bt.pos_dev, bt.smax, AX.SCALE)
        o = out_st.cpu()
        keep = torch.ones(o.shape, dtype=torch.bool)
        keep[1:bt.B + 1, :nh * HD] = False
        assert bool((o[keep] == AX.SENTINEL).all()) and AX.bands_intact(pst.cpu())          # the sentinel frames of out and of partial
        return o, pools

    o, pools = launch(rows)
    for b, r in enumerate(bt.reqs):
        exp = AX.expected(r.reference()[0], elem)
        y = o[b + 1, :nh * HD]
        assert torch.equal(y, exp), f"request {b} (pos {r.pos}): {AX.first_diff(y, exp)}"
        page = rows[b][r.pos // 64]
        row = [pool[page, :, r.pos % 64].cpu() for pool in pools]
        assert AX.new_row_error(r, row, elem, True, f"request {b}") is None
    # the same launch with the first pages of requests 4 and 5 swapped in the table: each reads 64 keys of the other, which never match
    wrong = [list(r) for r in rows]
    wrong[4][0], wrong[5][0] = rows[5][0], rows[4][0]
    o, _ = launch(wrong)
    for b in (4, 5):
        assert not torch.equal(o[b + 1, :nh * HD], AX.expected(bt.reqs[b].reference()[0], elem)), b
    for b in (0, 1, 2, 3):
        assert torch.equal(o[b + 1, :nh * HD], AX.expected(bt.reqs[b].reference()[0], elem)), b


# ---------------------------------------------------------------------------------------------------------------- 4. the guards
@pytest.mark.parametrize("how", ["page_unassigned", "page_outside_the_pool", "pos_at_seq_cap", "pos_past_seq_cap"])
def test_a_request_without_a_page_or_past_the_table_writes_nothing(ops, elem, how):
    """Request 4 (position 65, pages for slices 0 and 1) is broken in one way.  It must leave all four pools bit-unchanged, and the other
    requests' output rows and appended rows must equal a launch without it."""
    c = case(ops, 4, elem)
    victim, others = 4, [0, 1, 2, 3, 5]
    rows = [list(r) for r in c.rows]
    pos = c.pos.clone()
    if how == "page_unassigned":
        rows[victim][1] = -1
    elif how == "page_outside_the_pool":
        rows[victim][1] = c.n_pages + (0 if elem == torch.bfloat16 else 7)
    else:
        pos[victim] = SMAX + (0 if how == "pos_at_seq_cap" else 5)
    # the launch without it, on the unbroken table (its pools: the victim's pages hold its resident rows, nothing of it is appended)
    idx = torch.tensor(others, device=DEV)
    ref = c.pools()
    oref = _out(len(others), c.nh, elem)
    ops.attn_decode_kv8_paged(c.qkv[idx], ref, c.table()[idx], c.cos, c.sin, _nan_partial(len(others), c.nh), oref, c.nh, NKV, c.pos[idx], SMAX, SCALE)
    assert torch.equal(oref, c.out[idx])
    pools = c.pools()
    out = _out(c.B, c.nh, elem)
    ops.attn_decode_kv8_paged(c.qkv, pools, c.table(rows), c.cos, c.sin, _nan_partial(c.B, c.nh), out, c.nh, NKV, pos, SMAX, SCALE)
    torch.cuda.synchronize()
    assert torch.equal(out[idx], oref)
    assert all_same_bits(pools, ref)


# ---------------------------------------------------------------------------------------------------------------- 5. graph = eager
def test_replayed_graph_crosses_a_page_boundary_like_the_eager_contiguous_steps(ops, elem):
    nh, B, steps = NKV * 4, 2, 5
    pos0 = (62, 130)                                              # request 0 walks 62 .. 66: from its page 0 into its page 1
    cos, sin = _tables()
    qkvs = [_qkv(nh, 70 + s, elem, B) for s in range(steps)]
    start = _caches8(pos0, elem, 5)
    cont = clone_all(start)
    pos = torch.tensor(pos0, dtype=torch.int32, device=DEV)
    outs = torch.zeros(steps, B, nh * HD, dtype=elem, device=DEV)
    after, pc = [], _nan_partial(B, nh)
    for s in range(steps):                                        # eager, contiguous
        ops.attn_decode_kv8_batched(qkvs[s], cont, cos, sin, pc, outs[s], nh, NKV, pos, SMAX, SCALE)
        pos += 1
        after.append(clone_all(cont))
    rows = [[5, 2, -1, -1], [4, 6, 1, -1]]
    n_pages = 8
    pools = paginate(start, rows, n_pages)
    fresh = clone_all(pools)
    table = torch.tensor(rows, dtype=torch.int32, device=DEV)
    pos = torch.tensor(pos0, dtype=torch.int32, device=DEV)
    qbuf, obuf, pp = qkvs[0].clone(), _out(B, nh, elem), _nan_partial(B, nh)

    def step():
        ops.attn_decode_kv8_paged(qbuf, pools, table, cos, sin, pp, obuf, nh, NKV, pos, SMAX, SCALE)
        pos.add_(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                    # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for pool, f in zip(pools, fresh):                             # back to the start: all five steps are replays
        pool.copy_(f)
    pos.copy_(torch.tensor(pos0, dtype=torch.int32))
    for s in range(steps):
        qbuf.copy_(qkvs[s])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(obuf, outs[s]), s
        assert pos.tolist() == [p + s + 1 for p in pos0], s
        assert all_same_bits(pools, paginate(after[s], rows, n_pages)), s            # codes and scales, the appended row included
    assert not bool(pools[2][2, :, :3].isnan().any()) and bool(pools[2][2, :, 3:].isnan().all())      # rows 64 .. 66 landed in page 2
    assert bool((pools[0][2, :, 3:] == POISON_CODE).all())


# ---------------------------------------------------------------------------------------------------------------- 6. decoder
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


LENS = (70, 5, 129, 33, 64)                       # beside the golden prompt: ragged, below / at / above a page edge
N_NEW = 6


@pytest.fixture(scope="module")
def small(ops, golden_small):
    from videollama2_amd.decoder import HipMistralDecoder
    cfg = golden_small["cfg"]
    assert cfg["llm"]["head_dim"] == 128
    dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, golden_small["seed"], only=_keep), DEV, max_seq_len=256)
    g = torch.Generator().manual_seed(21)
    embeds = [golden_small["inputs_embeds"].to(DEV).bfloat16()] + [(torch.randn(n, dec.D, generator=g) * 0.5).bfloat16().to(DEV) for n in LENS]
    yield dec, embeds
    # a decoder that served a batcher is in a reference cycle with it: collect the pair (and its captured graphs) here
    dec._bb_busy = None
    del dec
    gc.collect()
    torch.cuda.empty_cache()


def _parked(dec, n):
    return [[0] + [-1] * (dec._bb["pages_per_seq"] - 1)] * n


@pytest.mark.parametrize("fmt", ["16bit", "fp8", "mxfp4"])
def test_generate_batch_on_fp8_pages_equals_the_contiguous_fp8_slots(small, fmt):
    from videollama2_amd.paging import pages_needed
    dec, embeds = small
    switch = {"16bit": None, "fp8": dec.enable_fp8_decode, "mxfp4": dec.enable_mxfp4_decode}[fmt]
    if switch:
        switch()
    try:
        # three lists: the multi-row GEMV step, the skinny-M step, and one whose requests land on the pages the first left dirty
        lists = {"a": embeds[:3], "b": embeds[3:] + embeds[:3], "c": embeds[3:5]}
        p16 = dec.prefill(embeds[0]).clone()
        dec.enable_fp8_kv()
        runs = {k: dec.generate_batch(v, max_new_tokens=N_NEW, return_logits=True) for k, v in lists.items()}
        gen = lambda: torch.Generator(device=DEV).manual_seed(7)
        sampled = dec.generate_batch(lists["a"], max_new_tokens=N_NEW, sampler=(0.8, 20, 0.9, gen()))
        dec.enable_fp8_kv(False)
        total = sum(pages_needed(e.shape[0], N_NEW, dec.max_seq_len) for e in embeds)
        dec.enable_paged_kv(total + 1, fp8=True)
        assert dec.paged_kv and dec.paged_kv_fp8 and dec.fp8_kv is False and dec.kv8 is None and dec.decode_format == fmt
        assert dec.kv_page_bytes() == dec.n_layers * 2 * dec.nkv * 64 * (128 + 4)
        pool = dec._ensure_batch(6)["pool"]
        for k in ("b", "a", "c", "a"):                             # the pool is not cleared on free: every run after the first lands on pages
            outs, logits = dec.generate_batch(lists[k], max_new_tokens=N_NEW, return_logits=True)        # that hold other requests' stale rows
            assert [o.tolist() for o in outs] == [o.tolist() for o in runs[k][0]], k
            assert torch.equal(logits, runs[k][1]), k
            assert pool is dec._bb["pool"], k                      # the same pools all along
            assert pool.n_free == total and dec._bb["table"].tolist() == _parked(dec, 6)
        assert any(bool(t.any()) for t in dec._bb["pools8"][0][:2])            # (stale codes are there)
        again = dec.generate_batch(lists["a"], max_new_tokens=N_NEW, sampler=(0.8, 20, 0.9, gen()))
        assert [o.tolist() for o in again] == [o.tolist() for o in sampled]
        eager = dec.generate_batch(lists["a"], max_new_tokens=N_NEW, return_logits=True, use_graph=False)
        assert torch.equal(eager[1], runs["a"][1])
        # memory: four pools of n_pages pages per layer, and nothing of another layout
        bb = dec._bb
        pool_bytes = sum(t.numel() * t.element_size() for ps in bb["pools8"] for t in ps)
        assert pool_bytes == (total + 1) * dec.kv_page_bytes() and len(bb["pools8"]) == dec.n_layers
        assert not any(k in bb for k in ("k", "v", "kv8", "kpool", "vpool"))
        # the single-sequence paths keep their 16-bit bits under fp8 pages
        assert torch.equal(dec.prefill(embeds[0]), p16)
        # off again: the contiguous 16-bit slots
        dec.enable_paged_kv(0, False)
        assert not dec.paged_kv_fp8
        dec.generate_batch(lists["c"], max_new_tokens=2)
        assert "k" in dec._bb and "pools8" not in dec._bb
    finally:
        dec.enable_paged_kv(0, False)
        dec.enable_fp8_kv(False)
        if switch:
            switch(False)


def _drain(b, owners=None, page_cap=None):
    """Step a batcher until it is empty -> (the request ids in the order they were admitted, the most requests in flight at once, the
    requests still queued after the first step).  owners: {page: [the requests that held it]}; page_cap: the pages in use never exceed it."""
    order, most, queued = [], 0, None
    while b.in_flight():
        b.step()
        queued = len(b.waiting) if queued is None else queued
        now = [r for r in b.slots if r is not None]
        assert page_cap is None or sum(r.need for r in now) <= page_cap
        for r in sorted(now, key=lambda r: r.rid):
            if r.rid not in order:
                order.append(r.rid)
                for pg in (r.pages if owners is not None else ()):
                    owners.setdefault(pg, []).append(r.rid)
        most = max(most, len(now))
    return order, most, queued


def test_continuous_batcher_on_a_pool_that_holds_two_reservations(small):
    """6 requests of mixed length through 4 slots and a pool of 5 fp8 pages: every reservation is 2 or 3 pages, so no three requests fit at
    once and three or more are queued behind the two in flight.  Admission order and every request's tokens equal the same batcher on
    contiguous fp8-KV slots, the pages of retired requests are reused dirty, and after run() every page is free again."""
    from videollama2_amd.serving import ContinuousBatcher
    dec, embeds = small
    g = torch.Generator().manual_seed(33)
    lens, n_new = (70, 129, 65, 100, 120, 64), (6, 3, 8, 5, 10, 4)
    reqs = [(torch.randn(n, dec.D, generator=g) * 0.5).bfloat16().to(DEV) for n in lens]
    try:
        dec.enable_fp8_kv()
        b = ContinuousBatcher(dec, max_slots=4, use_graph=True)
        rid = [b.submit(e, max_new_tokens=n) for e, n in zip(reqs, n_new)]
        order_ref, _, _ = _drain(b)
        want = [b.finished[r].tolist() for r in rid]
        rank_ref = [rid.index(r) for r in order_ref]                # admission order, as submission ranks
        assert rank_ref == list(range(6)) and [len(w) for w in want] == list(n_new)
        dec.enable_fp8_kv(False)
        dec.enable_paged_kv(6, fp8=True)
        for use_graph in (True, False):
            b = ContinuousBatcher(dec, max_slots=4, use_graph=use_graph)
            rid = [b.submit(e, max_new_tokens=n) for e, n in zip(reqs, n_new)]
            assert [r.need for r in b.waiting] == [2, 3, 2, 2, 3, 2]
            owners = {}
            order, most, queued = _drain(b, owners, page_cap=5)
            assert most == 2 and queued == 4                        # two reservations held, the other requests queued behind them
            assert [b.finished[r].tolist() for r in rid] == want, use_graph
            assert [rid.index(r) for r in order] == rank_ref
            assert 0 not in owners and max(len(o) for o in owners.values()) >= 2        # a freed (dirty) page served a later request
            bb = dec._bb
            assert bb["pool"].n_free == 5 and bb["table"].tolist() == _parked(dec, 4)
            dec._bb_busy = None
    finally:
        dec._bb_busy = None
        dec.enable_paged_kv(0, False)
        dec.enable_fp8_kv(False)


def test_model_level_switch_and_model_batcher(ops, golden_small):
    from videollama2_amd.model import VideoLLaMA2Hip
    cfg = golden_small["cfg"]
    model = VideoLLaMA2Hip(cfg, O.seeded_state_dict(cfg, golden_small["seed"], round_bf16=True), "cuda:0", max_seq_len=128)
    g = torch.Generator().manual_seed(5)
    rows = [torch.randint(3, cfg["llm"]["vocab_size"], (n,), generator=g) for n in (11, 70, 6)]
    solo16 = model.generate(rows[1][None], max_new_tokens=5)[0].tolist()
    model.enable_fp8_kv()
    solo = [model.generate(r[None], max_new_tokens=5)[0].tolist() for r in rows]        # the contiguous fp8-KV decode of every request
    model.enable_fp8_kv(False)
    assert model.enable_paged_kv(4, fp8=True) is model and model.decoder.paged_kv_fp8 and model.decoder.fp8_kv is False
    mb = model.batcher(max_slots=2)
    rid = [mb.submit(r[None], max_new_tokens=5) for r in rows]      # 1 + 2 + 1 pages on a pool of 3
    done = mb.run()
    assert [done[r].tolist() for r in rid] == solo
    assert model.decoder._bb["pool"].n_free == 3 and "pools8" in model.decoder._bb
    assert model.generate(rows[1][None], max_new_tokens=5)[0].tolist() == solo16        # the single-sequence path is untouched: 16-bit KV
    model.enable_paged_kv(0, False)
    assert not model.decoder.paged_kv and not model.decoder.paged_kv_fp8
    model.decoder._bb_busy = None
    del model, mb
    gc.collect()
    torch.cuda.empty_cache()
