"""The paged KV cache of the batched decode step on MI355X (include/vl2hip.h vl2_attn_decode_paged / vl2_kv_page_scatter, csrc/k_attn_paged.h,
DESIGN.md section 19).  Paging moves rows and changes no sum, so EVERY comparison here is torch.equal (on the storage bits where NaN poison is
involved): there is no tolerance in this file.  Kernels at nkv = 2, 256 positions (4 pages per sequence), both builds: the scatter is a byte
copy that touches nothing else; the attention equals vl2_attn_decode_batched on contiguous copies of the same rows in `out`, in the live
slices of `partial` and in the appended rows, and selects the right keys on the exact inputs of tests/attn_exact.py; a request without a page
or past the table writes nothing; a replayed graph crosses a page boundary like the eager contiguous steps.  Decoder and serving on the two
small golden configs: generate_batch, the continuous batcher and ModelBatcher on pages give the contiguous slots' tokens and logits."""
import gc

import pytest
import torch

from oracle import vl2_oracle as O
from tests import attn_exact as AX

pytestmark = pytest.mark.gpu
DEV = "cuda"
NKV, HD, SMAX = 2, 128, 256
PPS = SMAX // 64                                  # pages per sequence
SCALE = HD ** -0.5
POSITIONS = (0, 15, 63, 64, 65, 200)
SENTINEL = 0x5A5B                                 # the pools' bit pattern before a scatter (a finite 16-bit number in both element types)


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
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def _tables(rows=SMAX):
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.int64).float() / HD))
    fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().contiguous().to(DEV), fr.sin().contiguous().to(DEV)


def deal_pages(needs, n_pages, seed):
    """Page ids 1 .. n_pages - 1 shuffled and dealt to the requests (needs[b] pages each): non-monotone rows, interleaved across requests.
    -> (table rows as lists of PPS entries, -1 behind a request's pages; the ids nobody got)."""
    perm = (torch.randperm(n_pages - 1, generator=torch.Generator().manual_seed(seed)) + 1).tolist()
    rows = []
    for n in needs:
        rows.append(perm[:n] + [-1] * (PPS - n))
        perm = perm[n:]
    return rows, perm


def paginate(cache, rows, n_pages):
    """The pool [n_pages, nkv, 64, 128] that holds the contiguous caches [B, nkv, SMAX, 128] under the table `rows`; NaN in every page nobody
    owns (page 0 included)."""
    pool = torch.full((n_pages, cache.shape[1], 64, HD), float("nan"), dtype=cache.dtype, device=cache.device)
    for b, row in enumerate(rows):
        for j, page in enumerate(row):
            if 0 <= page < n_pages:
                pool[page] = cache[b, :, 64 * j:64 * j + 64]
    return pool


def _qkv(nh, seed, elem, rows):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((rows, (nh + 2 * NKV) * HD), generator=g) * 1.5).to(elem).to(DEV)


def _caches(positions, elem, seed):
    """Contiguous K and V [B, NKV, SMAX, 128]: random rows below each request's position, NaN from it on."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        c = torch.randn(len(positions), NKV, SMAX, HD, generator=g).to(elem)
        for b, p in enumerate(positions):
            c[b, :, p:] = float("nan")
        out.append(c.to(DEV))
    return out


def _nan_partial(B, nh, nsplit=PPS):
    return torch.full((B * nh * nsplit * 130,), float("nan"), dtype=torch.float32, device=DEV)


def _out(B, nh, elem):
    return torch.zeros((B, nh * HD), dtype=elem, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. the scatter
@pytest.mark.parametrize("p0,p1", [(0, 1), (0, 64), (63, 66), (0, 200)])
def test_scatter_copies_the_rows_byte_for_byte_and_nothing_else(ops, elem, p0, p1):
    n_pages = 12
    g = torch.Generator().manual_seed(100 + p1)
    k16 = torch.randn(NKV, SMAX, HD, generator=g).to(elem).to(DEV)
    v16 = torch.randn(NKV, SMAX, HD, generator=g).to(elem).to(DEV)
    mine, other = [7, 2, 9, 4], [3, 8, 1, 6]                  # non-monotone, interleaved with another request's pages
    for row in (mine, [7, -1, 9, 4], [7, n_pages, 9, n_pages + 5], [-1, -1, -1, -1]):
        kpool = bits(torch.empty((n_pages, NKV, 64, HD), dtype=elem, device=DEV)).fill_(SENTINEL).view(elem)
        vpool = bits(torch.empty((n_pages, NKV, 64, HD), dtype=elem, device=DEV)).fill_(SENTINEL + 1).view(elem)
        exp_k, exp_v = kpool.clone(), vpool.clone()
        for p in range(p0, p1):
            if 0 <= row[p // 64] < n_pages:
                exp_k[row[p // 64], :, p % 64] = k16[:, p]
                exp_v[row[p // 64], :, p % 64] = v16[:, p]
        table = torch.tensor([other, row], dtype=torch.int32, device=DEV)
        ops.kv_page_scatter(k16, v16, kpool, vpool, table[1], p0, p1)
        torch.cuda.synchronize()
        # the rows read back through the table are the staging rows; every other byte of both pools keeps the sentinel (the other
        # request's pages, the pages nobody owns, the rows of this request's pages outside [p0, p1), a row without a page)
        assert same_bits(kpool, exp_k) and same_bits(vpool, exp_v), row
        if row is mine:
            back_k = torch.cat([kpool[pg] for pg in row], 1)[:, p0:p1]
            assert same_bits(back_k, k16[:, p0:p1])
            untouched = torch.ones(n_pages, dtype=torch.bool, device=DEV)
            untouched[row] = False
            assert bool((bits(kpool)[untouched] == SENTINEL).all()) and bool((bits(vpool)[untouched] == SENTINEL + 1).all())


# ---------------------------------------------------------------------------------------------------------------- 2. the operator
class Case:
    """B = 6 requests at POSITIONS in one launch, computed once per (group, element type): random contiguous caches with NaN from `pos` on,
    their pages shuffled across the requests with NaN in every page nobody owns, and vl2_attn_decode_batched's results on the contiguous
    copies -- `out`, `partial` (NaN outside the slices it wrote) and the caches after the append."""

    def __init__(self, ops, group, elem, positions=POSITIONS, seed=0):
        self.nh, self.elem, self.positions = NKV * group, elem, positions
        B = self.B = len(positions)
        self.cos, self.sin = _tables()
        self.qkv = _qkv(self.nh, 10 * group + seed, elem, B)
        self.k0, self.v0 = _caches(positions, elem, 20 * group + seed)
        needs = [p // 64 + 1 for p in positions]
        self.n_pages = 1 + sum(needs) + 3
        self.rows, self.spare = deal_pages(needs, self.n_pages, 30 * group + seed)
        self.pos = torch.tensor(positions, dtype=torch.int32, device=DEV)
        self.k1, self.v1 = self.k0.clone(), self.v0.clone()
        self.partial = _nan_partial(B, self.nh)
        self.out = _out(B, self.nh, elem)
        ops.attn_decode_batched(self.qkv, self.k1, self.v1, self.cos, self.sin, self.partial, self.out, self.nh, NKV, self.pos, SMAX, SCALE)
        torch.cuda.synchronize()
        assert not bool(self.out.isnan().any())

    def table(self, rows=None):
        return torch.tensor(self.rows if rows is None else rows, dtype=torch.int32, device=DEV)

    def pools(self, rows=None):
        rows = self.rows if rows is None else rows
        return paginate(self.k0, rows, self.n_pages), paginate(self.v0, rows, self.n_pages)


_CASES = {}


def case(ops, group, elem):
    key = (group, elem)
    if key not in _CASES:
        _CASES[key] = Case(ops, group, elem)
    return _CASES[key]


@pytest.mark.parametrize("group", [4, 7], ids=["group4_mistral", "group7_qwen2"])
def test_paged_attention_equals_the_contiguous_call_bit_for_bit(ops, elem, group):
    c = case(ops, group, elem)
    kpool, vpool = c.pools()
    # the pages really are shuffled: some request's row is not ascending, and two requests' pages interleave
    assert any(r[j] > r[j + 1] >= 0 for r in c.rows for j in range(PPS - 1))
    partial, out = _nan_partial(c.B, c.nh), _out(c.B, c.nh, elem)
    ops.attn_decode_paged(c.qkv, kpool, vpool, c.table(), c.cos, c.sin, partial, out, c.nh, NKV, c.pos, SMAX, SCALE)
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
    # the pools after the step = the contiguous caches after theirs, page by page: the appended K / V rows byte for byte, every other row
    # (the NaN rows past `pos`, the pages nobody owns, page 0) untouched
    assert same_bits(kpool, paginate(c.k1, c.rows, c.n_pages)) and same_bits(vpool, paginate(c.v1, c.rows, c.n_pages))
    for b, pos in enumerate(c.positions):
        page = c.rows[b][pos // 64]
        assert same_bits(kpool[page, :, pos % 64], c.k1[b, :, pos]) and not bool(kpool[page, :, pos % 64].isnan().any()), b
        assert same_bits(vpool[page, :, pos % 64], c.v1[b, :, pos]), b
    # a smaller launch capacity (ctx_cap = the longest context): the same outputs
    partial2, out2 = _nan_partial(c.B, c.nh), _out(c.B, c.nh, elem)
    kpool, vpool = c.pools()
    ops.attn_decode_paged(c.qkv, kpool, vpool, c.table(), c.cos, c.sin, partial2, out2, c.nh, NKV, c.pos, max(c.positions) + 1, SCALE)
    torch.cuda.synchronize()
    assert torch.equal(out2, c.out)


@pytest.mark.parametrize("group", [4, 7], ids=["group4_mistral", "group7_qwen2"])
def test_a_wrong_page_would_select_a_wrong_key(ops, elem, group):
    """tests/attn_exact.py's key-selecting inputs (every K row encodes its own position, every query selects a power-of-two set of keys, the
    fp64 softmax rounded once is THE answer): the strided, poisoned batch of its batched cases, its rows moved into shuffled pages."""
    bt = AX.Batch(group, NKV, POSITIONS, elem, DEV)
    assert bt.smax % 64 == 0
    pps = bt.smax // 64
    needs = [p // 64 + 1 for p in POSITIONS]
    n_pages = 1 + sum(needs) + 2
    perm = (torch.randperm(n_pages - 1, generator=torch.Generator().manual_seed(group)) + 1).tolist()
    rows = []
    for n in needs:
        rows.append(perm[:n] + [-1] * (pps - n))
        perm = perm[n:]
    pools = []
    for cache in bt.cache:
        pool = torch.full((n_pages, NKV, 64, HD), float("nan"), dtype=elem, device=DEV)
        for b, row in enumerate(rows):
            for j, page in enumerate(row):
                if page >= 0:
                    pool[page] = cache[b, :, 64 * j:64 * j + 64]
        pools.append(pool)
    table = torch.tensor(rows, dtype=torch.int32, device=DEV)
    nh = bt.nh
    pst, partial = AX.partial_ws(bt.B * nh * pps * 130, DEV)
    out_st = torch.full((bt.B + 2, nh * HD + 8), AX.SENTINEL, dtype=elem, device=DEV)
    out = out_st[1:bt.B + 1, :nh * HD]
    ops.attn_decode_paged(bt.qkv, pools[0], pools[1], table, bt.cos, bt.sin, partial, out, nh, NKV, bt.pos_dev, bt.smax, AX.SCALE)
    o = out_st.cpu()
    keep = torch.ones(o.shape, dtype=torch.bool)
    keep[1:bt.B + 1, :nh * HD] = False
    assert bool((o[keep] == AX.SENTINEL).all()) and AX.bands_intact(pst.cpu())
    for b, r in enumerate(bt.reqs):
        exp = AX.expected(r.reference()[0], elem)
        y = o[b + 1, :nh * HD]
        assert torch.equal(y, exp), f"request {b} (pos {r.pos}): {AX.first_diff(y, exp)}"
        page = rows[b][r.pos // 64]
        row = [pools[0][page, :, r.pos % 64].cpu(), pools[1][page, :, r.pos % 64].cpu()]
        assert AX.new_row_error(r, row, elem, False, f"request {b}") is None


# ---------------------------------------------------------------------------------------------------------------- 3. the guards
@pytest.mark.parametrize("how", ["page_unassigned", "page_outside_the_pool", "pos_at_seq_cap", "pos_past_seq_cap"])
def test_a_request_without_a_page_or_past_the_table_writes_nothing(ops, elem, how):
    """Request 4 (position 65, pages for slices 0 and 1) is broken in one way.  It must leave both pools bit-unchanged, and the other
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
    kref, vref = c.pools()
    oref = _out(len(others), c.nh, elem)
    ops.attn_decode_paged(c.qkv[idx], kref, vref, c.table()[idx], c.cos, c.sin, _nan_partial(len(others), c.nh), oref, c.nh, NKV, c.pos[idx], SMAX, SCALE)
    assert torch.equal(oref, c.out[idx])
    kpool, vpool = c.pools()
    out = _out(c.B, c.nh, elem)
    ops.attn_decode_paged(c.qkv, kpool, vpool, c.table(rows), c.cos, c.sin, _nan_partial(c.B, c.nh), out, c.nh, NKV, pos, SMAX, SCALE)
    torch.cuda.synchronize()
    assert torch.equal(out[idx], oref)
    assert same_bits(kpool, kref) and same_bits(vpool, vref)


# ---------------------------------------------------------------------------------------------------------------- 4. graph = eager
def test_replayed_graph_crosses_a_page_boundary_like_the_eager_contiguous_steps(ops, elem):
    nh, B, steps = NKV * 4, 2, 5
    pos0 = (62, 130)                                              # request 0 walks 62 .. 66: from its page 0 into its page 1
    cos, sin = _tables()
    qkvs = [_qkv(nh, 70 + s, elem, B) for s in range(steps)]
    k, v = _caches(pos0, elem, 5)
    kc, vc = k.clone(), v.clone()
    pos = torch.tensor(pos0, dtype=torch.int32, device=DEV)
    outs = torch.zeros(steps, B, nh * HD, dtype=elem, device=DEV)
    pc = _nan_partial(B, nh)
    for s in range(steps):                                        # eager, contiguous
        ops.attn_decode_batched(qkvs[s], kc, vc, cos, sin, pc, outs[s], nh, NKV, pos, SMAX, SCALE)
        pos += 1
    rows = [[5, 2, -1, -1], [4, 6, 1, -1]]
    n_pages = 8
    kpool, vpool = paginate(k, rows, n_pages), paginate(v, rows, n_pages)
    fresh = (kpool.clone(), vpool.clone())
    table = torch.tensor(rows, dtype=torch.int32, device=DEV)
    pos = torch.tensor(pos0, dtype=torch.int32, device=DEV)
    qbuf, obuf, pp = qkvs[0].clone(), _out(B, nh, elem), _nan_partial(B, nh)

    def step():
        ops.attn_decode_paged(qbuf, kpool, vpool, table, cos, sin, pp, obuf, nh, NKV, pos, SMAX, SCALE)
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
    kpool.copy_(fresh[0]); vpool.copy_(fresh[1])                  # back to the start: all five steps are replays
    pos.copy_(torch.tensor(pos0, dtype=torch.int32))
    for s in range(steps):
        qbuf.copy_(qkvs[s])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(obuf, outs[s]), s
    assert pos.tolist() == [p + steps for p in pos0]
    assert same_bits(kpool, paginate(kc, rows, n_pages)) and same_bits(vpool, paginate(vc, rows, n_pages))
    assert not bool(kpool[2, :, :3].isnan().any()) and bool(kpool[2, :, 3:].isnan().all())      # rows 64 .. 66 landed in page 2


# ---------------------------------------------------------------------------------------------------------------- 5. decoder
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


LENS = (70, 5, 129, 33, 64)                       # beside the golden prompt: ragged, below / at / above a page edge
N_NEW = 6


def _decoder(golden, max_seq_len):
    from videollama2_amd.decoder import HipMistralDecoder
    cfg = golden["cfg"]
    assert cfg["llm"]["head_dim"] == 128
    dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, golden["seed"], only=_keep), DEV, max_seq_len=max_seq_len)
    g = torch.Generator().manual_seed(21)
    embeds = [golden["inputs_embeds"].to(DEV).bfloat16()] + [(torch.randn(n, dec.D, generator=g) * 0.5).bfloat16().to(DEV) for n in LENS]
    return dec, embeds


@pytest.fixture(scope="module", params=["mistral", "v21"])
def small(request, ops, golden_small, golden_small_v21):
    # max_seq_len 200 (v21): no multiple of the page, so the table covers 256 positions and the step gets cos / sin tables of its own
    dec, embeds = _decoder(golden_small if request.param == "mistral" else golden_small_v21, 256 if request.param == "mistral" else 200)
    yield dec, embeds
    # a decoder that served a batcher is in a reference cycle with it: collect the pair (and its captured graphs) here, not at some later
    # moment of the collector's choosing
    dec._bb_busy = None
    del dec
    gc.collect()
    torch.cuda.empty_cache()


def _needs(dec, embeds, n_new):
    from videollama2_amd.paging import pages_needed
    return [pages_needed(e.shape[0], n_new, dec.max_seq_len) for e in embeds]


@pytest.mark.parametrize("fmt", ["16bit", "fp8"])
def test_generate_batch_on_pages_equals_the_contiguous_slots(small, fmt, monkeypatch):
    dec, embeds = small
    if fmt == "fp8":
        dec.enable_fp8_decode()
    try:
        runs = {}
        for nb in (3, 6):                                         # the multi-row GEMV step, the skinny-M step
            runs[nb] = dec.generate_batch(embeds[:nb], max_new_tokens=N_NEW, return_logits=True)
        gen = lambda: torch.Generator(device=DEV).manual_seed(7)
        sampled = dec.generate_batch(embeds[:3], max_new_tokens=N_NEW, sampler=(0.8, 20, 0.9, gen()))
        total = sum(_needs(dec, embeds, N_NEW))
        dec.enable_paged_kv(total + 1)
        assert dec.paged_kv and dec.decode_format == fmt
        for nb in (3, 6):
            outs, logits = dec.generate_batch(embeds[:nb], max_new_tokens=N_NEW, return_logits=True)
            assert [o.tolist() for o in outs] == [o.tolist() for o in runs[nb][0]], nb
            assert torch.equal(logits, runs[nb][1]), nb
            pool = dec._bb["pool"]
            assert pool.n_free == total and dec._bb["table"][:nb].tolist() == [[0] + [-1] * (dec._bb["pages_per_seq"] - 1)] * nb
        again = dec.generate_batch(embeds[:3], max_new_tokens=N_NEW, sampler=(0.8, 20, 0.9, gen()))
        assert [o.tolist() for o in again] == [o.tolist() for o in sampled]
        eager = dec.generate_batch(embeds[:3], max_new_tokens=N_NEW, return_logits=True, use_graph=False)
        assert torch.equal(eager[1], runs[3][1])
        # memory: the pools are n_pages pages, and nothing in the slot buffers has max_seq_len rows per slot
        bb = dec._bb
        pool_bytes = sum(t.numel() * t.element_size() for t in bb["kpool"] + bb["vpool"])
        assert pool_bytes == (total + 1) * dec.kv_page_bytes()
        assert not any(k in bb for k in ("k", "v", "kv8"))
        for key, val in bb.items():
            tensors = [val] if torch.is_tensor(val) else [t for grp in val for t in grp] if key == "stage" else val if isinstance(val, list) else []
            for t in tensors:
                per_slot_rows = t.dim() >= 3 and t.shape[0] == bb["B"] and dec.max_seq_len in t.shape[1:]
                assert not per_slot_rows, (key, tuple(t.shape))
                if key == "stage":
                    assert tuple(t.shape) == (dec.nkv, dec.max_seq_len, 128)
        # a pool one page too small: refused before any kernel, every page still free
        dec.enable_paged_kv(total)
        from videollama2_amd import _lib

        def boom(*a, **k):
            raise AssertionError("a kernel was called")
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "call", boom)
            with pytest.raises(ValueError, match=f"need {total} pages .* the pool has {total - 1} free"):
                dec.generate_batch(embeds, max_new_tokens=N_NEW)
        assert dec._bb["pool"].n_free == total - 1
        # an error inside the call, with the pages reserved, gives them back as well
        def broken(*a, **k):
            assert dec._bb["pool"].n_free < total - 1
            raise RuntimeError("prefill failed")
        with monkeypatch.context() as mp:
            mp.setattr(dec, "prefill_slot", broken)
            with pytest.raises(RuntimeError, match="prefill failed"):
                dec.generate_batch(embeds[:2], max_new_tokens=N_NEW)
        assert dec._bb["pool"].n_free == total - 1 and dec._bb["table"][:, 0].tolist() == [0] * dec._bb["B"]
        # off again: the contiguous slots and their bits
        dec.enable_paged_kv(0, False)
        outs, logits = dec.generate_batch(embeds[:3], max_new_tokens=N_NEW, return_logits=True)
        assert torch.equal(logits, runs[3][1]) and "k" in dec._bb and "kpool" not in dec._bb
    finally:
        dec.enable_paged_kv(0, False)
        if fmt == "fp8":
            dec.enable_fp8_decode(False)


# ---------------------------------------------------------------------------------------------------------------- 6. serving
def test_continuous_batcher_on_a_pool_that_holds_two_reservations(small):
    """6 requests of mixed length through 4 slots and a pool of 5 pages: every reservation is 2 or 3 pages, so no three requests fit at once.
    Every request's tokens equal its solo greedy decode, admission is in submission order, the pages of retired requests are reused dirty,
    and after run() every page is free again."""
    from videollama2_amd.serving import ContinuousBatcher
    dec, embeds = small
    g = torch.Generator().manual_seed(33)
    lens, n_new = (70, 129, 65, 100, 120, 64), (6, 3, 8, 5, 10, 4)
    reqs = [(torch.randn(n, dec.D, generator=g) * 0.5).bfloat16().to(DEV) for n in lens]
    solo = [dec.generate(e, max_new_tokens=n, use_graph=True)[0].tolist() for e, n in zip(reqs, n_new)]
    dec.enable_paged_kv(6)
    try:
        for use_graph in (True, False):
            b = ContinuousBatcher(dec, max_slots=4, use_graph=use_graph)
            rid = [b.submit(e, max_new_tokens=n) for e, n in zip(reqs, n_new)]
            needs = [r.need for r in b.waiting]
            assert needs == [2, 3, 2, 2, 3, 2]
            order, owners, most = [], {}, 0
            while b.in_flight():
                b.step()
                now = [r for r in b.slots if r is not None]
                assert sum(r.need for r in now) <= 5
                for r in sorted(now, key=lambda r: r.rid):
                    if r.rid not in order:
                        order.append(r.rid)
                        for pg in r.pages:
                            owners.setdefault(pg, []).append(r.rid)
                most = max(most, len(now))
            done = b.finished
            assert [done[r].tolist() for r in rid] == solo, use_graph
            assert order == rid and most == 2
            assert 0 not in owners and max(len(o) for o in owners.values()) >= 2        # a freed (dirty) page served a later request
            bb = dec._bb
            assert bb["pool"].n_free == 5 and bb["table"].tolist() == [[0] + [-1] * (bb["pages_per_seq"] - 1)] * 4
    finally:
        dec.enable_paged_kv(0, False)


def test_model_level_switch_and_model_batcher(ops, golden_small):
    from videollama2_amd.model import VideoLLaMA2Hip
    cfg = golden_small["cfg"]
    model = VideoLLaMA2Hip(cfg, O.seeded_state_dict(cfg, golden_small["seed"], round_bf16=True), "cuda:0", max_seq_len=128)
    g = torch.Generator().manual_seed(5)
    rows = [torch.randint(3, cfg["llm"]["vocab_size"], (n,), generator=g) for n in (11, 70, 6)]
    solo = [model.generate(r[None], max_new_tokens=5)[0].tolist() for r in rows]
    assert model.enable_paged_kv(4) is model and model.decoder.paged_kv
    mb = model.batcher(max_slots=2)
    rid = [mb.submit(r[None], max_new_tokens=5) for r in rows]      # 1 + 2 + 1 pages on a pool of 3
    done = mb.run()
    assert [done[r].tolist() for r in rid] == solo
    assert model.decoder._bb["pool"].n_free == 3
    assert model.generate(rows[1][None], max_new_tokens=5)[0].tolist() == solo[1]       # the single-sequence path is untouched
    model.enable_paged_kv(0, False)
    assert not model.decoder.paged_kv
    model.decoder._bb_busy = None
    del model, mb
    gc.collect()
    torch.cuda.empty_cache()
