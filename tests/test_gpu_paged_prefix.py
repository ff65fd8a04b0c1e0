"""A shared prompt prefix held once in the page pool, on MI355X (include/vl2hip.h vl2_attn_decode_shared_paged / vl2_kv_page_gather,
csrc/k_attn_paged_shared.h).  Paging the cascade moves rows and changes no sum, so EVERY comparison here is torch.equal
(on the storage bits where NaN poison is involved): there is no tolerance in this file.  Kernels at nkv = 2, head_dim 128, both builds: the
gather inverts the scatter and touches nothing else; the operator equals vl2_attn_decode_shared on contiguous copies of the same rows in `out`,
in the live slices of `partial` and in the appended rows, and selects the right keys on tests/attn_exact.py's inputs; the guards.  Serving on the
two small golden configs: ContinuousBatcher.open_prefix / submit(prefix=) / close_prefix and ModelBatcher.open_video give every request the
tokens of its solo generate_batch(shared_prefix=) on an unpaged decoder.  Every test needs the new entry points: none passes without them."""
import gc

import pytest
import torch

from oracle import vl2_oracle as O
from tests import attn_exact as AX

pytestmark = pytest.mark.gpu
DEV = "cuda"
NKV, HD = 2, 128
SCALE = HD ** -0.5
OWN_CAP = 192
OWNS = (0, 15, 63, 64, 65, 130)                   # pos - Pf of the requests of one launch (cycled)
SENTINEL = 0x5A5B


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


def _tables(rows):
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.int64).float() / HD))
    fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().contiguous().to(DEV), fr.sin().contiguous().to(DEV)


def _filled(shape, elem, pattern):
    return bits(torch.empty(shape, dtype=elem, device=DEV)).fill_(pattern).view(elem)


# ---------------------------------------------------------------------------------------------------------------- 1. gather and scatter
@pytest.mark.parametrize("p0,p1", [(0, 1), (0, 64), (63, 66), (0, 200)])
def test_gather_inverts_scatter_and_writes_nothing_else(ops, elem, p0, p1):
    smax, n_pages = 256, 12
    g = torch.Generator().manual_seed(200 + p1)
    k16 = torch.randn(NKV, smax, HD, generator=g).to(elem).to(DEV)
    v16 = torch.randn(NKV, smax, HD, generator=g).to(elem).to(DEV)
    kp0 = torch.randn(n_pages, NKV, 64, HD, generator=g).to(elem).to(DEV)
    vp0 = torch.randn(n_pages, NKV, 64, HD, generator=g).to(elem).to(DEV)
    other = [3, 8, 1, 6]
    for row in ([7, 2, 9, 4], [7, -1, 9, 4], [7, n_pages, 9, n_pages + 5], [-1, -1, -1, -1]):
        table = torch.tensor([other, row], dtype=torch.int32, device=DEV)
        live = [p for p in range(p0, p1) if 0 <= row[p // 64] < n_pages]
        # gather(scatter(x)) == x on the rows that have a page; every other byte of the caches keeps the sentinel
        kpool, vpool = _filled(kp0.shape, elem, SENTINEL), _filled(kp0.shape, elem, SENTINEL + 1)
        ops.kv_page_scatter(k16, v16, kpool, vpool, table[1], p0, p1)
        pools_before = (kpool.clone(), vpool.clone())
        kb, vb = _filled(k16.shape, elem, SENTINEL + 2), _filled(k16.shape, elem, SENTINEL + 3)
        exp_k, exp_v = kb.clone(), vb.clone()
        for p in live:
            exp_k[:, p], exp_v[:, p] = k16[:, p], v16[:, p]
        ops.kv_page_gather(kpool, vpool, kb, vb, table[1], p0, p1)
        torch.cuda.synchronize()
        assert same_bits(kb, exp_k) and same_bits(vb, exp_v), row
        assert same_bits(kpool, pools_before[0]) and same_bits(vpool, pools_before[1])          # the gather reads the pools only
        # scatter(gather(pools)) == pools on those rows; every other byte of the second pools keeps the sentinel
        kb, vb = _filled(k16.shape, elem, SENTINEL + 2), _filled(k16.shape, elem, SENTINEL + 3)
        ops.kv_page_gather(kp0, vp0, kb, vb, table[1], p0, p1)
        kpool, vpool = _filled(kp0.shape, elem, SENTINEL), _filled(kp0.shape, elem, SENTINEL + 1)
        exp_k, exp_v = kpool.clone(), vpool.clone()
        for p in live:
            exp_k[row[p // 64], :, p % 64], exp_v[row[p // 64], :, p % 64] = kp0[row[p // 64], :, p % 64], vp0[row[p // 64], :, p % 64]
        ops.kv_page_scatter(kb, vb, kpool, vpool, table[1], p0, p1)
        torch.cuda.synchronize()
        assert same_bits(kpool, exp_k) and same_bits(vpool, exp_v), row


# ---------------------------------------------------------------------------------------------------------------- 2. the operator
def deal(n_pre, needs, n_pages, seed):
    """Page ids 1 .. n_pages - 1 shuffled and dealt to the prefix (n_pre) and then to the requests (needs[b]) so that no two consecutive
    pages of the prefix or of a request are neighbours in the pool.  -> (prefix pages, own pages per request, the ids nobody got)."""
    for s in range(seed, seed + 1000):
        perm = (torch.randperm(n_pages - 1, generator=torch.Generator().manual_seed(s)) + 1).tolist()
        lists, at = [], 0
        for n in [n_pre] + list(needs):
            lists.append(perm[at:at + n])
            at += n
        if all(abs(a - b) != 1 for lst in lists for a, b in zip(lst, lst[1:])):
            return lists[0], lists[1:], perm[at:]
    raise AssertionError("no shuffle without neighbours")


class Case:
    """nb requests at own offsets OWNS (cycled) behind a prefix of Pf rows, computed once per (group, element type, Pf, nb): random contiguous
    prefix caches (NaN from Pf on) and private caches (NaN from pos - Pf on), vl2_attn_decode_shared's results on them -- `out`, `partial`
    (NaN outside the slices it wrote), the private caches after the append -- and the same rows in pages dealt from one shuffled pool, NaN
    in every page nobody owns."""

    def __init__(self, ops, group, elem, Pf, nb, seed=0):
        self.nh, self.elem, self.Pf, self.nb = NKV * group, elem, Pf, nb
        self.owns = [OWNS[b % len(OWNS)] for b in range(nb)]
        g = torch.Generator().manual_seed(1000 * group + Pf + nb + seed)
        nan = float("nan")
        self.cos, self.sin = _tables(Pf + OWN_CAP)
        self.qkv = (torch.randn((nb, (self.nh + 2 * NKV) * HD), generator=g) * 1.5).to(elem).to(DEV)
        pre = []
        for _ in range(2):
            c = torch.randn(NKV, Pf + 64, HD, generator=g).to(elem)
            c[:, Pf:] = nan
            pre.append(c.to(DEV))
        self.kpre, self.vpre = pre
        own = []
        for _ in range(2):
            c = torch.randn(nb, NKV, OWN_CAP, HD, generator=g).to(elem)
            for b, o in enumerate(self.owns):
                c[b, :, o:] = nan
            own.append(c.to(DEV))
        self.k0, self.v0 = own
        self.pos = torch.tensor([Pf + o for o in self.owns], dtype=torch.int32, device=DEV)
        self.per = ops.shared_partial_floats(Pf, OWN_CAP, self.nh)
        self.nps = ops.shared_prefix_splits(Pf)
        self.k1, self.v1 = self.k0.clone(), self.v0.clone()
        self.partial = self.nan_partial()
        self.out = self.zero_out()
        ops.attn_decode_shared(self.qkv, self.kpre, self.vpre, self.k1, self.v1, self.cos, self.sin, self.partial, self.out, self.nh, NKV, Pf,
                               self.pos, SCALE)
        torch.cuda.synchronize()
        assert not bool(self.out.isnan().any())
        self.n_pre = Pf // 64
        needs = [o // 64 + 1 for o in self.owns]
        self.n_pages = 1 + self.n_pre + sum(needs) + 3
        self.pre_pages, self.own_pages, self.spare = deal(self.n_pre, needs, self.n_pages, 7 * group + Pf + nb)
        self.pps = self.n_pre + OWN_CAP // 64
        self.rows = [self.pre_pages + pg + [-1] * (self.pps - self.n_pre - len(pg)) for pg in self.own_pages]

    def nan_partial(self, nb=None):
        return torch.full(((self.nb if nb is None else nb) * self.per,), float("nan"), dtype=torch.float32, device=DEV)

    def zero_out(self, nb=None):
        return torch.zeros((self.nb if nb is None else nb, self.nh * HD), dtype=self.elem, device=DEV)

    def table(self, rows=None):
        return torch.tensor(self.rows if rows is None else rows, dtype=torch.int32, device=DEV)

    def prefix_pages(self, pages=None):
        return torch.tensor(self.pre_pages if pages is None else pages, dtype=torch.int32, device=DEV)

    def paginate(self, pre, own):
        """The pool that holds the prefix cache `pre` and the private caches `own` under the dealt pages; NaN everywhere else."""
        pool = torch.full((self.n_pages, NKV, 64, HD), float("nan"), dtype=self.elem, device=DEV)
        for j, page in enumerate(self.pre_pages):
            pool[page] = pre[:, 64 * j:64 * j + 64]
        for b, pg in enumerate(self.own_pages):
            for j, page in enumerate(pg):
                pool[page] = own[b, :, 64 * j:64 * j + 64]
        return pool

    def pools(self):
        return self.paginate(self.kpre, self.k0), self.paginate(self.vpre, self.v0)

    def run(self, ops, kpool, vpool, table=None, prefix_pages=None, pos=None, idx=None):
        idx = slice(None) if idx is None else idx
        qkv, tab, pos = self.qkv[idx], (self.table() if table is None else table)[idx], (self.pos if pos is None else pos)[idx]
        partial, out = self.nan_partial(qkv.shape[0]), self.zero_out(qkv.shape[0])
        ops.attn_decode_shared_paged(qkv, kpool, vpool, tab, self.prefix_pages() if prefix_pages is None else prefix_pages, self.cos, self.sin,
                                     partial, out, self.nh, NKV, self.Pf, OWN_CAP, pos, SCALE)
        torch.cuda.synchronize()
        return out, partial


_CASES = {}


def case(ops, group, elem, Pf, nb):
    key = (group, elem, Pf, nb)
    if key not in _CASES:
        _CASES[key] = Case(ops, group, elem, Pf, nb)
    return _CASES[key]


@pytest.mark.parametrize("nb", [1, 5, 33])
@pytest.mark.parametrize("Pf", [64, 128, 192, 3136])       # one tile; two tiles in one split; two splits, the last short; three tiles per split
@pytest.mark.parametrize("group", [4, 7], ids=["group4_mistral", "group7_qwen2"])
def test_paged_shared_attention_equals_the_contiguous_call_bit_for_bit(ops, elem, group, Pf, nb):
    c = case(ops, group, elem, Pf, nb)
    assert c.nps == {64: 1, 128: 1, 192: 2, 3136: 17}[Pf]
    kpool, vpool = c.pools()
    out, partial = c.run(ops, kpool, vpool)
    assert torch.equal(out, c.out), int((out != c.out).sum())
    # partial [nb][nh][nps + 3][130]: the live slices hold the contiguous call's bits, the others were not written (both still NaN)
    assert same_bits(partial, c.partial)
    p4 = partial.view(nb, c.nh, c.nps + OWN_CAP // 64, 130)
    for b, o in enumerate(c.owns):
        n = c.nps + o // 64 + 1
        assert not bool(p4[b, :, :n].isnan().any()) and bool(p4[b, :, n:].isnan().all()), b
    # the pools after the step = the contiguous caches after theirs, page by page: the appended K / V rows byte for byte; the prefix pages,
    # the NaN rows past `pos`, the pages nobody owns and page 0 untouched
    assert same_bits(kpool, c.paginate(c.kpre, c.k1)) and same_bits(vpool, c.paginate(c.vpre, c.v1))
    for b, o in enumerate(c.owns):
        page = c.own_pages[b][o // 64]
        assert same_bits(kpool[page, :, o % 64], c.k1[b, :, o]) and not bool(kpool[page, :, o % 64].isnan().any()), b
        assert same_bits(vpool[page, :, o % 64], c.v1[b, :, o]), b
    k_before, v_before = c.pools()
    quiet = torch.tensor([0] + c.pre_pages + c.spare, device=DEV)
    assert same_bits(kpool[quiet], k_before[quiet]) and same_bits(vpool[quiet], v_before[quiet])


@pytest.mark.parametrize("which", [2, 6], ids=["P128", "P3072"])
@pytest.mark.parametrize("group", [4, 7], ids=["group4_mistral", "group7_qwen2"])
def test_a_wrong_page_or_tile_would_select_a_wrong_key(ops, elem, group, which):
    """tests/attn_exact.py's SharedCase (every K row encodes its own position, every query selects a power-of-two set of keys across the prefix,
    the own rows and the boundary; the fp64 softmax rounded once is THE answer) at its page-aligned P, its rows moved into shuffled pages."""
    P, own_cap, nb, owns = AX.SHARED_CASES[which]
    assert P % 64 == 0
    sc = AX.SharedCase(P, own_cap, nb, owns, group, NKV, elem, DEV)
    n_pre, n_own = P // 64, own_cap // 64
    n_pages = 1 + n_pre + nb * n_own + 2
    pre_pages, own_pages, _ = deal(n_pre, [n_own] * nb, n_pages, group + which)
    pools = []
    for pre, own in ((sc.kprefix, sc.kown_st), (sc.vprefix, sc.vown_st)):
        pool = torch.full((n_pages, NKV, 64, HD), float("nan"), dtype=elem, device=DEV)
        for j, page in enumerate(pre_pages):
            pool[page] = pre[:, 64 * j:64 * j + 64]
        for b, pg in enumerate(own_pages):
            for j, page in enumerate(pg):
                pool[page] = own[b + 1, :, 64 * j:64 * j + 64]
        pools.append(pool)
    table = torch.tensor([pre_pages + pg for pg in own_pages], dtype=torch.int32, device=DEV)
    nh, w = sc.nh, (sc.nh + 2 * NKV) * HD
    pst, partial = AX.partial_ws(nb * ops.shared_partial_floats(P, own_cap, nh), DEV)
    out_st = torch.full((nb + 2, nh * HD + 8), AX.SENTINEL, dtype=elem, device=DEV)
    ops.attn_decode_shared_paged(sc.qkv_st[1:nb + 1, :w], pools[0], pools[1], table, torch.tensor(pre_pages, dtype=torch.int32, device=DEV),
                                 sc.cos, sc.sin, partial, out_st[1:nb + 1, :nh * HD], nh, NKV, P, own_cap, sc.pos_dev, AX.SCALE)
    o = out_st.cpu()
    keep = torch.ones(o.shape, dtype=torch.bool)
    keep[1:nb + 1, :nh * HD] = False
    assert bool((o[keep] == AX.SENTINEL).all()) and AX.bands_intact(pst.cpu())
    Kp, Vp = AX.k_rows(NKV, 0, torch.arange(P)).double(), AX.world().v_rows(NKV, 0, torch.arange(P)).double()
    for b, r in enumerate(sc.reqs):
        keys = torch.arange(P, r.pos)
        K = torch.cat([Kp, AX.k_rows(NKV, 0, keys).double(), r.k_new[:, None]], 1)
        V = torch.cat([Vp, AX.world().v_rows(NKV, b + 1, keys).double(), r.v_new[:, None]], 1)
        exp = AX.expected(r.reference(K, V)[0], elem)
        y = o[b + 1, :nh * HD]
        assert torch.equal(y, exp), f"request {b} (pos {r.pos}): {AX.first_diff(y, exp)}"
        own = r.pos - P
        page = own_pages[b][own // 64]
        assert torch.equal(pools[0][page, :, own % 64].cpu().double(), r.k_new) and torch.equal(pools[1][page, :, own % 64].cpu().double(), r.v_new), b


# ---------------------------------------------------------------------------------------------------------------- 3. the guards
@pytest.mark.parametrize("how", ["pos_below_the_prefix", "pos_at_own_cap", "own_page_unassigned", "own_page_outside_the_pool"])
def test_a_request_outside_its_window_or_without_an_own_page_writes_nothing(ops, elem, how):
    """Request 4 (own offset 65: own slices 0 and 1) is broken in one way.  It must leave both pools bit-unchanged and, where its position is
    outside [Pf, Pf + own_cap), its output row and its region of `partial` as well; the other requests' results equal a launch without it."""
    c = case(ops, 4, elem, 128, 5)
    victim, others = 4, torch.tensor([0, 1, 2, 3], device=DEV)
    rows, pos = [list(r) for r in c.rows], c.pos.clone()
    if how == "own_page_unassigned":
        rows[victim][c.n_pre + 1] = -1
    elif how == "own_page_outside_the_pool":
        rows[victim][c.n_pre + 1] = c.n_pages + (0 if elem == torch.bfloat16 else 7)
    else:
        pos[victim] = c.Pf - 1 if how == "pos_below_the_prefix" else c.Pf + OWN_CAP
    kref, vref = c.pools()
    oref, _ = c.run(ops, kref, vref, idx=others)
    assert torch.equal(oref, c.out[others])
    kpool, vpool = c.pools()
    out, partial = c.run(ops, kpool, vpool, table=c.table(rows), pos=pos)
    assert torch.equal(out[others], oref)
    assert same_bits(kpool, kref) and same_bits(vpool, vref)
    if how.startswith("pos"):
        assert not bool(out[victim].any()) and bool(partial.view(c.nb, -1)[victim].isnan().all())


@pytest.mark.parametrize("bad", [-1, "n_pages"])
def test_a_prefix_page_outside_the_pool_reads_nothing_and_the_call_succeeds(ops, elem, bad):
    """One prefix id outside [0, n_pages): the tile's buffer resources have length zero, so no memory is read; the launch succeeds, the pools
    end as after the unbroken launch (the own rows' appends, nothing else) and the device is healthy afterwards."""
    c = case(ops, 4, elem, 192, 5)
    kref, vref = c.pools()
    c.run(ops, kref, vref)
    for at in range(c.n_pre):
        pages = list(c.pre_pages)
        pages[at] = -1 if bad == -1 else c.n_pages
        kpool, vpool = c.pools()
        out, _ = c.run(ops, kpool, vpool, prefix_pages=c.prefix_pages(pages))
        assert same_bits(kpool, kref) and same_bits(vpool, vref), at
        assert not bool(out.isnan().any())                  # a zero tile in place of NaN pages: finite (and unspecified)
    out, _ = c.run(ops, kref.clone(), vref.clone())
    assert torch.equal(out, c.out)


# ---------------------------------------------------------------------------------------------------------------- 4. serving
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


@pytest.fixture(scope="module", params=["mistral", "v21"])
def small(request, ops, golden_small, golden_small_v21):
    # max_seq_len 200 (v21): no multiple of the page, so the table covers 256 positions and the step gets cos / sin tables of its own
    from videollama2_amd.decoder import HipMistralDecoder
    golden = golden_small if request.param == "mistral" else golden_small_v21
    cfg = golden["cfg"]
    assert cfg["llm"]["head_dim"] == 128
    dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, golden["seed"], only=_keep), DEV, max_seq_len=256 if request.param == "mistral" else 200)
    yield dec
    dec._bb_busy = None
    del dec
    gc.collect()
    torch.cuda.empty_cache()


def _rows(n, D, seed):
    return (torch.randn(n, D, generator=torch.Generator().manual_seed(seed)) * 0.5).bfloat16().to(DEV)


def _solo(dec, x_prefix, suffixes, n_new, **kw):
    """THE definition: each request alone through generate_batch(shared_prefix=) on the unpaged decoder, the ragged tail in front of its suffix."""
    assert not dec.paged_kv
    Pf = x_prefix.shape[0] // 64 * 64
    return [dec.generate_batch([torch.cat([x_prefix[Pf:], s])], max_new_tokens=n, shared_prefix=x_prefix[:Pf], **kw)[0].tolist()
            for s, n in zip(suffixes, n_new)]


LENS, N_NEW = (5, 9, 1, 45, 30, 17), (6, 3, 8, 3, 10, 5)


@pytest.mark.parametrize("tail", [0, 21])
@pytest.mark.parametrize("fmt", ["16bit", "fp8"])
def test_batcher_over_a_resident_prefix_equals_the_solo_shared_decodes(ops, small, fmt, tail, monkeypatch):
    """6 requests through 4 slots behind a prefix of 128 + tail rows, own reservations of 1 or 2 pages on a pool that holds the prefix and 3
    more.  Three requests join at the first step; the middle one retires first and leaves a live hole; a foreign prefill then takes the
    single-sequence cache; the other three are submitted behind it (the first of them waits for pages with a slot free, and blocks the two
    behind it)."""
    from videollama2_amd import ops as vops
    from videollama2_amd.paging import own_pages_needed
    from videollama2_amd.serving import ContinuousBatcher
    dec = small
    P = 128 + tail
    x_prefix = _rows(P, dec.D, 50 + tail)
    suf = [_rows(n, dec.D, 60 + i) for i, n in enumerate(LENS)]
    plain = _rows(70, dec.D, 77)
    if fmt == "fp8":
        dec.enable_fp8_decode()
    try:
        solo = _solo(dec, x_prefix, suf, N_NEW)
        plain_solo = dec.generate(plain, max_new_tokens=5, use_graph=True)[0].tolist()
        dec.enable_paged_kv(1 + 2 + 3)
        b = ContinuousBatcher(dec, max_slots=4)
        h = b.open_prefix(x_prefix)
        bb = dec._bb
        pool, pps = bb["pool"], bb["pages_per_seq"]
        assert (h.P, h.shared_rows, h.pages) == (P, 128, [1, 2]) and pool.n_free == 3
        assert bb["table"][:4].tolist() == [[1, 2, 0] + [-1] * (pps - 3)] * 4
        needs = [own_pages_needed(P, n, m, dec.max_seq_len) for n, m in zip(LENS, N_NEW)]
        assert set(needs) == ({1, 2} if tail else {1})
        seen, gathers = [], []
        admit, gather = b._admit, vops.kv_page_gather
        monkeypatch.setattr(b, "_admit", lambda: (admit(), seen.append([None if r is None else r.rid for r in b.slots]))[0])
        monkeypatch.setattr(vops, "kv_page_gather", lambda *a: (gathers.append(a[-2:]), gather(*a))[1])
        rid = [b.submit(s, max_new_tokens=n, prefix=h) for s, n in zip(suf[:3], N_NEW[:3])]
        order, owners = [], {}

        def step():
            b.step()
            used = pool.n_pages - 1 - pool.n_free
            now = [r for r in b.slots if r is not None]
            assert used == len(h.pages) + sum(r.need for r in now)                     # memory: the prefix once + the own reservations
            for r in sorted(now, key=lambda r: r.rid):
                if r.rid not in order:
                    order.append(r.rid)
                    for pg in r.pages:
                        owners.setdefault(pg, []).append(r.rid)
                    assert bb["table"][r.slot].tolist() == h.pages + r.pages + [-1] * (pps - 2 - len(r.pages))
        for _ in range(5):
            step()
        assert seen[0] == rid + [None] and seen[4] == [rid[0], None, rid[2], None]              # the live hole: slot 1 empty below slot 2
        assert bb["table"][1].tolist() == [1, 2, 0] + [-1] * (pps - 3)
        dec.prefill(_rows(150, dec.D, 99))                                             # someone else uses the single-sequence cache
        rid += [b.submit(s, max_new_tokens=n, prefix=h) for s, n in zip(suf[3:], N_NEW[3:])]
        while b.in_flight():
            step()
        assert [b.finished[r].tolist() for r in rid] == solo
        assert order == rid                                                            # FIFO
        if tail:                                                                       # request 3 (2 pages) waited with a slot free, 4 and 5 behind it
            assert seen[5] == [rid[0], None, rid[2], None]
        assert gathers == [(0, 128)] * dec.n_layers                                    # the prefix rows came back from the pages once
        assert max(len(o) for o in owners.values()) >= 2                               # a freed (dirty) own page served a later request
        assert not set(owners) & set(h.pages) and 0 not in owners
        assert pool.n_free == 3 and bb["table"][:4].tolist() == [[1, 2, 0] + [-1] * (pps - 3)] * 4
        with pytest.raises(ValueError, match="a prefix is open"):
            b.submit(plain, max_new_tokens=5)
        b.close_prefix()
        assert pool.n_free == 5 and bb["table"][:4].tolist() == [[0] + [-1] * (pps - 1)] * 4 and not h.open
        with pytest.raises(ValueError, match="closed"):
            b.submit(suf[0], max_new_tokens=2, prefix=h)
        r = b.submit(plain, max_new_tokens=5)                                          # a plain paged request decodes as before
        assert b.run()[r].tolist() == plain_solo and pool.n_free == 5
    finally:
        dec._bb_busy = None
        dec.enable_paged_kv(0, False)
        if fmt == "fp8":
            dec.enable_fp8_decode(False)


def test_five_graph_steps_across_an_own_page_boundary_equal_the_eager_steps(ops, small):
    """Request 0 holds 149 + 42 = 191 rows: its five steps write positions 191 .. 195, from its first own page into its second.  The
    replayed graph and the eager steps give the same tokens, logits and pages."""
    from videollama2_amd.serving import ContinuousBatcher
    dec = small
    x_prefix, suf = _rows(149, dec.D, 51), [_rows(42, dec.D, 71), _rows(3, dec.D, 72)]
    dec.enable_paged_kv(8)
    try:
        runs = []
        for use_graph in (True, False):
            b = ContinuousBatcher(dec, max_slots=2, use_graph=use_graph)
            h = b.open_prefix(x_prefix)
            bb = dec._bb
            rid = [b.submit(s, max_new_tokens=5, prefix=h) for s in suf]
            toks, logits = [], []
            for _ in range(5):
                toks.append(b.step())
                torch.cuda.synchronize()
                logits.append(bb["logits"][:2].clone())
            assert not b.in_flight() and bb["pos"][:2].tolist() == [196, 157]
            pages = h.pages + [3, 4, 5]                                                # request 0: pages 3 and 4 (rows 128 .. 195), request 1: page 5
            runs.append((toks, torch.stack(logits), [t[pages].clone() for t in bb["kpool"] + bb["vpool"]], [b.finished[r].tolist() for r in rid]))
            b.close_prefix()
        (t0, l0, p0, f0), (t1, l1, p1, f1) = runs
        assert t0 == t1 and f0 == f1 and torch.equal(l0, l1)
        assert all(same_bits(a, c) for a, c in zip(p0, p1))
    finally:
        dec._bb_busy = None
        dec.enable_paged_kv(0, False)


def test_a_sampled_request_repeats_under_its_seed_and_graph_equals_eager(ops, small):
    from videollama2_amd.serving import ContinuousBatcher
    dec = small
    x_prefix, suf = _rows(149, dec.D, 52), [_rows(7, dec.D, 81), _rows(20, dec.D, 82)]
    dec.enable_paged_kv(8)
    try:
        runs = []
        for seed, use_graph in ((3, True), (3, False), (3, True), (4, True)):
            b = ContinuousBatcher(dec, max_slots=2, use_graph=use_graph)
            h = b.open_prefix(x_prefix)
            gen = torch.Generator(device=DEV).manual_seed(seed)
            r0 = b.submit(suf[0], max_new_tokens=8, prefix=h, do_sample=True, temperature=0.9, top_k=20, top_p=0.95, generator=gen)
            r1 = b.submit(suf[1], max_new_tokens=8, prefix=h)                          # a greedy request beside it
            done = b.run()
            runs.append((done[r0].tolist(), done[r1].tolist()))
            b.close_prefix()
        assert runs[1] == runs[0] and runs[2] == runs[0]
        assert runs[3][1] == runs[0][1]                                                # the greedy neighbour does not depend on the seed
        greedy = _solo_after(dec, x_prefix, suf[:1], (8,))
        assert runs[0][0] != greedy[0] or runs[3][0] != runs[0][0]                      # the draws are draws, not the argmax
    finally:
        dec._bb_busy = None
        dec.enable_paged_kv(0, False)


def _solo_after(dec, x_prefix, suffixes, n_new):
    dec._bb_busy = None
    dec.enable_paged_kv(0, False)
    return _solo(dec, x_prefix, suffixes, n_new)


def test_model_batcher_one_video_three_questions_over_time(ops, golden_small):
    """open_video encodes once; three questions submitted at different steps give the tokens the inner batcher gives on the same embeddings."""
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.serving import ContinuousBatcher
    g = golden_small
    cfg = g["cfg"]
    model = VideoLLaMA2Hip(cfg, O.seeded_state_dict(cfg, g["seed"], round_bf16=True), "cuda:0", max_seq_len=256)
    gen = torch.Generator().manual_seed(5)
    rnd = lambda n: torch.randint(3, cfg["llm"]["vocab_size"], (n,), generator=gen)
    prefix_ids = torch.cat([g["input_ids"], rnd(30)])                                  # 44 + 30 = 74 rows: one shared page, a tail of 10
    questions = [torch.cat([prefix_ids, rnd(n)]) for n in (1, 5, 17)]
    frames = g["frames"].to("cuda:0")
    model.enable_paged_kv(6)
    try:
        seen = []
        hook = model.vision_tower.register_forward_pre_hook(lambda m, a: seen.append(a[0].shape[0]))
        try:
            mb = model.batcher(max_slots=4)
            h = mb.open_video(prefix_ids, [(frames, "video")])
            assert (h.P, h.shared_rows, len(h.pages)) == (74, 64, 1)
            rid = [mb.submit(questions[0], prefix=h, max_new_tokens=6)]
            mb.step(); mb.step()
            rid.append(mb.submit(questions[1][None], prefix=h, max_new_tokens=6))
            mb.step()
            rid.append(mb.submit(questions[2], prefix=h, max_new_tokens=6))
            done = mb.run()
            assert seen == [frames.shape[0]], seen
        finally:
            hook.remove()
        got = [done[r].tolist() for r in rid]
        with pytest.raises(ValueError, match="begin with the open prefix"):
            mb.submit(torch.cat([rnd(3), questions[0]]), prefix=h)
        with pytest.raises(ValueError, match="no media of its own"):
            mb.submit(torch.cat([prefix_ids, g["input_ids"]]), prefix=h)
        mb.close_video()
        assert model.decoder._bb["pool"].n_free == 5
        # the inner batcher on the same embeddings
        feats = model.encode_images_or_videos([(frames, "video")])
        x_prefix = model._embed_suffix(prefix_ids.tolist(), [feats[0]], 0)
        assert x_prefix.shape[0] == 74
        b = ContinuousBatcher(model.decoder, max_slots=4)
        hb = b.open_prefix(x_prefix)
        want = []
        for q in questions:
            emb = torch.empty((q.numel() - prefix_ids.numel(), model.decoder.D), dtype=torch.bfloat16, device="cuda:0")
            model._embed_ids(q[prefix_ids.numel():].to("cuda:0"), emb)
            want.append(b.submit(emb, max_new_tokens=6, prefix=hb))
        done = b.run()
        assert got == [done[r].tolist() for r in want]
        b.close_prefix()
    finally:
        model.decoder._bb_busy = None
        model.enable_paged_kv(0, False)
        del model
        gc.collect()
        torch.cuda.empty_cache()
