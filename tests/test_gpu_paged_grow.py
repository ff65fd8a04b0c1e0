"""Growing reservations page by page and preemption by swap on MI355X (include/vl2hip.h vl2_kv_pages_move, csrc/k_kv_swap.h,
ContinuousBatcher(reserve="grow")).  A swap moves bytes and growth moves nothing, so EVERY comparison here is
torch.equal (on the storage bits where NaN poison is involved): there is no tolerance in this file.  The kernel at nkv = 2 on a 12-page pool,
both builds and all three pool kinds; the batcher on the two small golden decoders (max_seq_len 256 and 200): growth across the 64 and 128
edges, the occupancy a 5-page pool reaches, preemption and resume on 16-bit and fp8 pages against the solo decodes, ModelBatcher.  The lengths
of the occupancy and the preemption case were chosen on the CPU simulation (tests/paged_grow_sim.py; tests/test_paged_grow_host.py asserts
what they need there).  Every test needs the new entry point or the new policy: none passes without them."""
import gc

import pytest
import torch

from oracle import vl2_oracle as O
from videollama2_amd.paging import pages_for, pages_needed, rows_next

pytestmark = pytest.mark.gpu
DEV = "cuda"
NKV, HD, SMAX = 2, 128, 256
PPS = SMAX // 64
SCALE = HD ** -0.5
N_PAGES = 12

# (prompt rows, max_new_tokens, tokens really emitted)
GROWTH = [(70, 70, 70), (129, 8, 8), (65, 64, 64), (5, 130, 130)]                   # cross the 64 and the 128 edge in flight
OCCUPANCY = dict(n_pages=5, requests=[(5, 130, 12), (20, 120, 12), (33, 100, 12), (50, 80, 12)])   # whole: 3 pages each; they stop after 12 tokens
PREEMPT = dict(n_pages=6, max_slots=4, requests=[(60, 12, 12), (61, 10, 10), (62, 9, 9), (125, 8, 8)], sampled=2)


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


def raw(t):
    return t.contiguous().view(torch.uint8)


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(raw(a), raw(b))


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
def _pool(kind, elem, n, seed):
    """A pool or arena of `n` pages of one of the three kinds, every byte random (seeded)."""
    dtype, tail = {"rows16": (elem, (64, HD)), "codes": (torch.uint8, (64, HD)), "scales": (torch.float32, (64,))}[kind]
    t = torch.empty((n, NKV) + tail, dtype=dtype)
    raw(t).copy_(torch.randint(0, 256, raw(t).shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)))
    return t.to(DEV)


@pytest.mark.parametrize("kind", ["rows16", "codes", "scales"])
def test_pages_move_copies_the_named_pages_byte_for_byte_and_nothing_else(ops, elem, kind):
    from videollama2_amd import _lib
    pool = _pool(kind, elem, N_PAGES, 1)
    pool0 = pool.clone()
    sentinel = _pool(kind, elem, 8, 2)
    # gather: shuffled ids with -1, 0 (the parking page) and 12 (past the pool) among them; slot 7 is behind the list
    ids = [7, -1, 3, 0, 11, 12, 1]
    arena = sentinel.clone()
    ops.kv_pages_move(pool, arena, torch.tensor(ids, dtype=torch.int32, device=DEV), True)
    torch.cuda.synchronize()
    assert same_bytes(pool, pool0)
    for i, pg in enumerate(ids):
        assert same_bytes(arena[i], pool0[pg] if 1 <= pg < N_PAGES else sentinel[i]), (i, pg)
    assert same_bytes(arena[7], sentinel[7])
    # scatter to other ids: exactly those pages, from their slots
    to = [2, 12, 9, -1, 5, 0, 4]
    exp = pool0.clone()
    for i, pg in enumerate(to):
        if 1 <= pg < N_PAGES:
            exp[pg] = arena[i]
    arena0 = arena.clone()
    ops.kv_pages_move(pool, arena, torch.tensor(to, dtype=torch.int32, device=DEV), False)
    torch.cuda.synchronize()
    assert same_bytes(pool, exp) and same_bytes(arena, arena0)
    assert same_bytes(pool[2], pool0[7]) and same_bytes(pool[9], pool0[3]) and same_bytes(pool[5], pool0[11]) and same_bytes(pool[4], pool0[1])
    assert same_bytes(pool[0], pool0[0])
    # n = 0 touches nothing: through the wrapper, and through the library itself with live pointers
    some = torch.tensor(to, dtype=torch.int32, device=DEV)
    for to_arena in (True, False):
        ops.kv_pages_move(pool, arena, some[:0], to_arena)
        _lib.call("vl2_kv_pages_move", pool.data_ptr(), arena.data_ptr(), some.data_ptr(), 0, N_PAGES, pool.stride(0) * pool.element_size(),
                  int(to_arena), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert same_bytes(pool, exp) and same_bytes(arena, arena0)
    # one page, and a whole table row of pages with a repeated skip
    one = sentinel.clone()
    ops.kv_pages_move(pool, one, torch.tensor([11], dtype=torch.int32, device=DEV), True)
    torch.cuda.synchronize()
    assert same_bytes(one[0], exp[11]) and same_bytes(one[1:], sentinel[1:])


def _tables(rows=SMAX):
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.int64).float() / HD))
    fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().contiguous().to(DEV), fr.sin().contiguous().to(DEV)


def test_attention_on_moved_pages_gives_the_bits_of_the_unmoved_ones(ops, elem):
    """Three requests at positions 65, 130 and 20; request 1's three pages are gathered and scattered to three other ids (its old pages
    poisoned), its table row rewritten: the step's outputs, partials and appended rows are those of the unmoved pool."""
    nh, positions = NKV * 4, (65, 130, 20)
    B = len(positions)
    g = torch.Generator().manual_seed(3)
    qkv = (torch.randn((B, (nh + 2 * NKV) * HD), generator=g) * 1.5).to(elem).to(DEV)
    rows = [[5, 2, -1, -1], [4, 9, 1, -1], [7, -1, -1, -1]]
    moved = [[5, 2, -1, -1], [10, 3, 8, -1], [7, -1, -1, -1]]
    kpool = torch.full((N_PAGES, NKV, 64, HD), float("nan"), dtype=elem, device=DEV)
    vpool = kpool.clone()
    for b, pos in enumerate(positions):
        for j in range(pos // 64 + 1):
            n = min(64, pos - 64 * j)
            kpool[rows[b][j], :, :n] = torch.randn(NKV, n, HD, generator=g).to(elem).to(DEV)
            vpool[rows[b][j], :, :n] = torch.randn(NKV, n, HD, generator=g).to(elem).to(DEV)
    cos, sin = _tables()
    pos = torch.tensor(positions, dtype=torch.int32, device=DEV)
    run = lambda kp, vp, table, partial, out: ops.attn_decode_paged(qkv, kp, vp, torch.tensor(table, dtype=torch.int32, device=DEV), cos, sin,
                                                                    partial, out, nh, NKV, pos, SMAX, SCALE)
    nan_partial = lambda: torch.full((B * nh * PPS * 130,), float("nan"), dtype=torch.float32, device=DEV)
    k0, v0, p0, o0 = kpool.clone(), vpool.clone(), nan_partial(), torch.zeros((B, nh * HD), dtype=elem, device=DEV)
    run(k0, v0, rows, p0, o0)
    arena = torch.empty((PPS, NKV, 64, HD), dtype=elem, device=DEV)
    src, dst = (torch.tensor(r[1][:3], dtype=torch.int32, device=DEV) for r in (rows, moved))
    for pool in (kpool, vpool):
        ops.kv_pages_move(pool, arena, src, True)
        ops.kv_pages_move(pool, arena, dst, False)
        pool[rows[1][:3]] = float("nan")                                # nothing may be read from where the pages were
    p1, o1 = nan_partial(), torch.zeros((B, nh * HD), dtype=elem, device=DEV)
    run(kpool, vpool, moved, p1, o1)
    torch.cuda.synchronize()
    assert not bool(o0.isnan().any()) and torch.equal(o1, o0) and same_bytes(p1, p0)
    for old, new in zip(rows[1][:3], moved[1][:3]):
        assert same_bytes(kpool[new], k0[old]) and same_bytes(vpool[new], v0[old])        # the appended row 130 included
    assert not bool(kpool[moved[1][2], :, 2].isnan().any()) and bool(kpool[moved[1][2], :, 3:].isnan().all())


# ---------------------------------------------------------------------------------------------------------------- the decoders
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


class Small:
    """One small golden decoder with its prompts and the solo decodes the tests share (computed once, on first use, never changed)."""

    def __init__(self, golden, max_seq_len):
        from videollama2_amd.decoder import HipMistralDecoder
        cfg = golden["cfg"]
        assert cfg["llm"]["head_dim"] == 128
        self.dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, golden["seed"], only=_keep), DEV, max_seq_len=max_seq_len)
        self._x, self._solo = {}, {}

    def x(self, S):
        if S not in self._x:
            g = torch.Generator().manual_seed(1000 + S)
            self._x[S] = (torch.randn(S, self.dec.D, generator=g) * 0.5).bfloat16().to(DEV)
        return self._x[S]

    def solo(self, S, budget, stop=None, seed=None):
        """The tokens of the request alone on the contiguous single-sequence cache (a sampled one: (0.8, 20, 0.9) under `seed`)."""
        key = (S, budget, stop, seed)
        if key not in self._solo:
            assert not self.dec.paged_kv and not self.dec.fp8_kv
            kw = dict(stopping_criteria=stop_after(stop)) if stop is not None and stop < budget else {}
            if seed is not None:
                kw["sampler"] = (0.8, 20, 0.9, torch.Generator(device=DEV).manual_seed(seed))
            self._solo[key] = self.dec.generate(self.x(S), max_new_tokens=budget, use_graph=True, **kw)[0].tolist()
        return self._solo[key]


def stop_after(n):
    return lambda ids, _: ids.shape[1] >= n


def submit_kw(budget, stop, seed=None):
    kw = dict(max_new_tokens=budget)
    if stop is not None and stop < budget:
        kw["stopping_criteria"] = stop_after(stop)
    if seed is not None:
        kw.update(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, generator=torch.Generator(device=DEV).manual_seed(seed))
    return kw


@pytest.fixture(scope="module", params=["mistral", "v21"])
def small(request, ops, golden_small, golden_small_v21):
    # max_seq_len 200 (v21): no multiple of the page, so the table covers 256 positions
    s = Small(golden_small if request.param == "mistral" else golden_small_v21, 256 if request.param == "mistral" else 200)
    yield s
    s.dec._bb_busy = None
    del s
    gc.collect()
    torch.cuda.empty_cache()


def drain(b, check=None):
    """Step b until it is empty.  Returns one record per step, taken when the step's kernels are issued: {request id: its page ids}."""
    dec, trace = b.dec, []
    snap = lambda: trace.append({r.rid: list(r.pages) for r in b.slots if r is not None})
    step, capture = dec._batched_step, dec.capture_batch_graph

    def eager(*a, **k):
        if not b.use_graph:
            snap()
        return step(*a, **k)

    def graph(*a, **k):
        snap()
        return capture(*a, **k)
    dec._batched_step, dec.capture_batch_graph = eager, graph
    try:
        while b.in_flight():
            before = b.preemptions
            flying = {r.rid: r for r in b.slots if r is not None}
            b.step()
            if check is not None:
                check(b, flying, before)
    finally:
        del dec._batched_step, dec.capture_batch_graph
    assert len(trace) == b.steps
    return trace


def all_parked(dec, n_usable, max_slots):
    bb = dec._bb
    return bb["pool"].n_free == n_usable and bb["table"][:max_slots].tolist() == [[0] + [-1] * (bb["pages_per_seq"] - 1)] * max_slots


# ---------------------------------------------------------------------------------------------------------------- 2. growth
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_growth_across_page_edges_with_a_roomy_pool(small, use_graph):
    from videollama2_amd.serving import ContinuousBatcher
    dec = small.dec
    solo = [small.solo(S, budget) for S, budget, _ in GROWTH]
    assert [len(t) for t in solo] == [n for _, _, n in GROWTH]
    whole_pages = [pages_needed(S, budget, dec.max_seq_len) for S, budget, _ in GROWTH]
    assert whole_pages == [3, 3, 3, 3]
    dec.enable_paged_kv(sum(whole_pages) + 1)
    try:
        runs = {}
        for reserve in ("whole", "grow"):
            b = ContinuousBatcher(dec, max_slots=4, use_graph=use_graph, reserve=reserve)
            rid = [b.submit(small.x(S), **submit_kw(budget, None)) for S, budget, _ in GROWTH]
            by_rid = {r.rid: r for r in b.waiting}
            graphs_before = len(dec.__dict__.get("_batch_graphs", {}))
            trace = drain(b)
            runs[reserve] = [b.finished[r].tolist() for r in rid]
            assert all_parked(dec, sum(whole_pages), 4) and b.preemptions == 0 and b.resumes == 0
            if reserve == "whole":
                assert all(len(pg) == whole_pages[r] for rec in trace for r, pg in rec.items())
                continue
            # at every step each request holds exactly the pages of the rows that exist, its next row included
            emitted = {r: 0 for r in rid}
            sizes = {r: set() for r in rid}
            for rec in trace:
                for r, pg in rec.items():
                    assert len(pg) == pages_for(rows_next(by_rid[r].S, emitted[r], dec.max_seq_len)), (r, emitted[r], pg)
                    assert len(set(pg)) == len(pg) and 0 not in pg
                    sizes[r].add(len(pg))
                    emitted[r] += 1
                assert len({p for pg in rec.values() for p in pg}) == sum(len(pg) for pg in rec.values())      # nobody shares a page
            assert [sorted(sizes[r]) for r in rid] == [[2, 3], [3], [2, 3], [1, 2, 3]]         # 70 -> 140, 129 -> 137, 65 -> 129, 5 -> 135 rows
            # the step graphs: one per occupancy, however many page edges were crossed
            if use_graph:
                keys = set(dec._batch_graphs)
                assert keys <= {(nb, False) for nb in (1, 2, 3, 4)} and len(keys) >= graphs_before
        assert runs["grow"] == runs["whole"] == solo
    finally:
        dec.enable_paged_kv(0, False)


# ---------------------------------------------------------------------------------------------------------------- 3. occupancy
def test_a_five_page_pool_holds_four_growing_requests_where_whole_reservations_hold_one(small):
    from videollama2_amd.serving import ContinuousBatcher
    dec = small.dec
    reqs = OCCUPANCY["requests"]
    assert all(pages_needed(S, budget, dec.max_seq_len) == 3 for S, budget, _ in reqs)
    solo = [small.solo(S, budget, stop) for S, budget, stop in reqs]
    dec.enable_paged_kv(OCCUPANCY["n_pages"])
    try:
        out = {}
        for reserve in ("whole", "grow"):
            b = ContinuousBatcher(dec, max_slots=4, use_graph=True, reserve=reserve)
            rid = [b.submit(small.x(S), **submit_kw(budget, stop)) for S, budget, stop in reqs]
            trace = drain(b)
            out[reserve] = ([b.finished[r].tolist() for r in rid], [len(rec) for rec in trace], b.steps)
            assert all_parked(dec, 4, 4) and b.preemptions == 0
        assert max(out["whole"][1]) == 1 and out["whole"][2] == 48
        assert out["grow"][1][0] == 4 and out["grow"][2] == 12 < out["whole"][2]
        assert out["grow"][0] == out["whole"][0] == solo
    finally:
        dec.enable_paged_kv(0, False)


# ---------------------------------------------------------------------------------------------------------------- 4. preemption
@pytest.mark.parametrize("pages", ["16bit", "fp8"])
def test_preempted_requests_resume_elsewhere_with_the_tokens_of_their_solo_decode(small, pages):
    from tests.paged_grow_sim import simulate
    from videollama2_amd.serving import ContinuousBatcher
    dec = small.dec
    reqs, n_pages, max_slots, sampled = PREEMPT["requests"], PREEMPT["n_pages"], PREEMPT["max_slots"], PREEMPT["sampled"]
    seeds = [100 + i if i == sampled else None for i in range(len(reqs))]
    plan = simulate(reqs, n_pages, max_slots, dec.max_seq_len)
    assert plan["preemptions"] >= 1
    if pages == "16bit":
        ref = [small.solo(S, budget, None, seed) for (S, budget, _), seed in zip(reqs, seeds)]
    else:                                         # the contiguous fp8-KV slots, every request alone in its batcher
        dec.enable_fp8_kv()
        try:
            ref = []
            for (S, budget, _), seed in zip(reqs, seeds):
                b = ContinuousBatcher(dec, max_slots=max_slots, use_graph=True)
                rid = b.submit(small.x(S), **submit_kw(budget, None, seed))
                ref.append(b.run()[rid].tolist())
        finally:
            dec.enable_fp8_kv(False)
    assert [len(t) for t in ref] == [n for _, _, n in reqs]
    dec.enable_paged_kv(n_pages, fp8=pages == "fp8")
    try:
        for use_graph in (True, False):
            b = ContinuousBatcher(dec, max_slots=max_slots, use_graph=use_graph, reserve="grow")
            rid = [b.submit(small.x(S), **submit_kw(budget, None, seed)) for (S, budget, _), seed in zip(reqs, seeds)]
            victims, homes = [], {}

            def check(b, flying, before):
                for r in b.slots:
                    if r is not None:
                        homes.setdefault(r.rid, []).append((r.slot, tuple(r.pages)))
                if b.preemptions > before:
                    out = [r for r in flying.values() if r.swap is not None]
                    assert len(out) == b.preemptions - before
                    left = [r.order for r in flying.values() if r.swap is None]
                    assert all(v.order > max(left) for v in out)                       # the newest admitted, and only they
                    assert all(t.dtype == p.dtype and t.is_pinned() for v in out for t, p in zip(v.swap[0], b._pools_of(0)))
                    victims.extend(v.rid for v in out)
                assert b.in_flight() == sum(r is not None for r in b.slots) + len(b.waiting) + len(b.swapped)
            trace = drain(b, check)
            assert [b.finished[r].tolist() for r in rid] == ref, (pages, use_graph)
            assert b.preemptions == plan["preemptions"] >= 1 and b.resumes == b.preemptions and b.steps == plan["steps"]
            assert victims == plan["victims"] and [len(rec) for rec in trace] == plan["in_flight"]
            assert [{r: len(pg) for r, pg in rec.items()} for rec in trace] == plan["held"]
            # a resumed request came back on other page ids (and kept the count): its first pages changed under it
            moved = [v for v in set(victims) if any(a[1][:len(c[1])] != c[1][:len(a[1])] for a, c in zip(homes[v], homes[v][1:]))]
            assert moved, homes
            assert all(r.swap is None for r in b.slots if r is not None) and len(b.swapped) == 0
            assert all_parked(dec, n_pages - 1, max_slots)
    finally:
        dec.enable_paged_kv(0, False)


# ---------------------------------------------------------------------------------------------------------------- 5. ModelBatcher
def test_model_batcher_grows_like_it_reserves(ops, golden_small):
    from videollama2_amd.model import VideoLLaMA2Hip
    cfg = golden_small["cfg"]
    model = VideoLLaMA2Hip(cfg, O.seeded_state_dict(cfg, golden_small["seed"], round_bf16=True), "cuda:0", max_seq_len=128)
    g = torch.Generator().manual_seed(5)
    rows = [torch.randint(3, cfg["llm"]["vocab_size"], (n,), generator=g) for n in (11, 62, 6)]     # 62 + 5 tokens cross the 64 edge
    model.enable_paged_kv(4)
    out = {}
    for reserve in ("whole", "grow"):
        mb = model.batcher(max_slots=2, reserve=reserve)
        assert mb.inner.reserve == reserve
        rid = [mb.submit(r[None], max_new_tokens=5) for r in rows]
        trace = drain(mb.inner)
        out[reserve] = [mb.finished[r].tolist() for r in rid]
        assert model.decoder._bb["pool"].n_free == 3
        if reserve == "grow":
            assert sorted({len(pg) for rec in trace for r, pg in rec.items() if r == rid[1]}) == [1, 2]
    assert out["grow"] == out["whole"]
    model.enable_paged_kv(0, False)
    assert out["whole"] == [model.generate(r[None], max_new_tokens=5)[0].tolist() for r in rows]
    model.decoder._bb_busy = None
    del model, mb
    gc.collect()
    torch.cuda.empty_cache()
