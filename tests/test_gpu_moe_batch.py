"""Batched and continuous decoding on the Mixtral decoder (enable_moe_batch): the compact routing tables, the grouped
skinny-M GEMM row by row against the dense skinny-M GEMM, the three regimes of the batched MoE block, batched prefill, the batcher and the
model-level calls.  Small Mixtral config (D 256, I 512, 8 experts, top 2, 2 layers, head_dim 128) unless noted."""
import os

import pytest
import torch

from tests import moe_oracle as MO
from tests.util import rel, token_tie_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, I, E, K2 = 256, 512, 8, 2


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def _el(t):
    from videollama2_amd import _lib
    return t.to(device=DEV, dtype=_lib.elem_dtype()).contiguous()


def _tables(ids, n_exp):
    """The compact routing tables (row tile 1) restated on the host from expert ids [S, k]: ascending token order inside an expert."""
    S, k = ids.shape
    ids = ids.cpu().long()
    counts = torch.stack([(ids == e).any(1).sum() for e in range(n_exp)]).int()
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), counts.long().cumsum(0)]).int()
    gather = torch.full((S * k,), -1, dtype=torch.int32)
    inv = torch.empty((S, k), dtype=torch.int32)
    for e in range(n_exp):
        tok, slot = torch.where(ids == e)
        rows = offs[e] + torch.arange(tok.numel())
        gather[rows] = tok.int()
        inv[tok, slot] = rows.int()
    assert int(offs[n_exp]) == S * k and (gather >= 0).all()
    return counts, offs, gather, inv


def _route_rows(x, wr, k):
    from videollama2_amd import ops
    S, n_exp = x.shape[0], wr.shape[0]
    i32 = dict(dtype=torch.int32, device=DEV)
    ids, wts = torch.full((S, k), -7, **i32), torch.zeros((S, k), dtype=torch.float32, device=DEV)
    t = dict(counts=torch.full((n_exp,), -7, **i32), offs=torch.full((n_exp + 1,), -7, **i32), gather=torch.full((S * k,), -7, **i32),
             inv=torch.full((S, k), -7, **i32))
    ops.moe_route_rows(x, wr, k, 1e-5, ids, wts, tables=t)
    torch.cuda.synchronize()
    return ids, wts, t


# ---------------------------------------------------------------------------------------------------------------- G1: the tables
@pytest.mark.parametrize("S", [1, 5, 17, 64])
def test_compact_route_tables(S):
    torch.manual_seed(S)
    x = _el(torch.randn(S, D))
    wr = _el(torch.randn(E, D) * D ** -0.5 * 4).float()
    ids, wts, t = _route_rows(x, wr, K2)
    h = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)
    rid, rw, probs = MO.route(h, wr, K2)
    ok = MO.margins(probs, K2) > 1e-3
    assert torch.equal(ids.long()[ok], rid[ok]) and (wts[ok] - rw[ok]).abs().max().item() <= 1e-5
    counts, offs, gather, inv = _tables(ids, E)
    assert torch.equal(t["counts"].cpu(), counts) and torch.equal(t["offs"].cpu(), offs) and int(t["offs"][E]) == S * K2
    assert torch.equal(t["gather"].cpu(), gather) and torch.equal(t["inv"].cpu(), inv)


def test_compact_route_tables_all_tokens_on_two_experts():
    torch.manual_seed(3)
    S = 64
    x = _el(torch.rand(S, D) + 0.1)
    wr = torch.full((E, D), -0.01)
    wr[0], wr[1] = 0.02, 0.015
    ids, wts, t = _route_rows(x, _el(wr).float(), K2)
    assert (ids[:, 0] == 0).all() and (ids[:, 1] == 1).all()
    assert t["counts"].cpu().tolist() == [S, S] + [0] * 6 and t["offs"].cpu().tolist() == [0, S] + [2 * S] * 7
    counts, offs, gather, inv = _tables(ids, E)
    assert torch.equal(t["gather"].cpu(), gather) and torch.equal(t["inv"].cpu(), inv)


# ---------------------------------------------------------------------------------------------------------------- G2: grouped == dense, row by row
def _ids_from_counts(counts, nb):
    """Expert ids [nb, 2] with the given per-expert counts (each <= nb, sum 2 * nb): token t takes entries t and t + nb of the sorted expert
    list, which differ because no expert has more than nb entries."""
    slots = [e for e, c in enumerate(counts) for _ in range(c)]
    assert len(slots) == 2 * nb and max(counts) <= nb
    return torch.tensor([[slots[t], slots[t + nb]] for t in range(nb)], dtype=torch.int32)


CASES = {                                                   # per-expert counts: 0, 1, 16, 17, 33 and 64 all occur
    "two_of_eight": (64, [64, 64, 0, 0, 0, 0, 0, 0]),
    "ragged": (64, [33, 17, 16, 1, 0, 30, 20, 11]),
    "five": (5, [5, 1, 0, 2, 2, 0, 0, 0]),
    "seventeen": (17, [17, 16, 1, 0, 0, 0, 0, 0]),
}
POISON = 12288.0                                            # (exact in bf16 and fp16)


def _grouped_vs_dense(nb, counts, N_gu, K_gu, N_dn, K_dn, shrink=None, split=True):
    """Gate/up (+SwiGLU, rows gathered through the row map) and down on crafted tables against ops.gemm_skinny on every single row.
    shrink = {expert: count}: the kernel is given smaller counts for those experts than their row ranges hold, so the rows left over are owned
    by nobody: their partial sums must keep the poison."""
    from videollama2_amd import ops
    ops.attach_workspace(DEV)
    torch.manual_seed(nb + N_gu)
    ids = _ids_from_counts(counts, nb)
    cnt, offs, gather, inv = _tables(ids, E)
    assert cnt.tolist() == counts
    cnt_k = cnt.clone()
    for e, c in (shrink or {}).items():
        cnt_k[e] = c
    R = 2 * nb
    owned = torch.zeros(R, dtype=torch.bool)
    for e in range(E):
        owned[int(offs[e]):int(offs[e]) + int(cnt_k[e])] = True
    t = dict(counts=cnt_k.to(DEV), offs=offs.to(DEV))
    h = _el(torch.randn(nb, K_gu))
    wgu = _el(torch.randn(E, N_gu, K_gu) * K_gu ** -0.5)
    wd = _el(torch.randn(E, N_dn, K_dn) * K_dn ** -0.5)
    a_in = _el(torch.randn(R, K_dn) * 0.5)
    tail = 64
    for (A, w, rowmap, sw, N, K) in ((h, wgu, gather.to(DEV), True, N_gu, K_gu), (a_in, wd, None, False, N_dn, K_dn)):
        need = ops.moe_skinny_part_bytes(nb, 2, N, K) // 4
        ks = need // (R * N)
        part = torch.full((need + tail,), POISON, dtype=torch.float32, device=DEV)
        ncol = N // 2 if sw else N
        out = _el(torch.full((R + 3, ncol), POISON))
        ops.moe_gemm_skinny(A, w, t, nb, 2, part, rowmap=rowmap, swiglu=sw, out=out)
        torch.cuda.synchronize()
        pv = part[:need].view(ks, R, N).cpu()
        assert (part[need:] == POISON).all() and (out[R:].float() == POISON).all()
        assert (pv[:, ~owned] == POISON).all(), "partial rows nobody owns were written"
        assert (pv[:, owned] != POISON).all() and torch.isfinite(pv[:, owned]).all(), "an owned partial row was not written"
        for p in torch.where(owned)[0].tolist():
            e = int(torch.searchsorted(offs[1:].contiguous(), torch.tensor(p), right=True))
            src = int(gather[p]) if rowmap is not None else p
            assert ids[int(gather[p])].tolist().count(e) == 1                      # (row p is a row of expert e)
            want = ops.gemm_skinny(A[src:src + 1], w[e], swiglu=sw)
            assert torch.equal(out[p:p + 1], want), (("gate/up" if sw else "down"), p, e)
        assert (ks > 1) == split, (N, K, ks)


@pytest.mark.parametrize("case", list(CASES))
def test_grouped_skinny_equals_dense_skinny_row_by_row(case):
    nb, counts = CASES[case]
    _grouped_vs_dense(nb, counts, 2 * I, D, D, I)                    # N 1024 / K 256 and N 256 / K 512: both plans split K


def test_grouped_skinny_leaves_the_neighbours_rows_alone():
    """Experts 0, 1 and 5 get smaller counts than their row ranges: rows offs[e] + count .. offs[e + 1] - 1 keep the poison in every K slice."""
    nb, counts = CASES["ragged"]
    _grouped_vs_dense(nb, counts, 2 * I, D, D, I, shrink={0: 30, 1: 16, 5: 0})


def test_grouped_skinny_without_a_k_split():
    """K = 1184 = 32 * 37: skinny_plan finds no split (ks = 1) and chunks the slice in 37 LDS chunks."""
    nb, counts = CASES["seventeen"]
    _grouped_vs_dense(nb, counts, 128, 1184, 128, 1184, split=False)


def test_grouped_skinny_on_the_fp16_build():
    from videollama2_amd import _lib
    _lib.set_elem("fp16")
    try:
        _grouped_vs_dense(*CASES["five"], 2 * I, D, D, I)
        _grouped_vs_dense(*CASES["ragged"], 2 * I, D, D, I)
    finally:
        _lib.set_elem("bf16")


# ---------------------------------------------------------------------------------------------------------------- decoders
def _decoder(seed=9, n_layers=2, max_seq_len=128, skinny_rows=None):
    """skinny_rows: MOE_SKINNY_ROWS of this decoder (None: the default dispatch; 64: the grouped skinny-M GEMM serves 5 .. 64 requests)."""
    from videollama2_amd.decoder import HipMixtralDecoder
    cfg = MO.small_mixtral_cfg(n_layers=n_layers)
    sd = MO.seeded_state_dict(cfg, seed=seed, router_scale=4.0)
    dec = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=max_seq_len).enable_moe_batch()
    if skinny_rows is not None:
        dec.MOE_SKINNY_ROWS = skinny_rows
    return cfg, sd, dec


def _prompts(lens, seed):
    g = torch.Generator().manual_seed(seed)
    return [(0.5 * torch.randn(n, D, generator=g)).bfloat16() for n in lens]


def _solo(dec, xs, n_new):
    return [dec.generate(x.to(DEV), max_new_tokens=n_new, return_logits=True) for x in xs]


# ---------------------------------------------------------------------------------------------------------------- G3: regime a == the solo step
@pytest.mark.parametrize("nb", [2, 4])
def test_few_requests_are_bit_for_bit_the_solo_step(nb):
    cfg, sd, dec = _decoder()
    assert nb < dec.MOE_GEMM_BATCH
    xs = _prompts((20, 1, 33, 7)[:nb], seed=nb)
    solo = _solo(dec, xs, 5)
    runs = {g: dec.generate_batch([x.to(DEV) for x in xs], max_new_tokens=5, return_logits=True, use_graph=g) for g in (False, True)}
    assert (nb, False) in dec._batch_graphs
    for g, (toks, logits) in runs.items():
        for b, (st, sl) in enumerate(solo):
            assert toks[b].tolist() == st[0].tolist(), (g, b)
            assert torch.equal(logits[:, b], sl), (g, b)


# ---------------------------------------------------------------------------------------------------------------- G4: regime b == its composition
@pytest.mark.parametrize("nb", [8, 64])
def test_grouped_block_equals_the_composition_of_existing_ops(nb):
    from videollama2_amd import ops
    from videollama2_amd.decoder import _Skinny
    cfg, sd, dec = _decoder(n_layers=1, skinny_rows=64)
    assert dec.MOE_GEMM_BATCH <= nb <= dec.MOE_SKINNY_ROWS
    dec._ensure_batch(nb)
    torch.manual_seed(nb)
    lw = dec.w["layers"][0]
    o, x = _el(0.5 * torch.randn(nb, dec.nh * dec.hd)), _el(0.5 * torch.randn(nb, D))
    x_in, x1 = x.clone(), torch.empty_like(x)
    dec._token_block(_Skinny(dec, "16bit", nb), 0, o, x, x1, None)
    torch.cuda.synchronize()
    ids, wts = dec.last_route["ids"].clone(), dec.last_route["wts"].clone()
    assert len(set(ids.flatten().tolist())) >= (2 if nb == 8 else 6)
    x1_ref = ops.gemm_skinny(o, lw["wo"], res=x_in)
    assert torch.equal(x1, x1_ref)
    h = ops.rmsnorm(x1_ref, dec.w["ones"], dec.eps)
    y = torch.empty((nb * K2, D), dtype=h.dtype, device=DEV)
    for t in range(nb):
        for j in range(K2):
            e = int(ids[t, j])
            a = ops.gemm_skinny(h[t:t + 1], lw["wgu"][e], swiglu=True)
            y[t * K2 + j:t * K2 + j + 1] = ops.gemm_skinny(a, lw["wd"][e])
    inv = torch.arange(nb * K2, dtype=torch.int32, device=DEV).view(nb, K2)
    want = ops.moe_combine(x1_ref, y, dict(inv=inv, wts=wts), dec.eps)
    assert torch.equal(x, want)


@pytest.mark.parametrize("nb", [8, 64])
def test_grouped_step_agrees_with_the_tiled_grouped_kernels_to_rounding(nb):
    """The whole step with MOE_SKINNY_ROWS = 0 (the prefill's grouped GEMM on the same rows) against the grouped skinny-M step."""
    cfg, sd, dec = _decoder(skinny_rows=64)
    xs = [x.to(DEV) for x in _prompts([1 + (7 * b) % 40 for b in range(nb)], seed=nb)]
    _, skinny = dec.generate_batch(xs, max_new_tokens=2, return_logits=True)
    dec.MOE_SKINNY_ROWS = 0
    dec._invalidate_graphs()
    _, tiled = dec.generate_batch(xs, max_new_tokens=2, return_logits=True)
    assert torch.equal(skinny[0], tiled[0])
    for b in range(nb):
        assert rel(skinny[1, b], tiled[1, b]) < 2e-2, b
    assert not torch.equal(skinny[1], tiled[1])                                 # (two different kernels ran)


# ---------------------------------------------------------------------------------------------------------------- G5: end to end to rounding
def _oracle_step_margins(sd, cfg, x, toks):
    """Teacher-forced fp32 oracle: entry s - 1 = the smallest top-k margin over the layers of the forward that turns toks[s - 1] into step s's logits."""
    rec, orig = [], MO.route

    def spy(h, wr, k):
        out = orig(h, wr, k)
        rec.append(MO.margins(out[2], k))
        return out
    MO.route = spy
    try:
        with torch.no_grad():
            _, caches = MO.mixtral_forward(sd, cfg, x)
            pos, res = x.shape[0], []
            for t in toks[:-1]:
                rec.clear()
                _, caches = MO.mixtral_forward(sd, cfg, sd["model.embed_tokens.weight"][t:t + 1], pos, caches)
                res.append(min(float(m.min()) for m in rec))
                pos += 1
    finally:
        MO.route = orig
    return res


def _compare_to_rounding(solo, outs, blogits, margins, min_pairs):
    """The dense decoders' bar (test_gpu_v21.test_batched_decode_gemm_path_matches_sequential_to_rounding) on the pairs (request, step >= 1) whose
    routing the fp32 oracle decides with margin >= 1e-2 up to that step and whose tokens so far agree.  Returns the number of pairs compared."""
    n = 0
    for b, (toks, logits) in enumerate(solo):
        assert torch.equal(blogits[0, b], logits[0]), b                       # step 0 is the prefill: identical
        for s in range(1, blogits.shape[0]):
            if outs[b][:s].tolist() != toks[0, :s].tolist() or margins[b][s - 1] < 1e-2:
                break
            n += 1
            r = rel(blogits[s, b], logits[s])
            print(f"request {b} step {s}: rel {r:.3e}, oracle routing margin {margins[b][s - 1]:.3e}")
            assert r < 2e-2, (b, s, r)
            if outs[b][s].item() != toks[0, s].item():
                ok, margin, dmax = token_tie_ok(blogits[s, b], logits[s])
                assert ok, (b, s, margin, dmax)
    assert all(m[0] >= 1e-2 for m in margins), "a request's first decode step is not decidable: choose another seed"
    assert n >= min_pairs, (n, min_pairs)
    return n


G5_LENS, G5_SEED, G5_NEW = (40, 1, 23, 5, 64, 17, 33, 9), 0, 4


@pytest.mark.parametrize("skinny_rows", [None, 64])
def test_eight_requests_match_solo_decoding_to_rounding(skinny_rows):
    """Seed and inputs checked on the CPU oracle beforehand: every request's step 1 and 21 of the 24 (request, step >= 1) pairs have every
    routing decision at margin >= 1e-2.  Both grouped forms: the default dispatch and the grouped skinny-M GEMM."""
    cfg, sd, dec = _decoder(seed=G5_SEED, skinny_rows=skinny_rows)
    xs = _prompts(G5_LENS, seed=G5_SEED)
    solo = _solo(dec, xs, G5_NEW)
    margins = [_oracle_step_margins(sd, cfg, x.float(), st[0].tolist()) for x, (st, _) in zip(xs, solo)]
    outs, blogits = dec.generate_batch([x.to(DEV) for x in xs], max_new_tokens=G5_NEW, return_logits=True)
    assert len(xs) >= dec.MOE_GEMM_BATCH
    n = _compare_to_rounding(solo, outs, blogits, margins, min_pairs=3 * len(xs) * (G5_NEW - 1) // 4)
    assert n >= len(xs)                                          # (every request was compared at step 1: its token 0 comes from equal logits)


# ---------------------------------------------------------------------------------------------------------------- G6: beyond 64 requests
def test_seventy_requests_run_the_sparse_block():
    cfg, sd, dec = _decoder(max_seq_len=64, skinny_rows=64)
    nb = 70
    assert nb > dec.MOE_SKINNY_ROWS
    xs = _prompts([1 + (5 * b) % 23 for b in range(nb)], seed=70)
    outs, blogits = dec.generate_batch([x.to(DEV) for x in xs], max_new_tokens=2, return_logits=True)
    assert torch.isfinite(blogits).all() and blogits.shape[:2] == (2, nb)
    for b in range(nb):
        assert torch.equal(blogits[0, b], dec.prefill(xs[b].to(DEV))), b
    for b in (0, 23, 64, 69):
        toks, logits = dec.generate(xs[b].to(DEV), max_new_tokens=2, return_logits=True)
        assert outs[b][0].item() == toks[0, 0].item()
        assert rel(blogits[1, b], logits[1]) < 2e-2, b
        if outs[b][1].item() != toks[0, 1].item():
            ok, margin, dmax = token_tie_ok(blogits[1, b], logits[1])
            assert ok, (b, margin, dmax)


# ---------------------------------------------------------------------------------------------------------------- G7: prefill_batch
def test_prefill_batch_is_the_prompts_one_by_one():
    cfg, sd, dec = _decoder()
    lens = (40, 1, 23, 5, 64)
    xs = [x.to(DEV) for x in _prompts(lens, seed=7)]
    bb = dec._ensure_batch(len(xs))
    caches = [([k[b] for k in bb["k"]], [v[b] for v in bb["v"]]) for b in range(len(xs))]
    dec.prefill_batch(xs, caches, bb["logits"][:len(xs)])
    torch.cuda.synchronize()
    for b, x in enumerate(xs):
        assert torch.equal(dec.prefill(x), bb["logits"][b]), b
        for li in range(dec.n_layers):
            assert torch.equal(dec.kcache[li][:, :lens[b]], bb["k"][li][b, :, :lens[b]]), (b, li)
            assert torch.equal(dec.vcache[li][:, :lens[b]], bb["v"][li][b, :, :lens[b]]), (b, li)
    one = torch.empty_like(bb["logits"][0])
    dec.prefill(xs[2], cache=caches[0], logits_out=one)                   # prefill(cache=...) is open with the switch
    assert torch.equal(one, bb["logits"][2])


# ---------------------------------------------------------------------------------------------------------------- G8: ContinuousBatcher
def test_continuous_batcher_four_slots_equals_solo():
    from videollama2_amd.serving import ContinuousBatcher
    cfg, sd, dec = _decoder()
    xs = [x.to(DEV) for x in _prompts((20, 1, 33, 7, 12, 3), seed=8)]
    n_new = [6, 2, 5, 4, 6, 3]
    solo = [dec.generate(x, max_new_tokens=n)[0].tolist() for x, n in zip(xs, n_new)]
    for use_graph in (True, False):
        b = ContinuousBatcher(dec, max_slots=4, use_graph=use_graph)
        sub = lambda i: b.submit(xs[i], max_new_tokens=n_new[i])
        rid = [sub(0), sub(1)]
        b.step()
        rid += [sub(2), sub(3)]
        b.step(); b.step()                                            # request 1 retires: a hole below slot 3
        rid += [sub(4), sub(5)]
        done = b.run()
        assert [done[r].tolist() for r in rid] == solo, use_graph
    b.submit(xs[0], max_new_tokens=3)
    b.step()
    with pytest.raises(RuntimeError, match="enable_moe_batch: a ContinuousBatcher holds requests in flight"):
        dec.enable_moe_batch(False)
    b.run()


@pytest.mark.parametrize("skinny_rows", [None, 64])
def test_continuous_batcher_eight_slots_matches_solo_to_rounding(skinny_rows):
    from videollama2_amd.serving import ContinuousBatcher
    cfg, sd, dec = _decoder(seed=G5_SEED, skinny_rows=skinny_rows)
    xs = _prompts(G5_LENS, seed=G5_SEED)
    solo = _solo(dec, xs, G5_NEW)
    margins = [_oracle_step_margins(sd, cfg, x.float(), st[0].tolist()) for x, (st, _) in zip(xs, solo)]
    b = ContinuousBatcher(dec, max_slots=8)
    rid = [b.submit(x.to(DEV), max_new_tokens=G5_NEW) for x in xs]
    V = dec.V
    blogits = torch.zeros((G5_NEW, len(xs), V), dtype=torch.float32, device=DEV)
    for bi, (_, sl) in enumerate(solo):
        blogits[0, bi] = sl[0]                                         # (the admission's prefill: checked against solo in G7; the batcher draws from it)
    for s in range(1, G5_NEW):                                         # after its s-th step a slot holds the logits step s + 1 draws from
        b.step()
        if s == 1:
            slots = {r.rid: sl for sl, r in enumerate(b.slots)}
        for bi, r in enumerate(rid):
            blogits[s, bi] = b.bb["logits"][slots[r]]
    done = b.run()
    outs = [done[r] for r in rid]
    assert all(o.numel() == G5_NEW for o in outs)
    _compare_to_rounding(solo, outs, blogits, margins, min_pairs=3 * len(xs) * (G5_NEW - 1) // 4)


def test_continuous_batcher_mixes_greedy_and_sampled_requests():
    """Six requests in eight slots admitted together: rows 1, 3, 4 sample; they equal generate_batch(sampler=...) rows given the same u."""
    from videollama2_amd.serving import ContinuousBatcher
    cfg, sd, dec = _decoder()
    xs = [x.to(DEV) for x in _prompts((20, 9, 33, 7, 12, 3), seed=18)]
    T, tk, tp, n_new = 1.1, 20, 0.9, 5
    ref, _ = dec.generate_batch(xs, max_new_tokens=n_new, return_logits=True, sampler=(T, tk, tp, torch.Generator(device=DEV).manual_seed(5)))
    g2 = torch.Generator(device=DEV).manual_seed(5)
    us = torch.stack([torch.rand((n_new + 1,), device=DEV, generator=g2) for _ in xs])
    greedy = dec.generate_batch(xs, max_new_tokens=n_new)
    sampled_rows = (1, 3, 4)
    b = ContinuousBatcher(dec, max_slots=8)
    rid = []
    for i, x in enumerate(xs):
        kw = dict(do_sample=True, temperature=T, top_k=tk, top_p=tp) if i in sampled_rows else {}
        rid.append(b.submit(x, max_new_tokens=n_new, **kw))
    for i in sampled_rows:                                             # the request's own uniform numbers <- row i of generate_batch's
        b.waiting[i].u = us[i, :n_new].clone()
    done = b.run()
    # a row's logits depend on the other rows only through the regime, which is the same here (6 rows, all admitted in the first step); the
    # routing of a row does not depend on the other rows, so sampled rows see generate_batch's logits and draw its tokens
    for i in range(len(xs)):
        want = ref[i] if i in sampled_rows else greedy[i]
        assert done[rid[i]].tolist() == want.tolist(), i


# ---------------------------------------------------------------------------------------------------------------- G9: model level
def test_model_generate_batch_on_the_golden_checkpoint(tmp_path):
    from tests.util import ToyTokenizer
    from videollama2_amd import api
    g = torch.load(os.path.join(os.path.dirname(__file__), "golden", "small_mixtral_T4.pt"), weights_only=False)
    MO.write_mixtral_checkpoint(tmp_path, g)
    model, _, _ = api.model_init(str(tmp_path), device=DEV, max_seq_len=192, tokenizer=ToyTokenizer(g["cfg"]["llm"]["vocab_size"]))
    ids = g["input_ids"].to(DEV)
    fr = [g["frames"].to(DEV), torch.flip(g["frames"], dims=[0]).contiguous().to(DEV)]
    reqs = [(ids, [(fr[0], "video")]), (torch.cat([ids[:3], ids[6:]]), [(fr[1], "video")]), (ids[:4], None)]
    n = len(g["new_tokens"])
    with pytest.raises(NotImplementedError, match="MoE \\(mixtral\\) decoder: batched decoding not built"):
        model.generate_batch(reqs, max_new_tokens=n)
    solo = [model.generate(i[None], attention_mask=torch.ones(1, i.numel(), dtype=torch.long, device=DEV), images=im, do_sample=False,
                           max_new_tokens=n)[0].tolist() for i, im in reqs]
    assert solo[0] == g["new_tokens"].tolist()
    assert model.enable_moe_batch() is model
    out = model.generate_batch(reqs, max_new_tokens=n)
    assert [o.tolist() for o in out] == solo
    b = model.batcher(max_slots=4)
    rid = [b.submit(i, im, max_new_tokens=n) for i, im in reqs]
    done = b.run()
    assert [done[r].tolist() for r in rid] == solo
    model.enable_moe_batch(False)
    with pytest.raises(NotImplementedError, match="MoE"):
        model.generate_batch(reqs, max_new_tokens=n)
