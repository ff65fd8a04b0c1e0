"""The tiled W4A16 grouped GEMM on the MXFP4 expert stacks (csrc/k_moe_gemm4.h, vl2_moe_gemm_mxfp4, enable_moe_mxfp4(tiled=True); DESIGN.md
section 22f) on the MI355X.  The kernel on tests/moe_gemm4_exact.py's table -- strided views of poisoned allocations, outputs in a sentinel
frame: plain outputs equal RNE(fp64) bit for bit, SwiGLU within moe_exact._check_rows's cap, and EVERY case of EVERY epilogue bit for bit
ops.moe_gemm on the dequantised stack E2M1 2^e (the kernel's contract: the same k order, the block scale inside the converted element) -- then
the same equality on randn inputs, where no order is hidden by exactness; a reduced table on the fp16 build; and the decoder with tiled=True:
graph = eager, 8 / 64 / 70 requests against the solo MXFP4 step, bit for bit the 16-bit tiled step of a decoder holding the dequantised
experts, the batcher, and tiled=False restoring the skinny form and the refusal.  Small Mixtral config (D 256, I 512, 8 experts, top 2, 2
layers).  The first exact case also settles where a 1-byte LDS-DMA piece lands (the scale image of the kernel's header).

Measured (bf16 build): SwiGLU of the table 19 of 3 753 600 outputs one step from RNE(fp64), largest share of a case 3.8e-5 (cap 1e-2); the
8 / 64 / 70-request comparisons against the solo MXFP4 step 4.6e-3 ... 8.0e-3 rel-L2 on 18, 18 and 25 pairs (bound 2e-2,
tests/test_gpu_moe_mxfp4.py's); the file runs in 9 s."""
import pytest
import torch

from tests import moe_exact as X
from tests import moe_gemm4_exact as M
from tests import moe_mxfp4_exact as X4
from tests import moe_oracle as MO
from tests import mxfp4_oracle as M4
from tests.test_gpu_moe_batch import _oracle_step_margins, _prompts, _solo
from tests.test_gpu_moe_mxfp4 import _compare_on_decidable_pairs

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, I, E, K2 = 256, 512, 8, 2


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib, ops as o
    _lib.load()
    o.attach_workspace(DEV)
    return o


def _report(errs, n):
    errs = [e for e in errs if e]
    assert not errs, f"{len(errs)} of {n} cases failed:\n" + "\n".join(errs[:12])


# ---------------------------------------------------------------------------------------------------------------- the kernel, exact inputs
def test_exact_table_sentinels_fp64_answer_and_the_16_bit_kernel_bit_for_bit(ops):
    cases = [M.Gemm4Case(r) for r in M.gemm4_table()]
    errs, nd, tot, worst = [], 0, 0, 0.0
    for c in cases:
        e, d = M.check_gemm4(c, *M.run_gemm4(ops, c, DEV))
        errs.append(e)
        if e is None and c.swiglu:
            nd, tot, worst = nd + d, tot + c.R * c.n_out, max(worst, d / max(1, c.R * c.n_out))
    print(f"\n  tiled W4A16 grouped GEMM SwiGLU: {nd} of {tot} outputs one step from RNE of the fp64 value; largest share of a case {worst:.2e}, cap 1.00e-02", end="")
    _report(errs, len(cases))


def test_reduced_table_on_the_fp16_build(ops):
    from videollama2_amd import _lib
    cases = [c for c in (M.Gemm4Case(r) for r in M.gemm4_table()) if M.fits_fp16(c)][::2]
    assert len(cases) >= 4 and {c.row.epi for c in cases} == set(X.MOE_EPIS)
    _lib.set_elem("fp16")
    try:
        _lib.load()
        errs = [M.check_gemm4(c, *M.run_gemm4(ops, c, DEV))[0] for c in cases]
    finally:
        _lib.set_elem("bf16")
    _report(errs, len(cases))


# ---------------------------------------------------------------------------------------------------------------- the kernel, randn inputs
def _route_from_counts(ops, counts):
    """The padded tables (row tile 128) of per-expert counts -> (route dict on the device, S, P, live rows)."""
    S = sum(counts) // K2
    P = ops.moe_rows(S, K2, len(counts))
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + (c + 127) // 128 * 128)
    live = torch.zeros(P, dtype=torch.bool)
    for e, c in enumerate(counts):
        live[offs[e]:offs[e] + c] = True
    route = dict(counts=torch.tensor(counts, dtype=torch.int32, device=DEV), offs=torch.tensor(offs, dtype=torch.int32, device=DEV))
    return route, S, P, live


@pytest.mark.parametrize("counts", [(33, 17, 16, 1, 0, 30, 20, 11), (64, 64, 0, 0, 0, 0, 0, 0)], ids=["ragged", "two_of_eight"])
def test_randn_inputs_equal_the_16_bit_kernel_on_the_dequantised_stack(ops, counts):
    """N = 256, K = 1088 (17 K-tiles), weights through ops.moe_quant_mxfp4, dequantised by tests/mxfp4_oracle.py: 1088 fp32 additions per
    output whose order nothing hides."""
    from videollama2_amd import _lib
    el = _lib.elem_dtype()
    N, K = 256, 1088
    g = torch.Generator().manual_seed(sum(counts) + counts[0])
    route, S, P, live = _route_from_counts(ops, list(counts))
    blk = torch.exp2(((torch.arange(N)[:, None] + 2 * torch.arange(K // 32)[None, :]) % 5).float()).repeat_interleave(32, 1)
    w = (torch.randn(E, N, K, generator=g) * 0.02 * blk[None]).to(DEV, el)
    q, s = ops.moe_quant_mxfp4(w)
    deq32 = torch.stack([M4.dequant(q[e], s[e]) for e in range(E)])
    deq = deq32.to(DEV, el)
    assert torch.equal(deq.float().cpu(), deq32)                                  # the element type holds E2M1 2^e exactly
    a = torch.randn(P, K, generator=g).to(DEV, el)
    rn = torch.stack([torch.zeros(P), 0.5 + torch.rand(P, generator=g)], 1).to(DEV)
    for kw in (dict(), dict(swiglu=True), dict(swiglu=True, row_norm=rn, eps=1e-5)):
        n_out = N // 2 if kw.get("swiglu") else N
        out4 = torch.full((P, n_out), X.SENTINEL, dtype=el, device=DEV)
        out16 = torch.full((P, n_out), X.SENTINEL, dtype=el, device=DEV)
        ops.moe_gemm_mxfp4(a, q, s, route, S, K2, out=out4, **kw)
        ops.moe_gemm(a, deq, route, S, K2, out=out16, **kw)
        assert torch.equal(out4, out16), kw
        assert bool((out4[~live.to(DEV)] == X.SENTINEL).all()) and bool(torch.isfinite(out4[live.to(DEV)].float()).all())
        assert not bool((out4[live.to(DEV)] == X.SENTINEL).all(1).any())


# ---------------------------------------------------------------------------------------------------------------- the decoder
FROM = 5                                  # MOE_MXFP4_TILED_FROM on the instance: every grouped size of these tests runs the tiled form
G5_LENS, G5_SEED, G5_NEW = (40, 1, 23, 5, 64, 17, 33, 9), 0, 4


def _decoder(seed=9, max_seq_len=128, tiled=True, mxfp4=True):
    from videollama2_amd.decoder import HipMixtralDecoder
    cfg = MO.small_mixtral_cfg(n_layers=2)
    sd = MO.seeded_state_dict(cfg, seed=seed, router_scale=4.0)
    dec = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=max_seq_len).enable_moe_batch()
    dec.MOE_MXFP4_TILED_FROM = FROM
    if mxfp4:
        dec.enable_moe_mxfp4(tiled=tiled)
        assert dec.moe_mxfp4 and dec.moe_mxfp4_tiled is tiled
    return cfg, sd, dec


def _spy(dec, monkeypatch):
    """Counts the grouped MXFP4 calls of the decoder's steps."""
    from videollama2_amd import decoder as dmod
    n = dict(tiled=0, skinny=0)
    t0, s0 = dmod.ops.moe_gemm_mxfp4, dmod.ops.moe_gemm_skinny_mxfp4
    monkeypatch.setattr(dmod.ops, "moe_gemm_mxfp4", lambda *a, **kw: (n.__setitem__("tiled", n["tiled"] + 1), t0(*a, **kw))[1])
    monkeypatch.setattr(dmod.ops, "moe_gemm_skinny_mxfp4", lambda *a, **kw: (n.__setitem__("skinny", n["skinny"] + 1), s0(*a, **kw))[1])
    return n


def test_graph_and_eager_agree_bit_for_bit(ops, monkeypatch):
    cfg, sd, dec = _decoder(seed=G5_SEED)
    n = _spy(dec, monkeypatch)
    xs = [x.to(DEV) for x in _prompts(G5_LENS, seed=G5_SEED)]
    runs = {g: dec.generate_batch(xs, max_new_tokens=G5_NEW, return_logits=True, use_graph=g) for g in (False, True)}
    assert (8, False) in dec._batch_graphs and n["tiled"] > 0 and n["skinny"] == 0
    assert [t.tolist() for t in runs[True][0]] == [t.tolist() for t in runs[False][0]] and torch.equal(runs[True][1], runs[False][1])


@pytest.mark.parametrize("nb", [8, 64, 70])
def test_8_64_and_70_requests_match_solo_mxfp4_to_summation_order(ops, monkeypatch, nb):
    """The tiled form against the solo MXFP4 step: the bound and the filter of tests/test_gpu_moe_mxfp4.py's same comparison -- 2e-2 rel-L2 on
    the logits of the (request, step) pairs whose routing the fp32 oracle on the dequantised experts decides with margin >= 1e-2, at least
    half of the checked pairs decidable (the forms differ by summation order only).  At 70 the requests past 64 join the checked ones."""
    cfg, sd, dec = _decoder(seed=X4.DEC_SEED)
    n = _spy(dec, monkeypatch)
    sd4 = X4.dequantised_state_dict(sd, cfg)
    ids = X4.DEC8_IDS if nb == 8 else tuple(range(nb))
    xs = [X4.dec_prompt(i) for i in ids]
    check = list(range(8)) if nb == 8 else list(X4.DEC64_CHECK) + list(range(64, nb))
    outs, blogits = dec.generate_batch([x.to(DEV) for x in xs], max_new_tokens=X4.DEC_NEW, return_logits=True)
    assert n["tiled"] > 0 and n["skinny"] == 0
    solo = _solo(dec, [xs[b] for b in check], X4.DEC_NEW)
    margins = [_oracle_step_margins(sd4, cfg, xs[b].float(), st[0].tolist()) for b, (st, _) in zip(check, solo)]
    got = _compare_on_decidable_pairs(solo, [outs[b] for b in check], blogits[:, check], margins)
    assert 2 * got >= len(check) * (X4.DEC_NEW - 1), (got, len(check))
    if nb > 64:                                                                  # a slot past 64 is among the pairs compared
        assert any(margins[i][0] >= 1e-2 for i, b in enumerate(check) if b >= 64)


def _dequantised_pair(ops, seed=G5_SEED, max_seq_len=128):
    """(MXFP4 tiled decoder, 16-bit decoder) on the SAME dequantised expert weights E2M1 2^e: the MXFP4 decoder's own 16-bit stacks are
    overwritten with them too, so both prefills are the same arithmetic and the decoders differ by the grouped kernel of the batched step
    alone."""
    from videollama2_amd import _lib
    from videollama2_amd.decoder import HipMixtralDecoder
    cfg, sd, dec = _decoder(seed=seed, max_seq_len=max_seq_len)
    d16 = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=max_seq_len).enable_moe_batch()
    assert d16.MOE_SKINNY_ROWS == 0 and not d16.moe_mxfp4 and not d16.moe_fp8   # the 16-bit default: the tiled grouped GEMM from MOE_GEMM_BATCH on
    for lw4, lw16, w4 in zip(dec.w["layers"], d16.w["layers"], dec.w4moe):
        for name in ("wgu", "wd"):
            q, s = w4[name]
            deq = torch.stack([M4.dequant(q[e], s[e]) for e in range(q.shape[0])]).to(DEV)
            lw4[name].copy_(deq.to(_lib.elem_dtype()))
            lw16[name].copy_(deq.to(_lib.elem_dtype()))
            assert torch.equal(lw16[name].float(), deq)
            q2, s2 = ops.moe_quant_mxfp4(lw4[name])                                # quantising the dequantised stack gives the same values back
            assert torch.equal(torch.stack([M4.dequant(q2[e], s2[e]) for e in range(q.shape[0])]).to(DEV), deq)
    return dec, d16


@pytest.mark.parametrize("nb", [8, 70])
def test_tiled_mxfp4_step_is_bit_for_bit_the_16_bit_tiled_step_on_the_dequantised_experts(ops, nb):
    dec, d16 = _dequantised_pair(ops)
    lens = G5_LENS if nb == 8 else [1 + (7 * b) % 40 for b in range(nb)]
    xs = [x.to(DEV) for x in _prompts(lens, seed=G5_SEED)]
    t4, l4 = dec.generate_batch(xs, max_new_tokens=G5_NEW, return_logits=True)
    t16, l16 = d16.generate_batch(xs, max_new_tokens=G5_NEW, return_logits=True)
    assert [t.tolist() for t in t4] == [t.tolist() for t in t16]
    assert torch.equal(l4, l16)


def test_continuous_batcher_eight_slots_with_a_sampled_request(ops, monkeypatch):
    """Eight slots in flight run the tiled form (MOE_MXFP4_TILED_FROM = 5 here): the batcher's rows are generate_batch's rows, the sampled
    request under the same uniform numbers."""
    from videollama2_amd.serving import ContinuousBatcher
    cfg, sd, dec = _decoder()
    cnt = _spy(dec, monkeypatch)
    xs = [x.to(DEV) for x in _prompts(G5_LENS, seed=8)]
    T, tk, tp, n = 1.1, 20, 0.9, 4
    ref, _ = dec.generate_batch(xs, max_new_tokens=n, return_logits=True, sampler=(T, tk, tp, torch.Generator(device=DEV).manual_seed(5)))
    g2 = torch.Generator(device=DEV).manual_seed(5)
    us = torch.stack([torch.rand((n + 1,), device=DEV, generator=g2) for _ in xs])
    greedy = dec.generate_batch(xs, max_new_tokens=n)
    assert cnt["tiled"] > 0 and cnt["skinny"] == 0                              # (the captures above: the batcher replays those graphs)
    b = ContinuousBatcher(dec, max_slots=8)
    rid = [b.submit(x, max_new_tokens=n, **(dict(do_sample=True, temperature=T, top_k=tk, top_p=tp) if i == 1 else {})) for i, x in enumerate(xs)]
    b.waiting[1].u = us[1, :n].clone()
    done = b.run()
    assert cnt["skinny"] == 0
    for i in range(len(xs)):
        assert done[rid[i]].tolist() == (ref[i] if i == 1 else greedy[i]).tolist(), i
    b.submit(xs[0], max_new_tokens=3)
    b.step()
    with pytest.raises(RuntimeError, match="enable_moe_mxfp4: a ContinuousBatcher holds requests in flight"):
        dec.enable_moe_mxfp4(tiled=False)
    b.run()


def test_tiled_off_restores_the_skinny_form_bit_for_bit_and_the_refusal(ops, monkeypatch):
    cfg, sd, dec = _decoder(tiled=False)
    cnt = _spy(dec, monkeypatch)
    xs = [x.to(DEV) for x in _prompts(G5_LENS, seed=3)]
    base = dec.generate_batch(xs, max_new_tokens=4, return_logits=True)
    assert cnt["skinny"] > 0 and cnt["tiled"] == 0
    epoch = dec.cache_epoch
    dec.enable_moe_mxfp4(tiled=True)
    assert dec._batch_graphs == {} and dec.cache_epoch == epoch + 1
    assert dec._ensure_batch(65)["B"] >= 65
    tiled = dec.generate_batch(xs, max_new_tokens=4, return_logits=True)
    assert cnt["tiled"] > 0 and torch.equal(tiled[1][0], base[1][0])            # step 0 is the prefill: 16-bit, untouched
    seen = cnt["tiled"]
    dec.enable_moe_mxfp4(tiled=False)
    with pytest.raises(NotImplementedError, match="at most 64 sequences.*no tiled W4A16 grouped GEMM is built"):
        dec._ensure_batch(65)
    again = dec.generate_batch(xs, max_new_tokens=4, return_logits=True)
    assert cnt["tiled"] == seen
    assert [t.tolist() for t in again[0]] == [t.tolist() for t in base[0]] and torch.equal(again[1], base[1])
