"""fp8 expert weights in every decode path of the Mixtral decoder (enable_moe_fp8; csrc/k_moe_fp8.h): the stack
quantiser, the expert-indexed fp8 GEMVs against ops.gemv_fp8 per slot, the down form on exact inputs and against an exactly rounded fma chain,
the grouped skinny-M GEMM row by row against ops.gemm_skinny_fp8, the fp16 build, and the decoder: solo, few requests, 8 and 64 requests, the
dequantised 16-bit decoder, the batcher and the switch.  Every comparison is torch.equal unless a bound is stated.
Small Mixtral config (D 256, I 512, 8 experts, top 2, 2 layers, head_dim 128)."""
import pytest
import torch

from oracle import fp8_oracle as F8
from tests import moe_exact as X
from tests import moe_fp8_exact as X8
from tests import moe_oracle as MO
from tests.test_gpu_moe_batch import _compare_to_rounding, _ids_from_counts, _oracle_step_margins, _prompts, _solo, _tables
from tests.util import rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, I, E, K2 = 256, 512, 8, 2
SENT, POISON = X.SENTINEL, 12288.0
QPAD = 0x7F                               # the NaN code of e4m3fn: the poison of the byte stacks' pads


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def _el(t):
    from videollama2_amd import _lib
    return t.to(device=DEV, dtype=_lib.elem_dtype()).contiguous()


def _stack8(wi, pad=True):
    """An expert stack [E, N, K] (exact in the element type) -> (q view [E, N, K] bytes, scale view [E, N]) from ops.moe_quant_fp8, laid into
    poisoned storages with ldq = K + 16, one extra row per expert (q_stride > N ldq) and s_stride = N + 3."""
    from videollama2_amd import ops
    w = _el(wi)
    assert torch.equal(w.double().cpu(), wi.double().cpu()), "the stack is not exact in the element type"
    q, sc = ops.moe_quant_fp8(w)
    if not pad:
        return q, sc
    n_exp, N, K = q.shape
    qs = torch.full((n_exp, N + 1, K + 16), QPAD, dtype=torch.uint8, device=DEV)
    ss = torch.full((n_exp, N + 3), float("nan"), dtype=torch.float32, device=DEV)
    qs[:, :N, :K], ss[:, :N] = q, sc
    return qs[:, :N, :K], ss[:, :N]


# ---------------------------------------------------------------------------------------------------------------- the quantiser
def test_stack_quantiser_equals_the_row_quantiser_expert_by_expert_and_the_oracle():
    from videollama2_amd import ops
    w = _el(X8.quant_stack())
    n_exp, N, K = w.shape
    q, sc = ops.moe_quant_fp8(w)
    assert q.shape == (n_exp, N, K) and q.dtype == torch.uint8 and sc.shape == (n_exp, N) and sc.dtype == torch.float32
    for e in range(n_exp):
        qe, se = ops.quant_fp8(w[e])
        assert torch.equal(q[e], qe) and torch.equal(sc[e], se), e
        qo, so = F8.quant_rows(w[e])
        assert torch.equal(q[e].cpu(), qo) and torch.equal(sc[e].cpu(), so), e
    assert sc[1, 4].item() == 1.0 and not q[1, 4].any()                    # the zero row: scale 1, codes 0
    assert len(set(sc[0, :5].tolist())) >= 3 and not torch.equal(sc[0], sc[2])      # rows and experts carry their own scales
    with pytest.raises(ValueError, match="contiguous"):
        ops.moe_quant_fp8(w[:, :, :16])


# ---------------------------------------------------------------------------------------------------------------- gate/up
@pytest.mark.parametrize("case", X8.GU8_CASES, ids=lambda c: "E%d-k%d-N%d-K%d" % c)
def test_gate_up_is_gemv_fp8_per_slot(case):
    """The solo form and the rows form (3 tokens) against ops.gemv_fp8(swiglu, rms_plain) on the slot's expert; outputs in sentinel frames."""
    from videollama2_amd import ops
    n_exp, k, N, K = case
    for S, batched in ((1, False), (X8.GU8_ROWS_S, True)):
        c = X8.GateUp8Case(S, n_exp, k, N, K, batched)
        assert 0 in c.ids[0].tolist() or k == 1
        assert n_exp - 1 in c.ids[0].tolist()
        q, sc = _stack8(c.wi)
        x_st = torch.full((S + 1, K + 8), float("nan"), dtype=torch.float32)
        x_st[:S, :K] = c.x.float()
        x = _el(x_st)[:S, :K]
        ids = c.ids.int().to(DEV)
        if not batched:
            out = _el(torch.full((k + 2, N // 2), SENT))
            ops.moe_gemv_fp8(q, sc, x[0], ids[0].contiguous(), swiglu=True, eps=X.EPS, out=out[1:k + 1])
            rows, frame = out[1:k + 1], torch.cat([out[:1].flatten(), out[k + 1:].flatten()])
        else:
            out = _el(torch.full((S * k + 1, N // 2 + 8), SENT))
            ops.moe_gemv_batched_fp8(q, sc, x, ids, swiglu=True, eps=X.EPS, out=out[:S * k, :N // 2])
            rows, frame = out[:S * k, :N // 2], torch.cat([out[S * k:].flatten(), out[:, N // 2:].flatten()])
        torch.cuda.synchronize()
        assert bool((frame == SENT).all()), (case, S, "the frame was written")          # (compared in the element type, which rounds the sentinel)
        for t in range(S):
            for j in range(k):
                e = int(c.ids[t, j])
                want = ops.gemv_fp8(q[e], sc[e], x[t], swiglu=True, rms_plain=True, eps=X.EPS)
                assert torch.equal(rows[t * k + j], want), (case, S, t, j, e)
        assert bool(torch.isfinite(rows.float()).all()) and float(rows.float().abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- down (a): exact inputs
def _run_down8(ops, c):
    el = X.elem_dtype()
    S, k, N, K = c.S, c.k, c.N, c.K
    q, sc = _stack8(c.wi)
    a = c.store["a"].to(el).to(DEV)
    ids, wts = c.ids.int().to(DEV), c.wts.float().to(DEV)
    res = c.store["res"].to(el).to(DEV) if c.res is not None else None
    if not c.batched:
        st, y = X.framed((N,), el, DEV)
        ops.moe_gemv_fp8(q, sc, a[:k], ids[0].contiguous(), wts=wts[0].contiguous(), res=None if res is None else res[0, :N], out=y)
        return st.cpu()
    out = torch.full((S + 1, N + 5), SENT, dtype=el, device=DEV)
    ops.moe_gemv_batched_fp8(q, sc, a[:S * k], ids, wts=wts, res=None if res is None else res[:S, :N], out=out[:S, :N])
    return out.cpu()


def test_down_on_exact_inputs_equals_the_fp64_answer():
    """Every row of moe_fp8_exact.down8_table: every KS in 1 .. 4, with and without res, N in {1, 3, 4, 5, 41}, single and batched (S in {1, 2,
    5}), K at the vector, slot and pass edges and at the LDS limit; check_down = torch.equal with bf16(fp64) and the frame intact."""
    from videollama2_amd import ops
    errs = []
    for r in X8.down8_table():
        c = X8.Down8Case(r)
        err = X.check_down(c, _run_down8(ops, c))
        if err:
            errs.append(err)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("batched", [False, True])
def test_down_refuses_the_first_k_beyond_the_lds(batched):
    from videollama2_amd import _lib, ops
    el, n_exp, N, k, K = X.elem_dtype(), 4, 5, 4, X8.DOWN8_K_REFUSED
    S = 2 if batched else 1
    q = torch.zeros((n_exp, N, K), dtype=torch.uint8, device=DEV)
    sc = torch.ones((n_exp, N), dtype=torch.float32, device=DEV)
    a = torch.zeros((S * k, K), dtype=el, device=DEV)
    ids = torch.arange(k, dtype=torch.int32, device=DEV).repeat(S, 1)
    wts = torch.full((S, k), 0.25, dtype=torch.float32, device=DEV)
    out = torch.full((S + 1, N + 3), SENT, dtype=el, device=DEV)
    with pytest.raises(_lib.Vl2HipError, match="must fit the LDS"):
        if batched:
            ops.moe_gemv_batched_fp8(q, sc, a, ids, wts=wts, out=out[:S, :N])
        else:
            ops.moe_gemv_fp8(q, sc, a, ids[0].contiguous(), wts=wts[0].contiguous(), out=out[0, :N])
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---------------------------------------------------------------------------------------------------------------- down (b): the fma chain
@pytest.mark.parametrize("S,k,N,K,has_res", [(1, 2, 42, 1040, True), (1, 4, 6, 8208, False), (3, 3, 8, 528, True), (2, 1, 4, 16, True)])
def test_down_on_random_inputs_is_the_exactly_rounded_fma_chain(S, k, N, K, has_res):
    """y = bf16(fl32(res + o)), o = fma(w_j, d_j, o) in slot order from 0 with d_j = ops.gemv_fp8(out_f32=True) on the slot's expert and row:
    the chain is rebuilt in exact rational arithmetic, one rounding per fma.  (N even: ops.gemv_fp8 owns pairs of rows; odd N run in (a).)"""
    from videollama2_amd import ops
    el = X.elem_dtype()
    g = torch.Generator().manual_seed(1000 * S + 10 * k + N)
    n_exp = 8
    w = _el(torch.randn((n_exp, N, K), generator=g) * X8.row_powers(N).float()[None, :, None] * K ** -0.5)
    q, sc = _stack8(w.float())
    a = _el(torch.randn((S * k, K), generator=g))
    ids = X._ids_for(S, n_exp, k, g).int().to(DEV)
    wts = torch.softmax(torch.randn((S, k), generator=g), 1).float().to(DEV)
    res = _el(torch.randn((S, N), generator=g)) if has_res else None
    if S == 1:
        st, y = X.framed((N,), el, DEV)
        ops.moe_gemv_fp8(q, sc, a, ids[0].contiguous(), wts=wts[0].contiguous(), res=None if res is None else res[0], out=y)
        got = y[None].cpu()
        assert X.frame_intact(st, N)
    else:
        out = torch.full((S + 1, N + 5), SENT, dtype=el, device=DEV)
        ops.moe_gemv_batched_fp8(q, sc, a, ids, wts=wts, res=res, out=out[:S, :N])
        got = out[:S, :N].cpu()
        assert bool((out[S:] == SENT).all()) and bool((out[:, N:] == SENT).all())
    want = torch.empty((S, N), dtype=torch.float32)
    for t in range(S):
        d = torch.stack([ops.gemv_fp8(q[int(ids[t, j])], sc[int(ids[t, j])], a[t * k + j], out_f32=True) for j in range(k)]).cpu()      # [k, N] fp32
        for n in range(N):
            want[t, n] = X8.fma_chain(wts[t].tolist(), d[:, n].tolist(), None if res is None else float(res[t, n]))
    assert torch.equal(got, want.to(el)), (got.float() - want).abs().max()


def test_down_slot_order_shows():
    from videollama2_amd import _lib, ops
    assert _lib.elem() == "bf16"                                              # (the numbers are chosen for an 8-bit significand)
    c = X8.Down8Case.order_case8()
    st = _run_down8(ops, c)
    assert st[8:8 + c.N].float().tolist() == [1.0078125] * 3, st[8:8 + c.N].tolist()      # the reverse order would store 1.0
    assert X.check_down(c, st) is None


# ---------------------------------------------------------------------------------------------------------------- the grouped skinny-M GEMM
def _grouped8_vs_dense(nb, counts, shrink=None):
    """Gate/up (SwiGLU, rows through the row map; N 1024, K 256) and down (N 256, K 512) on crafted tables: every owned permuted row equals
    ops.gemm_skinny_fp8 on that row with its expert's bytes and scales, the whole output equals ops.moe_gemm_skinny on the dequantised stack on
    the owned rows; rows nobody owns keep the poison in the partials AND in the output."""
    from videollama2_amd import ops
    ops.attach_workspace(DEV)
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
    g = torch.Generator().manual_seed(nb)
    h = _el(torch.randn((nb, D), generator=g))
    a_in = _el(torch.randn((R, I), generator=g) * 0.5)
    for (A, wi, rowmap, sw, N, K) in ((h, X8.skinny8_stack(E, 2 * I, D, 1), gather.to(DEV), True, 2 * I, D),
                                      (a_in, X8.skinny8_stack(E, D, I, 2), None, False, D, I)):
        q, sc = _stack8(wi)
        need = ops.moe_skinny_part_bytes(nb, 2, N, K) // 4
        ks = need // (R * N)
        assert ks > 1
        part = torch.full((need + 64,), POISON, dtype=torch.float32, device=DEV)
        ncol = N // 2 if sw else N
        out = _el(torch.full((R + 3, ncol + 4), POISON))
        ops.moe_gemm_skinny_fp8(A, q, sc, t, nb, 2, part, rowmap=rowmap, swiglu=sw, out=out[:R, :ncol])
        torch.cuda.synchronize()
        pv = part[:need].view(ks, R, N).cpu()
        assert (part[need:] == POISON).all() and (out[R:].float() == POISON).all() and (out[:, ncol:].float() == POISON).all()
        assert (pv[:, ~owned] == POISON).all(), "partial rows nobody owns were written"
        assert torch.isfinite(pv[:, owned]).all() and (pv[:, owned] != POISON).all(), "an owned partial row was not written"
        assert (out[:R, :ncol][~owned.to(DEV)].float() == POISON).all(), "an output row nobody owns was written"
        for p in torch.where(owned)[0].tolist():
            e = int(torch.searchsorted(offs[1:].contiguous(), torch.tensor(p), right=True))
            src = int(gather[p]) if rowmap is not None else p
            want = ops.gemm_skinny_fp8(A[src:src + 1], q[e], sc[e], swiglu=sw)
            assert torch.equal(out[p:p + 1, :ncol], want), (("gate/up" if sw else "down"), p, e)
        # the 16-bit grouped kernel on the dequantised stack q 2^e, which the element type holds exactly
        deq = _el(wi)
        part16 = torch.empty((need,), dtype=torch.float32, device=DEV)
        want16 = ops.moe_gemm_skinny(A, deq, t, nb, 2, part16, rowmap=rowmap, swiglu=sw)
        assert torch.equal(out[:R, :ncol][owned.to(DEV)], want16[owned.to(DEV)]), ("gate/up" if sw else "down")


@pytest.mark.parametrize("case", list(X8.SKINNY8_CASES))
def test_grouped_skinny_fp8_row_by_row(case):
    nb, counts = X8.SKINNY8_CASES[case]
    _grouped8_vs_dense(nb, counts)


def test_grouped_skinny_fp8_leaves_unowned_rows_alone():
    nb, counts = X8.SKINNY8_CASES["ragged"]
    _grouped8_vs_dense(nb, counts, shrink={0: 30, 1: 16, 5: 0})


# ---------------------------------------------------------------------------------------------------------------- the fp16 build
def test_the_kernels_on_the_fp16_build():
    """A reduced table on libvl2hip_f16.so: one gate/up case per NP, down at every KS and both pass counts, the grouped form at two sizes."""
    from videollama2_amd import _lib, ops
    _lib.set_elem("fp16")
    try:
        for case in ((4, 2, 64, 1040), (4, 4, 192, 4112)):
            test_gate_up_is_gemv_fp8_per_slot(case)
        errs = [X.check_down(c, _run_down8(ops, c)) for c in (X8.Down8Case(r) for r in X8.down8_table() if r.N == 5 and r.K in (1040, 8208))]
        assert len(errs) >= 8 and not any(errs), errs
        _grouped8_vs_dense(*X8.SKINNY8_CASES["five"])
        _grouped8_vs_dense(*X8.SKINNY8_CASES["ragged"])
    finally:
        _lib.set_elem("bf16")


# ---------------------------------------------------------------------------------------------------------------- the decoder
def _decoder(seed=9, n_layers=2, max_seq_len=128, fp8=True):
    from videollama2_amd.decoder import HipMixtralDecoder
    cfg = MO.small_mixtral_cfg(n_layers=n_layers)
    sd = MO.seeded_state_dict(cfg, seed=seed, router_scale=4.0)
    dec = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=max_seq_len).enable_moe_batch()
    assert dec.moe_fp8 is False
    if fp8:
        dec.enable_moe_fp8()
    return cfg, sd, dec


def test_solo_step_graph_and_eager_agree_and_the_switch_restores_16_bit():
    cfg, sd, dec = _decoder(fp8=False)
    x = _prompts((20,), seed=1)[0].to(DEV)
    base = dec.generate(x, max_new_tokens=6, return_logits=True)
    epoch = dec.cache_epoch
    assert dec.enable_moe_fp8() is dec and dec.moe_fp8 and dec.decode_format == "16bit" and dec.cache_epoch == epoch + 1 and dec.graph is None
    assert len(dec.w8moe) == dec.n_layers and dec.w8moe[0]["wgu"][0].shape == (E, 2 * I, D) and dec.w8moe[0]["wd"][1].shape == (E, D)
    runs = [dec.generate(x, max_new_tokens=6, return_logits=True, use_graph=g) for g in (True, False)]
    assert dec.graph is not None
    assert runs[0][0].tolist() == runs[1][0].tolist() and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][1][0], base[1][0])                              # step 0 is the prefill: 16-bit, untouched
    assert not torch.equal(runs[0][1][1:], base[1][1:])                        # (the fp8 expert products ran)
    epoch = dec.cache_epoch                                                    # (a prefill bumps it too)
    dec.enable_moe_fp8(False)
    assert dec.graph is None and dec.cache_epoch == epoch + 1
    again = dec.generate(x, max_new_tokens=6, return_logits=True)
    assert again[0].tolist() == base[0].tolist() and torch.equal(again[1], base[1])


@pytest.mark.parametrize("nb", [2, 4])
def test_few_requests_are_bit_for_bit_the_solo_fp8_step(nb):
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


G5_LENS, G5_SEED, G5_NEW = (40, 1, 23, 5, 64, 17, 33, 9), 0, 4


@pytest.mark.parametrize("nb", [8, 64])
def test_8_and_64_requests_match_solo_fp8_to_summation_order(nb):
    """The grouped skinny-M form against the solo fp8 step on the (request, step) pairs whose routing the fp32 oracle decides with margin >= 1e-2:
    the 16-bit form-against-form bound of tests/test_gpu_moe_batch.py, 2e-2 rel-L2 on the logits (the forms differ by summation order only)."""
    cfg, sd, dec = _decoder(seed=G5_SEED)
    lens = G5_LENS if nb == 8 else [1 + (7 * b) % 40 for b in range(nb)]
    xs = _prompts(lens, seed=G5_SEED)
    check = list(range(nb)) if nb == 8 else [0, 9, 23, 38, 47, 63]          # (the solo reference of six of the 64 requests)
    outs, blogits = dec.generate_batch([x.to(DEV) for x in xs], max_new_tokens=G5_NEW, return_logits=True)
    assert dec.MOE_GEMM_BATCH <= nb <= dec.MOE_FP8_ROWS
    solo = _solo(dec, [xs[b] for b in check], G5_NEW)
    margins = [_oracle_step_margins(sd, cfg, xs[b].float(), st[0].tolist()) for b, (st, _) in zip(check, solo)]
    decidable = [i for i, m in enumerate(margins) if m[0] >= 1e-2]
    assert len(decidable) >= (len(check) + 1) // 2
    n = _compare_to_rounding([solo[i] for i in decidable], [outs[check[i]] for i in decidable], blogits[:, [check[i] for i in decidable]],
                             [margins[i] for i in decidable], min_pairs=len(decidable))
    assert n >= len(decidable)


def _dequantised_decoder(dec, cfg, sd):
    """A second decoder whose 16-bit expert weights are the dequantised fp8 copies q 2^e of `dec` (exact in the element type)."""
    from videollama2_amd import _lib
    from videollama2_amd.decoder import HipMixtralDecoder
    d16 = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=dec.max_seq_len)
    for lw, w8 in zip(d16.w["layers"], dec.w8moe):
        for name in ("wgu", "wd"):
            q, sc = w8[name]
            deq = q.view(torch.float8_e4m3fn).float() * sc[:, :, None]
            lw[name].copy_(deq.to(_lib.elem_dtype()))
            assert torch.equal(lw[name].float(), deq)
    return d16


def test_fp8_step_against_the_16_bit_step_on_the_dequantised_weights():
    """The bound of the dense decoders' same comparison (tests/test_gpu_fp8.py): 6e-3 rel-L2 on the logits, on the margin-filtered steps.  The
    16-bit decoder steps teacher-forced on the fp8 decoder's own tokens and cache rows (its prefill would read the dequantised experts, the fp8
    decoder's reads the original ones), so a step differs by the expert products' arithmetic alone."""
    cfg, sd, dec = _decoder(seed=G5_SEED)
    d16 = _dequantised_decoder(dec, cfg, sd)
    n = 0
    for x in _prompts(G5_LENS[:4], seed=G5_SEED):
        L = x.shape[0]
        t8, l8 = dec.generate(x.to(DEV), max_new_tokens=G5_NEW, return_logits=True)
        margins = _oracle_step_margins(sd, cfg, x.float(), t8[0].tolist())
        for s in range(1, G5_NEW):
            if margins[s - 1] < 1e-2:
                break
            for li in range(dec.n_layers):
                d16.kcache[li].copy_(dec.kcache[li])
                d16.vcache[li].copy_(dec.vcache[li])
            d16.pos = L + s - 1
            l16 = d16.decode_step(t8[0, s - 1:s].to(torch.int32))
            r = rel(l8[s], l16)
            print(f"prompt of {L} rows, step {s}: fp8 against dequantised 16-bit rel {r:.3e} (oracle routing margin {margins[s - 1]:.3e})")
            assert r < 6e-3, (L, s, r)
            n += 1
    assert n >= 4


def test_continuous_batcher_four_slots_equals_solo_fp8_with_a_sampled_request():
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
        b.step(); b.step()
        rid += [sub(4), sub(5)]
        done = b.run()
        assert [done[r].tolist() for r in rid] == solo, use_graph
    # a sampled request beside greedy ones: the rows are generate_batch's rows under the same uniform numbers
    T, tk, tp, n = 1.1, 20, 0.9, 4
    ref, _ = dec.generate_batch(xs[:3], max_new_tokens=n, return_logits=True, sampler=(T, tk, tp, torch.Generator(device=DEV).manual_seed(5)))
    g2 = torch.Generator(device=DEV).manual_seed(5)
    us = torch.stack([torch.rand((n + 1,), device=DEV, generator=g2) for _ in xs[:3]])
    greedy = dec.generate_batch(xs[:3], max_new_tokens=n)
    b = ContinuousBatcher(dec, max_slots=4)
    rid = [b.submit(x, max_new_tokens=n, **(dict(do_sample=True, temperature=T, top_k=tk, top_p=tp) if i == 1 else {})) for i, x in enumerate(xs[:3])]
    b.waiting[1].u = us[1, :n].clone()
    done = b.run()
    for i in range(3):
        assert done[rid[i]].tolist() == (ref[i] if i == 1 else greedy[i]).tolist(), i
    b.submit(xs[0], max_new_tokens=3)
    b.step()
    with pytest.raises(RuntimeError, match="enable_moe_fp8: a ContinuousBatcher holds requests in flight"):
        dec.enable_moe_fp8(False)
    b.run()


def test_more_than_64_requests_are_refused_and_the_switch_off_restores_the_16_bit_batch():
    cfg, sd, dec = _decoder(max_seq_len=64, fp8=False)
    xs = [x.to(DEV) for x in _prompts((20, 1, 33), seed=3)]
    base = dec.generate_batch(xs, max_new_tokens=4, return_logits=True)
    dec.enable_moe_fp8()
    with pytest.raises(NotImplementedError, match="at most 64 sequences"):
        dec._ensure_batch(65)
    fp8 = dec.generate_batch(xs, max_new_tokens=4, return_logits=True)
    assert not torch.equal(fp8[1][1:], base[1][1:])
    dec.enable_moe_fp8(False)
    again = dec.generate_batch(xs, max_new_tokens=4, return_logits=True)
    assert [t.tolist() for t in again[0]] == [t.tolist() for t in base[0]] and torch.equal(again[1], base[1])
