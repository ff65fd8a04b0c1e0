"""MXFP4 expert weights in every decode path of the Mixtral decoder (enable_moe_mxfp4; csrc/k_moe_mxfp4.h): the stack
quantiser, the expert-indexed MXFP4 GEMVs against ops.gemv_mxfp4 per slot, the down form on exact inputs and against an exactly rounded fma
chain, the grouped skinny-M GEMM row by row against ops.gemm_skinny_mxfp4, the fp16 build, and the decoder: solo, few requests, 8 and 64
requests, the dequantised 16-bit decoder, the batcher and the switch.  Every comparison is torch.equal unless a bound is stated.
Small Mixtral config (D 256, I 512, 8 experts, top 2, 2 layers, head_dim 128)."""
import pytest
import torch

from tests import moe_exact as X
from tests import moe_mxfp4_exact as X4
from tests import moe_oracle as MO
from tests import mxfp4_oracle as M4
from tests.test_gpu_moe_batch import _ids_from_counts, _oracle_step_margins, _prompts, _solo, _tables
from tests.util import rel, token_tie_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, I, E, K2 = 256, 512, 8, 2
SENT, POISON = X.SENTINEL, 12288.0
QPAD, SPAD = 0x7F, 0xFF                   # the pads of the byte stacks: non-zero codes (-6 | 6) and the NaN scale byte of E8M0


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def _el(t):
    from videollama2_amd import _lib
    return t.to(device=DEV, dtype=_lib.elem_dtype()).contiguous()


def _stack4(wi, pad=True):
    """An expert stack [E, N, K] (exact in the element type) -> (q view [E, N, K / 2] bytes, s view [E, N, K / 32] bytes) from
    ops.moe_quant_mxfp4, laid into poisoned storages with ldq = K / 2 + 16, lds = K / 32 + 3 and one extra row per expert (q_stride > N ldq,
    s_stride > N lds); the pads hold non-zero codes and scale byte 0xFF."""
    from videollama2_amd import ops
    w = _el(wi)
    assert torch.equal(w.double().cpu(), wi.double().cpu()), "the stack is not exact in the element type"
    q, s = ops.moe_quant_mxfp4(w)
    if not pad:
        return q, s
    n_exp, N, K = w.shape
    qs = torch.full((n_exp, N + 1, K // 2 + 16), QPAD, dtype=torch.uint8, device=DEV)
    ss = torch.full((n_exp, N + 1, K // 32 + 3), SPAD, dtype=torch.uint8, device=DEV)
    qs[:, :N, :K // 2], ss[:, :N, :K // 32] = q, s
    return qs[:, :N, :K // 2], ss[:, :N, :K // 32]


# ---------------------------------------------------------------------------------------------------------------- the quantiser
def test_stack_quantiser_equals_the_row_quantiser_expert_by_expert_and_the_oracle():
    from videollama2_amd import ops
    w = _el(X4.quant_stack())
    n_exp, N, K = w.shape
    q, s = ops.moe_quant_mxfp4(w)
    assert q.shape == (n_exp, N, K // 2) and q.dtype == torch.uint8 and s.shape == (n_exp, N, K // 32) and s.dtype == torch.uint8
    for e in range(n_exp):
        qe, se = ops.quant_mxfp4(w[e])
        assert torch.equal(q[e], qe) and torch.equal(s[e], se), e
        qo, so = M4.quant_blocks(w[e])
        assert torch.equal(q[e].cpu(), qo) and torch.equal(s[e].cpu(), so), e
    assert s[1, 4].tolist() == [127] * (K // 32) and not q[1, 4].any()            # the zero row: scale 2^0, codes 0
    assert s[2, 0, 1].item() == 127 and not q[2, 0, 16:].any() and q[2, 0, :16].any()      # the zero block
    assert len(set(s[0, :5, 0].tolist())) >= 3 and not torch.equal(s[0], s[2])    # rows and experts carry their own scales
    with pytest.raises(ValueError, match="contiguous"):
        ops.moe_quant_mxfp4(w[:, :, :32])


# ---------------------------------------------------------------------------------------------------------------- gate/up
@pytest.mark.parametrize("case", X4.GU4_CASES, ids=lambda c: "E%d-k%d-N%d-K%d" % c)
def test_gate_up_is_gemv_mxfp4_per_slot(case):
    """The solo form and the rows form (3 tokens) against ops.gemv_mxfp4(swiglu, rms_plain) on the slot's expert; outputs in sentinel frames."""
    from videollama2_amd import ops
    n_exp, k, N, K = case
    for S, batched in ((1, False), (X4.GU4_ROWS_S, True)):
        c = X4.GateUp4Case(S, n_exp, k, N, K, batched)
        assert 0 in c.ids[0].tolist() or k == 1
        assert n_exp - 1 in c.ids[0].tolist()
        q, s = _stack4(c.wi)
        x_st = torch.full((S + 1, K + 8), float("nan"), dtype=torch.float32)
        x_st[:S, :K] = c.x.float()
        x = _el(x_st)[:S, :K]
        ids = c.ids.int().to(DEV)
        if not batched:
            out = _el(torch.full((k + 2, N // 2), SENT))
            ops.moe_gemv_mxfp4(q, s, x[0], ids[0].contiguous(), swiglu=True, eps=X.EPS, out=out[1:k + 1])
            rows, frame = out[1:k + 1], torch.cat([out[:1].flatten(), out[k + 1:].flatten()])
        else:
            out = _el(torch.full((S * k + 1, N // 2 + 8), SENT))
            ops.moe_gemv_batched_mxfp4(q, s, x, ids, swiglu=True, eps=X.EPS, out=out[:S * k, :N // 2])
            rows, frame = out[:S * k, :N // 2], torch.cat([out[S * k:].flatten(), out[:, N // 2:].flatten()])
        torch.cuda.synchronize()
        assert bool((frame == SENT).all()), (case, S, "the frame was written")          # (compared in the element type, which rounds the sentinel)
        for t in range(S):
            for j in range(k):
                e = int(c.ids[t, j])
                want = ops.gemv_mxfp4(q[e], s[e], x[t], swiglu=True, rms_plain=True, eps=X.EPS)
                assert torch.equal(rows[t * k + j], want), (case, S, t, j, e)
        assert bool(torch.isfinite(rows.float()).all()) and float(rows.float().abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- down (a): exact inputs
def _run_down4(ops, c):
    el = X.elem_dtype()
    S, k, N, K = c.S, c.k, c.N, c.K
    q, s = _stack4(c.wi)
    a = c.store["a"].to(el).to(DEV)
    ids, wts = c.ids.int().to(DEV), c.wts.float().to(DEV)
    res = c.store["res"].to(el).to(DEV) if c.res is not None else None
    if not c.batched:
        st, y = X.framed((N,), el, DEV)
        ops.moe_gemv_mxfp4(q, s, a[:k], ids[0].contiguous(), wts=wts[0].contiguous(), res=None if res is None else res[0, :N], out=y)
        return st.cpu()
    out = torch.full((S + 1, N + 5), SENT, dtype=el, device=DEV)
    ops.moe_gemv_batched_mxfp4(q, s, a[:S * k], ids, wts=wts, res=None if res is None else res[:S, :N], out=out[:S, :N])
    return out.cpu()


def test_down_on_exact_inputs_equals_the_fp64_answer():
    """Every row of moe_mxfp4_exact.down4_table: every KS in 1 .. 4, with and without res, N in {1, 3, 4, 5, 41}, single and batched (S in {1,
    2, 5}), K at the vector, slot and pass edges and at the LDS limit; check_down = torch.equal with elem(fp64) and the frame intact."""
    from videollama2_amd import ops
    errs = []
    for r in X4.down4_table():
        c = X4.Down4Case(r)
        err = X.check_down(c, _run_down4(ops, c))
        if err:
            errs.append(err)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("batched", [False, True])
def test_down_refuses_the_first_k_beyond_the_lds(batched):
    from videollama2_amd import _lib, ops
    el, n_exp, N, k, K = X.elem_dtype(), 4, 5, 4, X4.DOWN4_K_REFUSED
    S = 2 if batched else 1
    q = torch.zeros((n_exp, N, K // 2), dtype=torch.uint8, device=DEV)
    s = torch.full((n_exp, N, K // 32), 127, dtype=torch.uint8, device=DEV)
    a = torch.zeros((S * k, K), dtype=el, device=DEV)
    ids = torch.arange(k, dtype=torch.int32, device=DEV).repeat(S, 1)
    wts = torch.full((S, k), 0.25, dtype=torch.float32, device=DEV)
    out = torch.full((S + 1, N + 3), SENT, dtype=el, device=DEV)
    with pytest.raises(_lib.Vl2HipError, match="must fit the LDS"):
        if batched:
            ops.moe_gemv_batched_mxfp4(q, s, a, ids, wts=wts, out=out[:S, :N])
        else:
            ops.moe_gemv_mxfp4(q, s, a, ids[0].contiguous(), wts=wts[0].contiguous(), out=out[0, :N])
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---------------------------------------------------------------------------------------------------------------- down (b): the fma chain
@pytest.mark.parametrize("S,k,N,K,has_res", [(1, 2, 42, 2080, True), (1, 4, 6, 16416, False), (3, 3, 8, 544, True), (2, 1, 4, 32, True)])
def test_down_on_random_inputs_is_the_exactly_rounded_fma_chain(S, k, N, K, has_res):
    """y = elem(fl32(res + o)), o = fma(w_j, d_j, o) in slot order from 0 with d_j = ops.gemv_mxfp4(out_f32=True) on the slot's expert and row:
    the chain is rebuilt in exact rational arithmetic, one rounding per fma.  (N even: ops.gemv_mxfp4 owns pairs of rows; odd N run in (a).)"""
    from videollama2_amd import ops
    el = X.elem_dtype()
    g = torch.Generator().manual_seed(1000 * S + 10 * k + N)
    n_exp = 8
    w = _el(torch.randn((n_exp, N, K), generator=g) * K ** -0.5)
    q, s = ops.moe_quant_mxfp4(w)
    qs = torch.full((n_exp, N + 1, K // 2 + 16), QPAD, dtype=torch.uint8, device=DEV)
    ss = torch.full((n_exp, N + 1, K // 32 + 3), SPAD, dtype=torch.uint8, device=DEV)
    qs[:, :N, :K // 2], ss[:, :N, :K // 32] = q, s
    q, s = qs[:, :N, :K // 2], ss[:, :N, :K // 32]
    a = _el(torch.randn((S * k, K), generator=g))
    ids = X._ids_for(S, n_exp, k, g).int().to(DEV)
    wts = torch.softmax(torch.randn((S, k), generator=g), 1).float().to(DEV)
    res = _el(torch.randn((S, N), generator=g)) if has_res else None
    if S == 1:
        st, y = X.framed((N,), el, DEV)
        ops.moe_gemv_mxfp4(q, s, a, ids[0].contiguous(), wts=wts[0].contiguous(), res=None if res is None else res[0], out=y)
        got = y[None].cpu()
        assert X.frame_intact(st, N)
    else:
        out = torch.full((S + 1, N + 5), SENT, dtype=el, device=DEV)
        ops.moe_gemv_batched_mxfp4(q, s, a, ids, wts=wts, res=res, out=out[:S, :N])
        got = out[:S, :N].cpu()
        assert bool((out[S:] == SENT).all()) and bool((out[:, N:] == SENT).all())
    want = torch.empty((S, N), dtype=torch.float32)
    for t in range(S):
        d = torch.stack([ops.gemv_mxfp4(q[int(ids[t, j])], s[int(ids[t, j])], a[t * k + j], out_f32=True) for j in range(k)]).cpu()      # [k, N] fp32
        for n in range(N):
            want[t, n] = X4.fma_chain(wts[t].tolist(), d[:, n].tolist(), None if res is None else float(res[t, n]))
    assert torch.equal(got, want.to(el)), (got.float() - want).abs().max()


def test_down_slot_order_shows():
    from videollama2_amd import _lib, ops
    assert _lib.elem() == "bf16"                                              # (the numbers are chosen for an 8-bit significand)
    c = X4.Down4Case.order_case4()
    st = _run_down4(ops, c)
    assert st[8:8 + c.N].float().tolist() == [1.0078125] * 3, st[8:8 + c.N].tolist()      # the reverse order would store 1.0
    assert X.check_down(c, st) is None


# ---------------------------------------------------------------------------------------------------------------- the grouped skinny-M GEMM
def _grouped4_vs_dense(nb, counts, shrink=None):
    """Gate/up (SwiGLU, rows through the row map; N 1024, K 256) and down (N 256, K 512) on crafted tables: every owned permuted row equals
    ops.gemm_skinny_mxfp4 on that row with its expert's bytes and scales, the whole output equals ops.moe_gemm_skinny on the dequantised stack
    on the owned rows; rows nobody owns keep the poison in the partials AND in the output."""
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
    for (A, wi, rowmap, sw, N, K) in ((h, X4.skinny4_stack(E, 2 * I, D, 1), gather.to(DEV), True, 2 * I, D),
                                      (a_in, X4.skinny4_stack(E, D, I, 2), None, False, D, I)):
        q, s = _stack4(wi)
        need = ops.moe_skinny_part_bytes(nb, 2, N, K) // 4
        ks = need // (R * N)
        assert ks > 1
        part = torch.full((need + 64,), POISON, dtype=torch.float32, device=DEV)
        ncol = N // 2 if sw else N
        out = _el(torch.full((R + 3, ncol + 4), POISON))
        ops.moe_gemm_skinny_mxfp4(A, q, s, t, nb, 2, part, rowmap=rowmap, swiglu=sw, out=out[:R, :ncol])
        torch.cuda.synchronize()
        pv = part[:need].view(ks, R, N).cpu()
        assert (part[need:] == POISON).all() and (out[R:].float() == POISON).all() and (out[:, ncol:].float() == POISON).all()
        assert (pv[:, ~owned] == POISON).all(), "partial rows nobody owns were written"
        assert torch.isfinite(pv[:, owned]).all() and (pv[:, owned] != POISON).all(), "an owned partial row was not written"
        assert (out[:R, :ncol][~owned.to(DEV)].float() == POISON).all(), "an output row nobody owns was written"
        for p in torch.where(owned)[0].tolist():
            e = int(torch.searchsorted(offs[1:].contiguous(), torch.tensor(p), right=True))
            src = int(gather[p]) if rowmap is not None else p
            want = ops.gemm_skinny_mxfp4(A[src:src + 1], q[e], s[e], swiglu=sw)
            assert torch.equal(out[p:p + 1, :ncol], want), (("gate/up" if sw else "down"), p, e)
        # the 16-bit grouped kernel on the dequantised stack g 2^p, which the element type holds exactly
        deq = _el(wi)
        part16 = torch.empty((need,), dtype=torch.float32, device=DEV)
        want16 = ops.moe_gemm_skinny(A, deq, t, nb, 2, part16, rowmap=rowmap, swiglu=sw)
        assert torch.equal(out[:R, :ncol][owned.to(DEV)], want16[owned.to(DEV)]), ("gate/up" if sw else "down")


@pytest.mark.parametrize("case", list(X4.SKINNY4_CASES))
def test_grouped_skinny_mxfp4_row_by_row(case):
    nb, counts = X4.SKINNY4_CASES[case]
    _grouped4_vs_dense(nb, counts)


def test_grouped_skinny_mxfp4_leaves_unowned_rows_alone():
    nb, counts = X4.SKINNY4_CASES["ragged"]
    _grouped4_vs_dense(nb, counts, shrink={0: 30, 1: 16, 5: 0})


# ---------------------------------------------------------------------------------------------------------------- the fp16 build
def test_the_kernels_on_the_fp16_build():
    """A reduced table on libvl2hip_f16.so: one gate/up case per NP, down at every KS and both pass counts, the grouped form at two sizes."""
    from videollama2_amd import _lib, ops
    _lib.set_elem("fp16")
    try:
        for case in ((64, 2, 64, 2080), (4, 4, 64, 4128)):
            test_gate_up_is_gemv_mxfp4_per_slot(case)
        errs = [X.check_down(c, _run_down4(ops, c)) for c in (X4.Down4Case(r) for r in X4.down4_table() if r.N == 5 and r.K in (2080, X4.DOWN4_K[4]))]
        assert len(errs) >= 8 and not any(errs), errs
        _grouped4_vs_dense(*X4.SKINNY4_CASES["five"])
        _grouped4_vs_dense(*X4.SKINNY4_CASES["ragged"])
    finally:
        _lib.set_elem("bf16")


# ---------------------------------------------------------------------------------------------------------------- the decoder
def _decoder(seed=9, n_layers=2, max_seq_len=128, mxfp4=True):
    from videollama2_amd.decoder import HipMixtralDecoder
    cfg = MO.small_mixtral_cfg(n_layers=n_layers)
    sd = MO.seeded_state_dict(cfg, seed=seed, router_scale=4.0)
    dec = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=max_seq_len).enable_moe_batch()
    assert dec.moe_mxfp4 is False and dec.moe_fp8 is False
    if mxfp4:
        dec.enable_moe_mxfp4()
    return cfg, sd, dec


def test_solo_step_graph_and_eager_agree_and_the_switch_restores_16_bit():
    cfg, sd, dec = _decoder(mxfp4=False)
    x = _prompts((20,), seed=1)[0].to(DEV)
    base = dec.generate(x, max_new_tokens=6, return_logits=True)
    epoch = dec.cache_epoch
    assert dec.enable_moe_mxfp4() is dec and dec.moe_mxfp4 and dec.decode_format == "16bit" and dec.cache_epoch == epoch + 1 and dec.graph is None
    assert len(dec.w4moe) == dec.n_layers and dec.w4moe[0]["wgu"][0].shape == (E, 2 * I, D // 2) and dec.w4moe[0]["wgu"][1].shape == (E, 2 * I, D // 32)
    assert dec.w4moe[0]["wd"][0].shape == (E, D, I // 2) and dec.w4moe[0]["wd"][1].shape == (E, D, I // 32)
    with pytest.raises(ValueError, match="MXFP4 expert weights are on: call enable_moe_mxfp4\\(False\\) before enable_moe_fp8\\(\\)"):
        dec.enable_moe_fp8()
    runs = [dec.generate(x, max_new_tokens=6, return_logits=True, use_graph=g) for g in (True, False)]
    assert dec.graph is not None
    assert runs[0][0].tolist() == runs[1][0].tolist() and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][1][0], base[1][0])                              # step 0 is the prefill: 16-bit, untouched
    assert not torch.equal(runs[0][1][1:], base[1][1:])                        # (the MXFP4 expert products ran)
    epoch = dec.cache_epoch                                                    # (a prefill bumps it too)
    dec.enable_moe_mxfp4(False)
    assert dec.graph is None and dec.cache_epoch == epoch + 1
    again = dec.generate(x, max_new_tokens=6, return_logits=True)
    assert again[0].tolist() == base[0].tolist() and torch.equal(again[1], base[1])


@pytest.mark.parametrize("nb", [2, 4])
def test_few_requests_are_bit_for_bit_the_solo_mxfp4_step(nb):
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


def _compare_on_decidable_pairs(solo, outs, blogits, margins):
    """tests/test_gpu_moe_batch.py _compare_to_rounding's bar -- 2e-2 rel-L2 on the logits, a differing token only at a tie -- on the pairs
    (request, step >= 1) whose routing the fp32 oracle on the dequantised experts decides with margin >= 1e-2 up to that step and whose tokens
    so far agree.  Returns the number of pairs compared."""
    n = 0
    for b, (toks, logits) in enumerate(solo):
        assert torch.equal(blogits[0, b], logits[0]), b                       # step 0 is the prefill: identical
        for s in range(1, blogits.shape[0]):
            if outs[b][:s].tolist() != toks[0, :s].tolist() or margins[b][s - 1] < 1e-2:
                break
            n += 1
            r = rel(blogits[s, b], logits[s])
            print(f"request {b} step {s}: grouped against solo MXFP4 rel {r:.3e}, oracle routing margin {margins[b][s - 1]:.3e}")
            assert r < 2e-2, (b, s, r)
            if outs[b][s].item() != toks[0, s].item():
                ok, margin, dmax = token_tie_ok(blogits[s, b], logits[s])
                assert ok, (b, s, margin, dmax)
    return n


@pytest.mark.parametrize("nb", [8, 64])
def test_8_and_64_requests_match_solo_mxfp4_to_summation_order(nb):
    """The grouped skinny-M form against the solo MXFP4 step on the (request, step) pairs whose routing the fp32 oracle on the dequantised
    experts decides with margin >= 1e-2: the project's form-against-form bound (tests/test_gpu_moe_batch.py, tests/test_gpu_mxfp4.py), 2e-2
    rel-L2 on the logits (the forms differ by summation order only).  At least half of the checked pairs must be decidable: the cap that
    tests/test_moe_mxfp4_host.py holds on the CPU oracle alone."""
    cfg, sd, dec = _decoder(seed=X4.DEC_SEED)
    sd4 = X4.dequantised_state_dict(sd, cfg)
    ids = X4.DEC8_IDS if nb == 8 else tuple(range(64))
    xs = [X4.dec_prompt(i) for i in ids]
    check = list(range(8)) if nb == 8 else list(X4.DEC64_CHECK)
    outs, blogits = dec.generate_batch([x.to(DEV) for x in xs], max_new_tokens=X4.DEC_NEW, return_logits=True)
    assert dec.MOE_GEMM_BATCH <= nb <= dec.MOE_MXFP4_ROWS
    solo = _solo(dec, [xs[b] for b in check], X4.DEC_NEW)
    margins = [_oracle_step_margins(sd4, cfg, xs[b].float(), st[0].tolist()) for b, (st, _) in zip(check, solo)]
    n = _compare_on_decidable_pairs(solo, [outs[b] for b in check], blogits[:, check], margins)
    assert 2 * n >= len(check) * (X4.DEC_NEW - 1), (n, len(check))


def _dequantised_decoder(dec, cfg, sd):
    """A second decoder whose 16-bit expert weights are the dequantised MXFP4 copies E2M1 2^e of `dec` (exact in the element type)."""
    from videollama2_amd import _lib
    from videollama2_amd.decoder import HipMixtralDecoder
    d16 = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=dec.max_seq_len)
    for lw, w4 in zip(d16.w["layers"], dec.w4moe):
        for name in ("wgu", "wd"):
            q, s = w4[name]
            deq = torch.stack([M4.dequant(q[e], s[e]) for e in range(q.shape[0])]).to(DEV)
            lw[name].copy_(deq.to(_lib.elem_dtype()))
            assert torch.equal(lw[name].float(), deq)
    return d16


def test_mxfp4_step_against_the_16_bit_step_on_the_dequantised_weights():
    """The project's bound for this comparison (tests/test_gpu_mxfp4.py, tests/test_gpu_moe_fp8.py): 6e-3 rel-L2 on the logits, on the
    margin-filtered steps.  The 16-bit decoder steps teacher-forced on the MXFP4 decoder's own tokens and cache rows (its prefill would read the
    dequantised experts, the MXFP4 decoder's reads the original ones), so a step differs by the expert products' arithmetic alone."""
    cfg, sd, dec = _decoder(seed=X4.DEC_SEED)
    sd4 = X4.dequantised_state_dict(sd, cfg)
    d16 = _dequantised_decoder(dec, cfg, sd)
    n = 0
    for i in X4.DEC8_IDS[:4]:
        x = X4.dec_prompt(i)
        L = x.shape[0]
        t4, l4 = dec.generate(x.to(DEV), max_new_tokens=X4.DEC_NEW, return_logits=True)
        margins = _oracle_step_margins(sd4, cfg, x.float(), t4[0].tolist())
        for s in range(1, X4.DEC_NEW):
            if margins[s - 1] < 1e-2:
                break
            for li in range(dec.n_layers):
                d16.kcache[li].copy_(dec.kcache[li])
                d16.vcache[li].copy_(dec.vcache[li])
            d16.pos = L + s - 1
            l16 = d16.decode_step(t4[0, s - 1:s].to(torch.int32))
            r = rel(l4[s], l16)
            print(f"request {i} ({L} rows), step {s}: MXFP4 against dequantised 16-bit rel {r:.3e} (oracle routing margin {margins[s - 1]:.3e})")
            assert r < 6e-3, (L, s, r)
            n += 1
    assert 2 * n >= 4 * (X4.DEC_NEW - 1), n


def test_continuous_batcher_four_slots_equals_solo_mxfp4_with_a_sampled_request():
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
    with pytest.raises(RuntimeError, match="enable_moe_mxfp4: a ContinuousBatcher holds requests in flight"):
        dec.enable_moe_mxfp4(False)
    b.run()


def test_more_than_64_requests_are_refused_and_the_switch_off_restores_the_16_bit_batch():
    cfg, sd, dec = _decoder(max_seq_len=64, mxfp4=False)
    xs = [x.to(DEV) for x in _prompts((20, 1, 33), seed=3)]
    base = dec.generate_batch(xs, max_new_tokens=4, return_logits=True)
    dec.enable_moe_mxfp4()
    with pytest.raises(NotImplementedError, match="at most 64 sequences.*no tiled W4A16 grouped GEMM is built"):
        dec._ensure_batch(65)
    mx4 = dec.generate_batch(xs, max_new_tokens=4, return_logits=True)
    assert not torch.equal(mx4[1][1:], base[1][1:])
    dec.enable_moe_mxfp4(False)
    again = dec.generate_batch(xs, max_new_tokens=4, return_logits=True)
    assert [t.tolist() for t in again[0]] == [t.tolist() for t in base[0]] and torch.equal(again[1], base[1])
