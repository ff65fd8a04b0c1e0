"""Batched and continuous decoding on the fp8 decode weights (W8A16) on MI355X.  Kernels (include/vl2hip.h vl2_gemm_skinny_fp8 /
vl2_gemv_batched_fp8): the skinny-M fp8 GEMM is bit for bit the 16-bit skinny-M GEMM on the dequantised weights and its rows do not depend on
the batch; the multi-row fp8 GEMV is, row by row, the single-row fp8 GEMV.  Decoder and serving at Mistral-7B widths (2 layers): generate_batch,
graph replay, toggling the weights under captured graphs, the continuous batcher with greedy and sampled requests, the Qwen2 decoder; the
fp16 build."""
import pytest
import torch

from oracle import fp8_oracle as F8
from oracle import vl2_oracle as O
from tests.util import TOL_BF16_OUT, TOL_F32_OUT, rel, token_tie_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib, ops as o
    _lib.load()
    return o


def _lut():
    return torch.tensor([F8.e4m3fn_decode(c) for c in range(256)], dtype=torch.float32, device=DEV)


def dequant(q, sc):
    """F8.dequant on the device (a table of the 256 codes, from the specification): q * 2^e in fp32, exact in bf16 / half."""
    return _lut()[q.long()] * sc[:, None]


def weights(ops, N, K, seed, elem=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(elem)
    q, sc = ops.quant_fp8(w)
    return q, sc


def acts(M, K, seed, elem=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(M, K, generator=g, device=DEV).to(elem)


def ref_epilogue(y, bias=None, res=None, swiglu=False):
    if swiglu:
        y = y.view(y.shape[0], -1, 2, 32)
        y = (torch.nn.functional.silu(y[:, :, 0]) * y[:, :, 1]).reshape(y.shape[0], -1)
    if bias is not None:
        y = y + bias
    if res is not None:
        y = y + res.float()
    return y


SHAPES = [("qkv", 6144, 4096, dict(bias=True)), ("qwen2_qkv", 4608, 3584, dict(bias=True)), ("o", 4096, 4096, dict(res=True)),
          ("gate_up", 28672, 4096, dict(swiglu=True)), ("down", 4096, 14336, dict(res=True)), ("lm_head", 32000, 4096, dict(f32=True)),
          ("qwen2_lm_head", 152064, 3584, dict(f32=True))]


def _skinny_args(N, K, kw, M, seed):
    n_out = N // 2 if kw.get("swiglu") else N
    g = torch.Generator(device=DEV).manual_seed(seed)
    bias = torch.randn(n_out, generator=g, device=DEV) if kw.get("bias") else None
    res = torch.randn(M, n_out, generator=g, device=DEV).bfloat16() if kw.get("res") else None
    return dict(bias=bias, res=res, swiglu=bool(kw.get("swiglu")), out_f32=bool(kw.get("f32")))


@pytest.mark.parametrize("name,N,K,kw", SHAPES, ids=[s[0] for s in SHAPES])
def test_skinny_fp8_equals_skinny_on_dequantised_weights(ops, name, N, K, kw):
    q, sc = weights(ops, N, K, seed=N + K)
    wd = dequant(q, sc)
    if N <= 6144:                                                     # the device table against the oracle's dequantiser
        assert torch.equal(wd[:64].cpu(), F8.dequant(q[:64].cpu(), sc[:64].cpu()))
    wb = wd.bfloat16()
    assert torch.equal(wb.float(), wd)                               # the dequantised weights are exact in bf16
    for M in (5, 16, 33, 64):
        x = acts(M, K, seed=M)
        a = _skinny_args(N, K, kw, M, seed=M + 1)
        y8 = ops.gemm_skinny_fp8(x, q, sc, **a)
        y16 = ops.gemm_skinny(x, wb, **a)
        assert torch.equal(y8, y16), (name, M, int((y8 != y16).sum()))
        ref = ref_epilogue(x.float() @ wd.T, a["bias"], a["res"], a["swiglu"])
        e = rel(y8.float(), ref)
        assert e < (TOL_F32_OUT if a["out_f32"] else TOL_BF16_OUT), (name, M, e)


@pytest.mark.parametrize("name,N,K,kw", [SHAPES[0], SHAPES[3], SHAPES[4], SHAPES[5]], ids=["qkv", "gate_up", "down", "lm_head"])
def test_skinny_fp8_rows_do_not_depend_on_the_batch(ops, name, N, K, kw):
    q, sc = weights(ops, N, K, seed=3 * N + K)
    row = acts(1, K, seed=77)
    x5, x64 = acts(5, K, seed=5), acts(64, K, seed=64)
    x5[2], x64[40] = row[0], row[0]
    a64 = _skinny_args(N, K, kw, 64, seed=9)
    a5 = dict(a64, res=None if a64["res"] is None else a64["res"][38:43].contiguous())
    y5 = ops.gemm_skinny_fp8(x5, q, sc, **a5)
    y64 = ops.gemm_skinny_fp8(x64, q, sc, **a64)
    assert torch.equal(y5[2], y64[40]), name
    # 80 rows: the wrapper runs 64 + 16; the same rows as 40 + 40
    x80 = acts(80, K, seed=80)
    a80 = _skinny_args(N, K, kw, 80, seed=81)
    y80 = ops.gemm_skinny_fp8(x80, q, sc, **a80)
    for r0, r1 in ((0, 40), (40, 80)):
        part = ops.gemm_skinny_fp8(x80[r0:r1], q, sc, **dict(a80, res=None if a80["res"] is None else a80["res"][r0:r1]))
        assert torch.equal(part, y80[r0:r1]), (name, r0)


GEMV_SHAPES = [("qkv", 6144, 4096, dict(rms=True, bias=True)), ("o", 4096, 4096, dict(res=True)),
               ("gate_up", 28672, 4096, dict(rms=True, swiglu=True)), ("down", 4096, 14336, dict(res=True)),
               ("lm_head", 32000, 4096, dict(norm_w=True, f32=True)), ("qwen2_down", 3584, 18944, dict(res=True))]


@pytest.mark.parametrize("name,N,K,kw", GEMV_SHAPES, ids=[s[0] for s in GEMV_SHAPES])
def test_gemv_batched_fp8_rows_equal_the_single_row_gemv(ops, name, N, K, kw):
    q, sc = weights(ops, N, K, seed=N + 2 * K)
    n_out = N // 2 if kw.get("swiglu") else N
    g = torch.Generator(device=DEV).manual_seed(N)
    bias = torch.randn(n_out, generator=g, device=DEV) if kw.get("bias") else None
    nw = (torch.rand(K, generator=g, device=DEV) + 0.5) if kw.get("norm_w") else None
    common = dict(norm_w=nw, eps=1e-5, bias=bias, swiglu=bool(kw.get("swiglu")), out_f32=bool(kw.get("f32")), rms_plain=bool(kw.get("rms")))
    for MB in (1, 2, 3, 4, 7):
        x = acts(MB, K, seed=MB + K)
        res = torch.randn(MB, n_out, generator=g, device=DEV).bfloat16() if kw.get("res") else None
        y = ops.gemv_batched_fp8(q, sc, x, res=res, **common)
        for b in range(MB):
            y1 = ops.gemv_fp8(q, sc, x[b], res=None if res is None else res[b], **common)
            assert torch.equal(y[b], y1), (name, MB, b)
    ref = F8.gemv(q.cpu(), sc.cpu(), x[6].cpu(), norm_w=None if nw is None else nw.cpu(), eps=1e-5, res=None if res is None else res[6].cpu(),
                  bias=None if bias is None else bias.cpu(), swiglu=bool(kw.get("swiglu")), rms=bool(kw.get("rms")))
    e = rel(y[6].float().cpu(), ref)
    assert e < (2e-4 if kw.get("f32") else TOL_BF16_OUT), (name, e)


# ---------------------------------------------------------------------------------------------------------------------------------------
# decoder and serving
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


def _decoder(seed=5, cfg=None):
    from videollama2_amd.decoder import HipMistralDecoder
    if cfg is None:
        cfg = O.config_videollama2_7b(16)
    cfg["llm"]["num_hidden_layers"] = 2
    return HipMistralDecoder(cfg, O.seeded_state_dict(cfg, seed, only=_keep), DEV, max_seq_len=512)


def _embeds(lens, seed, D=4096):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, D, generator=g) * 0.5).bfloat16().to(DEV) for n in lens]


@pytest.fixture(scope="module")
def dec7(ops):
    d = _decoder()
    d.enable_fp8_decode()
    yield d
    del d
    torch.cuda.empty_cache()


def _check_to_rounding(toks, logits, solo, b):
    """Row b of a batched run against its solo decode (toks / logits of generate): rel < 2e-2 while the tokens agree, a differing token only
    on a tie."""
    st, sl = solo
    assert torch.equal(logits[0, b], sl[0])                           # step 0 is the prefill
    for s in range(1, logits.shape[0]):
        if toks[b][:s].tolist() != st[0, :s].tolist():
            break
        assert rel(logits[s, b], sl[s]) < 2e-2, (b, s)
        if toks[b][s].item() != st[0, s].item():
            ok, margin, dmax = token_tie_ok(logits[s, b], sl[s])
            assert ok, (b, s, margin, dmax)


def test_four_requests_equal_their_solo_fp8_decodes(dec7):
    embeds = _embeds((300, 77, 129, 1), seed=8)
    solo = [dec7.generate(e, max_new_tokens=6, return_logits=True) for e in embeds]
    outs, blogits = dec7.generate_batch(embeds, max_new_tokens=6, return_logits=True)
    for b, (toks, logits) in enumerate(solo):
        assert outs[b].tolist() == toks[0].tolist(), b
        assert torch.equal(blogits[:, b], logits), b
    eager, elogits = dec7.generate_batch(embeds, max_new_tokens=6, return_logits=True, use_graph=False)
    assert [o.tolist() for o in eager] == [o.tolist() for o in outs] and torch.equal(elogits, blogits)


def test_eight_requests_skinny_path_equal_16bit_kernels_on_dequantised_weights(ops):
    dec = _decoder(seed=6)
    dec.enable_fp8_decode()
    for lw, q8 in zip(dec.w["layers"], dec.w8["layers"]):           # every run prefills on the dequantised weights: identical caches
        for k in ("wqkv", "wo", "wgu", "wd"):
            lw[k].copy_(dequant(*q8[k]).to(lw[k].dtype))
    dec.w["lm_head"].copy_(dequant(*dec.w8["lm_head"]).to(dec.w["lm_head"].dtype))
    dec._stage = None
    embeds = _embeds((200, 31, 77, 5, 129, 64, 1, 300), seed=9)
    assert len(embeds) >= dec.GEMM_BATCH
    solo = [dec.generate(e, max_new_tokens=4, return_logits=True) for e in embeds]
    t8, l8 = dec.generate_batch(embeds, max_new_tokens=4, return_logits=True)
    for b in range(len(embeds)):
        _check_to_rounding(t8, l8, solo[b], b)
    e8, el8 = dec.generate_batch(embeds, max_new_tokens=4, return_logits=True, use_graph=False)
    assert torch.equal(el8, l8)
    dec.enable_fp8_decode(False)
    t16, l16 = dec.generate_batch(embeds, max_new_tokens=4, return_logits=True)
    assert [t.tolist() for t in t16] == [t.tolist() for t in t8]
    assert torch.equal(l16, l8)
    # more than 64 requests: the fp8 skinny kernel in calls of at most 64 rows; a row keeps its bits
    dec.enable_fp8_decode()
    many = _embeds([17 + (7 * i) % 50 for i in range(70)], seed=10)
    tm, lm = dec.generate_batch(many, max_new_tokens=2, return_logits=True)
    t64, l64 = dec.generate_batch(many[:64], max_new_tokens=2, return_logits=True)
    assert torch.equal(lm[:, :64], l64)
    t6, l6 = dec.generate_batch(many[64:], max_new_tokens=2, return_logits=True)
    assert torch.equal(lm[:, 64:], l6)
    del dec
    torch.cuda.empty_cache()


def test_toggling_fp8_selects_the_graph_of_the_weights(dec7):
    embeds = _embeds((90, 41, 150, 12, 60), seed=11)
    dec7.enable_fp8_decode(False)
    try:
        t16, l16 = dec7.generate_batch(embeds, max_new_tokens=3, return_logits=True)            # captures the 16-bit batch graph
        g16 = dec7.capture_batch_graph(len(embeds))
        dec7.enable_fp8_decode()
        assert dec7.capture_batch_graph(len(embeds)) is not g16
        tg, lg = dec7.generate_batch(embeds, max_new_tokens=3, return_logits=True)
        te, le = dec7.generate_batch(embeds, max_new_tokens=3, return_logits=True, use_graph=False)
        assert torch.equal(lg, le)                                    # the replayed step is the fp8 step
        assert not torch.equal(lg[1], l16[1])
        dec7.enable_fp8_decode(False)
        assert dec7.capture_batch_graph(len(embeds)) is not g16       # every toggle drops the captured batch graphs
        t16b, l16b = dec7.generate_batch(embeds, max_new_tokens=3, return_logits=True)
        assert torch.equal(l16b, l16)
    finally:
        dec7.enable_fp8_decode()


def test_continuous_batching_on_fp8_weights(dec7):
    from videollama2_amd.serving import ContinuousBatcher
    embeds = _embeds((120, 33, 200, 7, 64, 150), seed=12)
    samp = [dict(do_sample=True, temperature=1.2, top_k=30, top_p=0.85), None, dict(do_sample=True, temperature=0.7, top_k=0, top_p=0.9), None,
            None, dict(do_sample=True, temperature=0.9)]
    n_new = [7, 3, 6, 4, 5, 6]
    seed = lambda i: torch.Generator(device=DEV).manual_seed(200 + i)

    def solo(i):
        s = samp[i]
        sampler = None if s is None else (s["temperature"], s.get("top_k", 50), s.get("top_p", 1.0), seed(i))
        return dec7.generate(embeds[i], max_new_tokens=n_new[i], sampler=sampler, return_logits=True)

    solos = [solo(i) for i in range(6)]
    for use_graph in (True, False):
        b = ContinuousBatcher(dec7, max_slots=4, use_graph=use_graph)
        sub = lambda i: b.submit(embeds[i], max_new_tokens=n_new[i], **(dict(samp[i], generator=seed(i)) if samp[i] else {}))
        rid = [sub(0), sub(1)]
        b.step()
        rid += [sub(2), sub(3)]
        b.step(); b.step(); b.step()
        rid += [sub(4), sub(5)]
        done = b.run()
        assert [done[r].tolist() for r in rid] == [s[0][0].tolist() for s in solos], use_graph
    # 8 slots (the skinny-M fp8 step once 5 or more are occupied): greedy requests equal their solo decode to rounding
    embeds8 = _embeds((50, 80, 20, 130, 64, 9, 100, 40), seed=13)
    solo8 = [dec7.generate(e, max_new_tokens=5, return_logits=True) for e in embeds8]
    b = ContinuousBatcher(dec7, max_slots=8)
    rid = [b.submit(e, max_new_tokens=5) for e in embeds8]
    done = b.run()
    for i, r in enumerate(rid):
        toks, sl = solo8[i]
        got = done[r].tolist()
        for s in range(5):
            if got[s] != toks[0, s].item():
                top2 = sl[s].float().topk(2).values
                assert (top2[0] - top2[1]).item() < 4e-2 * sl[s].abs().max().item(), (i, s)   # a near-tie the rounding may decide
                break


def test_qwen2_decoder_batched_fp8(ops):
    cfg = O.config_videollama2_1_7b_16f(16)
    dec = _decoder(seed=7, cfg=cfg)
    assert dec.V == 152064 and dec.w["layers"][0]["bqkv"] is not None
    dec.enable_fp8_decode()
    D = cfg["llm"]["hidden_size"]
    for lens in ((60, 130, 9), (60, 130, 9, 44, 87, 21)):
        embeds = _embeds(lens, seed=len(lens), D=D)
        solo = [dec.generate(e, max_new_tokens=4, return_logits=True) for e in embeds]
        toks, logits = dec.generate_batch(embeds, max_new_tokens=4, return_logits=True)
        for b in range(len(lens)):
            if len(lens) < dec.GEMM_BATCH:
                assert toks[b].tolist() == solo[b][0][0].tolist() and torch.equal(logits[:, b], solo[b][1]), b
            else:
                _check_to_rounding(toks, logits, solo[b], b)
    del dec
    torch.cuda.empty_cache()


def test_fp8_batch_kernels_in_the_fp16_build():
    from videollama2_amd import _lib, ops
    _lib.set_elem("fp16")
    try:
        for N, K, kw in ((6144, 4096, dict()), (28672, 4096, dict(swiglu=True)), (32000, 4096, dict(out_f32=True))):
            q, sc = weights(ops, N, K, seed=N, elem=torch.float16)
            wh = dequant(q, sc).half()
            x = acts(16, K, seed=3, elem=torch.float16)
            y8 = ops.gemm_skinny_fp8(x, q, sc, **kw)
            y16 = ops.gemm_skinny(x, wh, **kw)
            assert y8.dtype == y16.dtype
            assert rel(y8.float(), y16.float()) < (TOL_F32_OUT if kw.get("out_f32") else TOL_BF16_OUT), (N, K)
            xb = acts(3, K, seed=4, elem=torch.float16)
            g8 = ops.gemv_batched_fp8(q, sc, xb, eps=1e-5, rms_plain=True, **kw)
            g16 = ops.gemv_batched(wh, xb, norm_w=torch.ones(K, device=DEV), eps=1e-5, **kw)
            assert rel(g8.float(), g16.float()) < (TOL_F32_OUT if kw.get("out_f32") else TOL_BF16_OUT), (N, K)
    finally:
        _lib.set_elem("bf16")
