"""MXFP4 (OCP MX v1.0: E2M1 elements, one E8M0 scale per 32) decode weights on MI355X: the kernels of csrc/k_mxfp4.h through the C ABI against
tests/mxfp4_oracle.py.  KERNEL error is asserted tight (the quantiser bit for bit, the conversion's 16-code table, the GEMV to fp32 summation
order, the multi-row GEMV and the skinny-M GEMM bit for bit against their single-row / 16-bit twins, every decode path against the solo decode
or the 16-bit kernels on the dequantised weights); FORMAT error (about 11 % per projection, the price of 4 bits) is reported, not bounded."""
import json
import os

import pytest
import torch

from oracle import vl2_oracle as O
from tests import mxfp4_oracle as M4
from tests.util import TOL_BF16_OUT, TOL_F32_OUT, rel, token_tie_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from videollama2_amd import _lib, ops as o
    _lib.load()
    return o


def bf(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).bfloat16()


def dequant_dev(q, s):
    """M4.dequant on the device: the 16-entry table from the specification, times 2^(s - 127); fp32, exact in bf16."""
    tab = torch.tensor([M4.e2m1_decode(c) for c in range(16)], dtype=torch.float32, device=q.device)
    codes = torch.stack([q & 15, q >> 4], dim=2).view(q.shape[0], -1).long()
    return tab[codes] * torch.exp2(s.float() - 127.0).repeat_interleave(32, dim=1)


def boundary_matrix(hi=2.0 ** 20):
    """Every E2M1 grid point, every midpoint and a point either side of it, at block scales 2^-12, 1 and `hi` (the block maximum 6 pins e);
    a zero block; a 1e-30 block; block maxima on and just past 4 * 2^k and 6 * 2^k."""
    grid = M4.E2M1_VALUES
    pts = list(grid)
    for a, b in zip(grid[:-1], grid[1:]):
        m = (a + b) / 2
        pts += [m, m - (b - a) / 8, m + (b - a) / 8]
    pts = [p for p in pts if p < 8]                                     # 29 points, all exact in bf16
    blk = torch.zeros(32)
    blk[:len(pts)] = torch.tensor(pts)
    blk[len(pts)] = 4.0                                                 # amax = 6, in [4, 8): e = 0 at scale 1
    rows = []
    for sc in (2.0 ** -12, 1.0, hi):
        rows.append(torch.cat([blk * sc, -blk * sc, torch.zeros(32), torch.randn(32, generator=torch.Generator().manual_seed(1)) * 1e-30]))
    edge = []
    for k in (-3, 0, 5):
        for top in (4.0, 4.03125, 3.984375, 6.0, 6.03125, 5.96875, 7.96875, 8.0):
            b = torch.randn(32, generator=torch.Generator().manual_seed(int(top * 64) + k)) * 2.0 ** k
            b[5] = -top * 2.0 ** k
            edge.append(b)
    edge = torch.cat(edge)
    rows.append(edge[:128]); rows.append(edge[128:256]); rows.append(edge[256:384]); rows.append(edge[384:512]); rows.append(edge[512:640]); rows.append(edge[640:768])
    return torch.stack(rows)


def _quantiser_cases(ops, elem):
    w = boundary_matrix(2.0 ** 20 if elem == torch.bfloat16 else 2.0 ** 12).to(elem)      # half ends at 65504: its large scale is 2^12
    q, s = ops.quant_mxfp4(w.to(DEV))
    qo, so = M4.quant_blocks(w)
    assert torch.equal(s.cpu(), so), (s.cpu(), so)
    assert torch.equal(q.cpu(), qo), f"{int((q.cpu() != qo).sum())} code bytes differ"
    big = (torch.randn(4096, 14336, generator=torch.Generator().manual_seed(3)) * 14336 ** -0.5).to(elem)
    q, s = ops.quant_mxfp4(big.to(DEV))
    qo, so = M4.quant_blocks(big)
    assert torch.equal(s.cpu(), so) and torch.equal(q.cpu(), qo)


def test_quantiser_on_device_matches_the_oracle_bit_for_bit(ops):
    _quantiser_cases(ops, torch.bfloat16)


def test_conversion_table_of_all_16_codes_and_the_nibble_order(ops):
    """Row n of q holds code n in the LOW nibble of byte 0 and code 15 - n in the HIGH nibble of byte 1 (k = 0 and k = 3); a one-hot x reads
    them back through the kernel's own conversion (v_cvt_scalef32_pk_bf16_fp4) at three scales."""
    N, K = 16, 64
    for sb in (127, 127 - 9, 127 + 14):
        q = torch.zeros(N, K // 2, dtype=torch.uint8)
        for n in range(N):
            q[n, 0] = n
            q[n, 1] = (15 - n) << 4
        s = torch.full((N, K // 32), sb, dtype=torch.uint8)
        for k, code_of in ((0, lambda n: n), (3, lambda n: 15 - n), (1, lambda n: 0)):
            x = torch.zeros(K)
            x[k] = 1.0
            y = ops.gemv_mxfp4(q.to(DEV), s.to(DEV), x.bfloat16().to(DEV), out_f32=True).cpu()
            want = torch.tensor([M4.e2m1_decode(code_of(n)) * 2.0 ** (sb - 127) for n in range(N)])
            assert torch.equal(y, want), (sb, k, y, want)
            assert torch.equal(y.double(), M4.gemv(q, s, x.bfloat16()))


GEMV_SHAPES = [("qkv", 6144, 4096, dict(rms=True, bias=True)), ("o", 4096, 4096, dict(res=True)),
               ("gate_up", 28672, 4096, dict(rms=True, swiglu=True)), ("down", 4096, 14336, dict(res=True)),
               ("lm_head", 32000, 4096, dict(norm_w=True, f32=True)), ("qwen2_down", 3584, 18944, dict(res=True))]


@pytest.mark.parametrize("name,N,K,kw", GEMV_SHAPES, ids=[s[0] for s in GEMV_SHAPES])
def test_gemv_mxfp4_at_decoder_shapes(ops, name, N, K, kw):
    """Against the fp64 oracle on the same codes and scales: fp32 summation order and, for a 16-bit output, its one rounding -- the bars of the
    fp8 GEMV of the same family (2e-4 fp32 out, 3e-3 16-bit out)."""
    w, x = bf(N, K, scale=K ** -0.5, seed=1), bf(K, seed=2)
    q, s = ops.quant_mxfp4(w.to(DEV))
    n_out = N // 2 if kw.get("swiglu") else N
    bias = torch.randn(n_out) if kw.get("bias") else None
    res = bf(n_out, seed=4) if kw.get("res") else None
    nw = (torch.rand(K) + 0.5) if kw.get("norm_w") else None
    y = ops.gemv_mxfp4(q, s, x.to(DEV), norm_w=None if nw is None else nw.to(DEV), eps=1e-5, res=None if res is None else res.to(DEV),
                       bias=None if bias is None else bias.to(DEV), swiglu=bool(kw.get("swiglu")), out_f32=bool(kw.get("f32")),
                       rms_plain=bool(kw.get("rms")))
    ref = M4.gemv(q.cpu(), s.cpu(), x, norm_w=nw, eps=1e-5, res=res, bias=bias, swiglu=bool(kw.get("swiglu")), rms=bool(kw.get("rms")))
    e = rel(y.double().cpu(), ref)
    print(f"[mxfp4] gemv {name}: rel-L2 to the fp64 oracle {e:.3e}")
    assert e < (2e-4 if kw.get("f32") else 3e-3), (name, e)


@pytest.mark.parametrize("name,N,K,kw", GEMV_SHAPES, ids=[s[0] for s in GEMV_SHAPES])
def test_gemv_batched_mxfp4_rows_equal_the_single_row_gemv(ops, name, N, K, kw):
    g = torch.Generator(device=DEV).manual_seed(N + 2 * K)
    q, s = ops.quant_mxfp4((torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).bfloat16())
    n_out = N // 2 if kw.get("swiglu") else N
    bias = torch.randn(n_out, generator=g, device=DEV) if kw.get("bias") else None
    nw = (torch.rand(K, generator=g, device=DEV) + 0.5) if kw.get("norm_w") else None
    common = dict(norm_w=nw, eps=1e-5, bias=bias, swiglu=bool(kw.get("swiglu")), out_f32=bool(kw.get("f32")), rms_plain=bool(kw.get("rms")))
    for MB in (2, 3, 4, 7):                                             # 7: a split launch (4 + 3; K = 14336 / 18944: fewer rows fit LDS)
        x = torch.randn(MB, K, generator=g, device=DEV).bfloat16()
        res = torch.randn(MB, n_out, generator=g, device=DEV).bfloat16() if kw.get("res") else None
        y = ops.gemv_batched_mxfp4(q, s, x, res=res, **common)
        for b in range(MB):
            y1 = ops.gemv_mxfp4(q, s, x[b], res=None if res is None else res[b], **common)
            assert torch.equal(y[b], y1), (name, MB, b)


SKINNY_SHAPES = [("qkv", 6144, 4096, dict(bias=True)), ("qwen2_qkv", 4608, 3584, dict(bias=True)), ("o", 4096, 4096, dict(res=True)),
                 ("gate_up", 28672, 4096, dict(swiglu=True)), ("down", 4096, 14336, dict(res=True)), ("qwen2_down", 3584, 18944, dict(res=True)),
                 ("f32", 32000, 4096, dict(f32=True))]


def _skinny_args(N, kw, M, seed):
    n_out = N // 2 if kw.get("swiglu") else N
    g = torch.Generator(device=DEV).manual_seed(seed)
    bias = torch.randn(n_out, generator=g, device=DEV) if kw.get("bias") else None
    res = torch.randn(M, n_out, generator=g, device=DEV).bfloat16() if kw.get("res") else None
    return dict(bias=bias, res=res, swiglu=bool(kw.get("swiglu")), out_f32=bool(kw.get("f32")))


@pytest.mark.parametrize("name,N,K,kw", SKINNY_SHAPES, ids=[s[0] for s in SKINNY_SHAPES])
def test_skinny_mxfp4_equals_skinny_on_dequantised_weights_and_rows_ignore_the_batch(ops, name, N, K, kw):
    """The kernel keeps the 16-bit skinny-M kernel's lane-to-k assignment: torch.equal with ops.gemm_skinny on dequant(q, s)."""
    g = torch.Generator(device=DEV).manual_seed(N + K)
    q, s = ops.quant_mxfp4((torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).bfloat16())
    wd = dequant_dev(q, s)
    assert torch.equal(wd[:64].cpu(), M4.dequant(q[:64], s[:64]))      # the device table against the oracle's dequantiser
    wb = wd.bfloat16()
    assert torch.equal(wb.float(), wd)                                 # the dequantised weights are exact in bf16
    for M in (5, 16, 33, 64):
        x = torch.randn(M, K, generator=g, device=DEV).bfloat16()
        a = _skinny_args(N, kw, M, seed=M + 1)
        y4 = ops.gemm_skinny_mxfp4(x, q, s, **a)
        y16 = ops.gemm_skinny(x, wb, **a)
        assert torch.equal(y4, y16), (name, M, int((y4 != y16).sum()))
    # rows do not depend on the batch: a row of an M = 5 call inside an M = 64 call
    x5 = torch.randn(5, K, generator=g, device=DEV).bfloat16()
    x64 = torch.randn(64, K, generator=g, device=DEV).bfloat16()
    x64[38:43] = x5
    a64 = _skinny_args(N, kw, 64, seed=9)
    a5 = dict(a64, res=None if a64["res"] is None else a64["res"][38:43].contiguous())
    assert torch.equal(ops.gemm_skinny_mxfp4(x5, q, s, **a5), ops.gemm_skinny_mxfp4(x64, q, s, **a64)[38:43]), name
    x80 = torch.randn(80, K, generator=g, device=DEV).bfloat16()      # 80 rows: the wrapper runs 64 + 16
    a80 = _skinny_args(N, kw, 80, seed=81)
    y80 = ops.gemm_skinny_mxfp4(x80, q, s, **a80)
    part = ops.gemm_skinny_mxfp4(x80[40:], q, s, **dict(a80, res=None if a80["res"] is None else a80["res"][40:]))
    assert torch.equal(part, y80[40:]), name


def test_mxfp4_kernels_in_the_fp16_build():
    """libvl2hip_f16.so: the quantiser reads half weights (bit for bit the oracle), the GEMV converts with v_cvt_scalef32_pk_f16_fp4 and takes
    half activations (against the oracle with elem = float16), the skinny-M kernel equals the half skinny-M kernel on the dequantised weights."""
    from videollama2_amd import _lib, ops
    _lib.set_elem("fp16")
    try:
        _quantiser_cases(ops, torch.float16)
        g = torch.Generator().manual_seed(11)
        w = (torch.randn(512, 4096, generator=g) * 0.02).half()
        q, s = ops.quant_mxfp4(w.to(DEV))
        x = torch.randn(4096, generator=g).half()
        y = ops.gemv_mxfp4(q, s, x.to(DEV), eps=1e-5, out_f32=True, rms_plain=True)
        assert rel(y.double().cpu(), M4.gemv(q.cpu(), s.cpu(), x, eps=1e-5, rms=True, elem=torch.float16)) < 2e-4
        ysw = ops.gemv_mxfp4(q, s, x.to(DEV), eps=1e-5, swiglu=True, rms_plain=True)
        assert ysw.dtype == torch.float16
        assert rel(ysw.double().cpu(), M4.gemv(q.cpu(), s.cpu(), x, eps=1e-5, rms=True, swiglu=True, elem=torch.float16)) < 3e-3
        xb = torch.randn(3, 4096, generator=g).half().to(DEV)
        yb = ops.gemv_batched_mxfp4(q, s, xb, eps=1e-5, rms_plain=True)
        assert all(torch.equal(yb[b], ops.gemv_mxfp4(q, s, xb[b], eps=1e-5, rms_plain=True)) for b in range(3))
        wh = dequant_dev(q, s).half()
        assert torch.equal(wh.float(), dequant_dev(q, s))
        xs = torch.randn(16, 4096, generator=g).half().to(DEV)
        assert torch.equal(ops.gemm_skinny_mxfp4(xs, q, s), ops.gemm_skinny(xs, wh))
    finally:
        _lib.set_elem("bf16")


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


def _load_dequantised(dec):
    """The decoder's 16-bit projections := its MXFP4 copies, dequantised (bf16 holds them exactly); lm_head is 16-bit in both arithmetics."""
    for lw, q4 in zip(dec.w["layers"], dec.w4["layers"]):
        for k in ("wqkv", "wo", "wgu", "wd"):
            lw[k].copy_(dequant_dev(*q4[k]).to(lw[k].dtype))
    dec._stage = None


@pytest.fixture(scope="module")
def dec7(ops):
    d = _decoder()
    d.enable_mxfp4_decode()
    yield d
    del d
    torch.cuda.empty_cache()


def test_mxfp4_decode_graph_equals_eager_and_format_error_is_reported(ops):
    """Mistral-7B widths, 2 layers, S = 300 prefill (16-bit), decode on the MXFP4 copies: the replayed hipGraph == the eager loop bit for bit
    (greedy and sampled); lm_head and the prefill stay 16-bit.  The FORMAT's error against the unquantised decoder is written down and printed,
    asserted only to be finite: random weights at 2 layers say little about a trained model."""
    dec = _decoder()
    x = (torch.randn(300, 4096, generator=torch.Generator().manual_seed(2)).bfloat16().float() * 0.5).to(DEV)
    t16, l16 = dec.generate(x, max_new_tokens=6, return_logits=True)
    e0 = dec.cache_epoch
    dec.enable_mxfp4_decode()
    assert dec.cache_epoch > e0 and dec.decode_format == "mxfp4" and dec.graph is None
    assert set(dec.w4) == {"layers"}                                  # no MXFP4 lm_head
    te, le = dec.generate(x, max_new_tokens=6, return_logits=True)
    tg, lg = dec.generate(x, max_new_tokens=6, return_logits=True, use_graph=True)
    assert te.tolist() == tg.tolist() and torch.equal(le, lg)
    assert torch.equal(le[0], l16[0])                                 # the prefill logits do not involve the MXFP4 copies
    smp = lambda graph: dec.generate(x, max_new_tokens=6, return_logits=True, use_graph=graph,
                                     sampler=(0.8, 40, 0.9, torch.Generator(device=DEV).manual_seed(7)))
    (ts, ls), (tsg, lsg) = smp(False), smp(True)
    assert ts.tolist() == tsg.tolist() and torch.equal(ls, lsg)
    rows = []
    for s in range(1, le.shape[0]):
        if te[0, :s].tolist() != t16[0, :s].tolist():
            break
        rows.append(dict(step=s, mxfp4_vs_unquantised_rel_l2=rel(le[s].cpu(), l16[s].cpu()), top1_equal=bool(te[0, s] == t16[0, s])))
    assert rows
    e_fmt = rows[0]["mxfp4_vs_unquantised_rel_l2"]
    print(f"[mxfp4] full-width 2-layer decode, MXFP4 weights vs unquantised: step-1 logits rel-L2 {e_fmt:.3e}, top-1 equal {rows[0]['top1_equal']}; "
          f"tokens mxfp4 {te[0].tolist()} unquantised {t16[0].tolist()}")
    out = os.path.join(os.environ.get("VL2_REPORT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles"),
                       "r11_mxfp4_parity.json")                        # the committed copy lives in profiles/: same seeds, same figures
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(dict(config="Mistral-7B widths, 2 layers, random weights, S=300 prefill on 16-bit weights, decode on MXFP4 copies (W4A16), lm_head 16-bit",
                   graph_equals_eager=True, rows=rows, tokens_mxfp4=te[0].tolist(), tokens_unquantised=t16[0].tolist()), open(out, "w"), indent=1)
    assert e_fmt == e_fmt and e_fmt != float("inf")                   # finite: the format's error is a report, not a bar
    dec.enable_mxfp4_decode(False)
    t16b, l16b = dec.generate(x, max_new_tokens=6, return_logits=True, use_graph=True)
    assert torch.equal(l16b, l16)                                     # switching it off restores the 16-bit bits
    del dec
    torch.cuda.empty_cache()


def test_mxfp4_decode_kernels_equal_16bit_kernels_on_dequantised_weights(ops):
    """One decode step from an identical cache: the MXFP4 projections against the 16-bit projections of the SAME decoder whose weights were
    replaced by the (bf16-exact) dequantised copies -- same products, fp32 summation order aside (the fp8 test's 6e-3)."""
    dec = _decoder(seed=6)
    dec.enable_mxfp4_decode()
    _load_dequantised(dec)                                            # BOTH runs prefill on the dequantised weights: identical caches
    x = (torch.randn(200, 4096, generator=torch.Generator().manual_seed(3)).bfloat16().float() * 0.5).to(DEV)
    t4, l4 = dec.generate(x, max_new_tokens=4, return_logits=True)
    dec.enable_mxfp4_decode(False)
    t16, l16 = dec.generate(x, max_new_tokens=4, return_logits=True)
    assert torch.equal(l4[0], l16[0])
    n = 1
    while n < l4.shape[0] and t4[0, :n].tolist() == t16[0, :n].tolist():
        e = rel(l4[n].cpu(), l16[n].cpu())
        print(f"[mxfp4] decode step {n}: MXFP4 kernels vs 16-bit kernels on dequantised weights rel-L2 {e:.2e}")
        assert e < 6e-3, (n, e)
        n += 1
    assert n >= 2
    # eight requests (the skinny-M step): track their solo decodes to rounding, and ARE the 16-bit skinny-M step on the dequantised weights
    dec.enable_mxfp4_decode()
    embeds = _embeds((200, 31, 77, 5, 129, 64, 1, 300), seed=9)
    assert len(embeds) >= dec.GEMM_BATCH
    solo = [dec.generate(e, max_new_tokens=4, return_logits=True) for e in embeds]
    t8, l8 = dec.generate_batch(embeds, max_new_tokens=4, return_logits=True)
    for b, (st, sl) in enumerate(solo):
        assert torch.equal(l8[0, b], sl[0])
        for s in range(1, l8.shape[0]):
            if t8[b][:s].tolist() != st[0, :s].tolist():
                break
            assert rel(l8[s, b], sl[s]) < 2e-2, (b, s)
            if t8[b][s].item() != st[0, s].item():
                ok, margin, dmax = token_tie_ok(l8[s, b], sl[s])
                assert ok, (b, s, margin, dmax)
    e8, el8 = dec.generate_batch(embeds, max_new_tokens=4, return_logits=True, use_graph=False)
    assert torch.equal(el8, l8)
    dec.enable_mxfp4_decode(False)
    t16, l16 = dec.generate_batch(embeds, max_new_tokens=4, return_logits=True)
    assert [t.tolist() for t in t16] == [t.tolist() for t in t8] and torch.equal(l16, l8)
    del dec
    torch.cuda.empty_cache()


def test_three_requests_equal_their_solo_mxfp4_decodes(dec7):
    embeds = _embeds((300, 77, 129), seed=8)
    solo = [dec7.generate(e, max_new_tokens=6, return_logits=True) for e in embeds]
    outs, blogits = dec7.generate_batch(embeds, max_new_tokens=6, return_logits=True)
    for b, (toks, logits) in enumerate(solo):
        assert outs[b].tolist() == toks[0].tolist(), b
        assert torch.equal(blogits[:, b], logits), b
    eager, elogits = dec7.generate_batch(embeds, max_new_tokens=6, return_logits=True, use_graph=False)
    assert [o.tolist() for o in eager] == [o.tolist() for o in outs] and torch.equal(elogits, blogits)


def test_toggling_mxfp4_16bit_fp8_selects_the_graph_of_the_weights(dec7):
    embeds = _embeds((90, 41, 150, 12, 60), seed=11)
    n = len(embeds)
    try:
        t4, l4 = dec7.generate_batch(embeds, max_new_tokens=3, return_logits=True)
        g4 = dec7.capture_batch_graph(n)
        assert torch.equal(l4, dec7.generate_batch(embeds, max_new_tokens=3, return_logits=True, use_graph=False)[1])
        with pytest.raises(ValueError, match=r"enable_mxfp4_decode\(False\)"):
            dec7.enable_fp8_decode()
        e0 = dec7.cache_epoch
        dec7.enable_mxfp4_decode(False)
        assert dec7.cache_epoch == e0 + 1 and dec7.capture_batch_graph(n) is not g4
        t16, l16 = dec7.generate_batch(embeds, max_new_tokens=3, return_logits=True)
        assert torch.equal(l16[0], l4[0]) and not torch.equal(l16[1], l4[1])
        dec7.enable_fp8_decode()
        assert dec7.decode_format == "fp8"
        with pytest.raises(ValueError, match=r"enable_fp8_decode\(False\)"):
            dec7.enable_mxfp4_decode()
        t8, l8 = dec7.generate_batch(embeds, max_new_tokens=3, return_logits=True)
        assert not torch.equal(l8[1], l4[1]) and not torch.equal(l8[1], l16[1])
        dec7.enable_fp8_decode(False)
        e1 = dec7.cache_epoch
        dec7.enable_mxfp4_decode()
        assert dec7.cache_epoch == e1 + 1 and dec7.capture_batch_graph(n) is not g4       # every toggle drops the captured graphs
        assert torch.equal(dec7.generate_batch(embeds, max_new_tokens=3, return_logits=True)[1], l4)
        # the single-sequence graph follows the switch too (five requests run the skinny-M step, so the solo decode is its own reference)
        solo = lambda graph: dec7.generate(embeds[0], max_new_tokens=3, return_logits=True, use_graph=graph)[1]
        s4 = solo(True)
        assert dec7.graph is not None and torch.equal(s4, solo(False))
        dec7.enable_mxfp4_decode(False)
        assert dec7.graph is None
        s16 = solo(True)
        assert torch.equal(s16, solo(False)) and torch.equal(s16[0], s4[0]) and not torch.equal(s16[1], s4[1])
    finally:
        dec7.enable_fp8_decode(False)
        dec7.enable_mxfp4_decode()


def test_continuous_batching_on_mxfp4_weights(dec7):
    """Staggered admission, early retirement and slot reuse: every request (greedy or sampled) equals its solo MXFP4 decode."""
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
    # a toggle with requests in flight: the next step runs every slot on the weights then selected
    b = ContinuousBatcher(dec7, max_slots=4)
    rid = [b.submit(embeds[1], max_new_tokens=4), b.submit(embeds[3], max_new_tokens=4)]
    b.step()
    e0 = dec7.cache_epoch
    dec7.enable_mxfp4_decode(False)
    b.step()
    dec7.enable_mxfp4_decode()
    assert dec7.cache_epoch == e0 + 2
    done = b.run()
    assert all(len(done[r]) == 4 for r in rid)


def test_qwen2_decoder_on_mxfp4(ops):
    """Qwen2 widths (q/k/v bias, K = 3584 / 18944): below GEMM_BATCH a request is its solo decode to the bit, from 5 on to rounding."""
    cfg = O.config_videollama2_1_7b_16f(16)
    dec = _decoder(seed=7, cfg=cfg)
    assert dec.V == 152064 and dec.w["layers"][0]["bqkv"] is not None
    dec.enable_mxfp4_decode()
    D = cfg["llm"]["hidden_size"]
    for lens in ((60, 130, 9), (60, 130, 9, 44, 87, 21)):
        embeds = _embeds(lens, seed=len(lens), D=D)
        solo = [dec.generate(e, max_new_tokens=4, return_logits=True) for e in embeds]
        toks, logits = dec.generate_batch(embeds, max_new_tokens=4, return_logits=True)
        for b in range(len(lens)):
            st, sl = solo[b]
            if len(lens) < dec.GEMM_BATCH:
                assert toks[b].tolist() == st[0].tolist() and torch.equal(logits[:, b], sl), b
                continue
            assert torch.equal(logits[0, b], sl[0])
            for s in range(1, logits.shape[0]):
                if toks[b][:s].tolist() != st[0, :s].tolist():
                    break
                assert rel(logits[s, b], sl[s]) < 2e-2, (b, s)
    del dec
    torch.cuda.empty_cache()
