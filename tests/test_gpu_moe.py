"""VideoLLaMA2-8x7B's sparse MoE block on the device (csrc/k_moe.h): routing tables, grouped GEMMs, a full-width MoE prefill against the
fp32 oracle (tests/moe_oracle.py), the decode step and its graph, and the prefill captured into a graph (no host synchronisation)."""
import pytest
import torch

from tests import moe_oracle as MO
from tests.util import TOL_BF16_OUT, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


def _bf(t):
    return t.to(device=DEV, dtype=torch.bfloat16).contiguous()


def _tables(ids, E, BM=128):
    """The routing tables recomputed in torch from the kernel's expert ids (ascending token order inside an expert)."""
    S, k = ids.shape
    ids = ids.cpu().long()
    counts = torch.stack([(ids == e).any(1).sum() for e in range(E)]).int()
    padded = (counts + BM - 1) // BM * BM
    offs = torch.cat([torch.zeros(1, dtype=torch.int64), padded.cumsum(0)]).int()
    P = (S * k + E * (BM - 1) + BM - 1) // BM * BM
    gather = torch.full((P,), -1, dtype=torch.int32)
    inv = torch.empty((S, k), dtype=torch.int32)
    for e in range(E):
        tok, slot = torch.where(ids == e)
        rows = offs[e] + torch.arange(tok.numel())
        gather[rows] = tok.int()
        inv[tok, slot] = rows.int()
    return counts, offs, gather, inv


def _route_ref(x, wr, k, eps):
    h = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)
    return MO.route(h, wr.float(), k)


@pytest.mark.parametrize("S", [1, 7, 64, 945, 1621])
def test_route_tables(S):
    from videollama2_amd import ops
    torch.manual_seed(S)
    D, E, k, eps = 4096, 8, 2, 1e-5
    x = _bf(torch.randn(S, D))
    wr = _bf(torch.randn(E, D) * D ** -0.5 * 4).float()
    r = ops.moe_route(x, wr, k, eps)
    torch.cuda.synchronize()
    rid, rw, probs = _route_ref(x, wr, k, eps)
    ok = MO.margins(probs, k) > 1e-3
    assert torch.equal(r["ids"].long()[ok], rid[ok])
    assert (r["wts"][ok] - rw[ok]).abs().max().item() <= 1e-5
    counts, offs, gather, inv = _tables(r["ids"], E)
    assert torch.equal(r["counts"].cpu(), counts) and torch.equal(r["offs"].cpu(), offs)
    assert torch.equal(r["gather"].cpu(), gather) and torch.equal(r["inv"].cpu(), inv)
    live = gather >= 0
    assert torch.equal(r["xg"][live.to(DEV)], x[gather[live].long().to(DEV)])


def test_route_all_tokens_to_two_experts():
    from videollama2_amd import ops
    torch.manual_seed(3)
    S, D, E, k = 300, 4096, 8, 2
    x = _bf(torch.rand(S, D) + 0.1)                           # positive rows
    wr = torch.full((E, D), -0.01)
    wr[0], wr[1] = 0.02, 0.015
    r = ops.moe_route(x, _bf(wr).float(), k, 1e-5)
    torch.cuda.synchronize()
    assert (r["ids"][:, 0] == 0).all() and (r["ids"][:, 1] == 1).all()
    assert r["counts"].cpu().tolist() == [S, S] + [0] * 6
    counts, offs, gather, inv = _tables(r["ids"], E)
    assert torch.equal(r["offs"].cpu(), offs) and torch.equal(r["gather"].cpu(), gather) and torch.equal(r["inv"].cpu(), inv)


def _grouped_case(S, D, I, E, k, seed, two_experts=False):
    from videollama2_amd import ops
    torch.manual_seed(seed)
    x = _bf(torch.randn(S, D))
    wr = torch.randn(E, D) * D ** -0.5 * 4
    if two_experts:
        x = _bf(torch.rand(S, D) + 0.1)
        wr = torch.full((E, D), -0.01); wr[0], wr[1] = 0.02, 0.015
    wgu = _bf(torch.randn(E, 2 * I, D) * D ** -0.5)
    wd = _bf(torch.randn(E, D, I) * I ** -0.5)
    r = ops.moe_route(x, _bf(wr).float(), k, 1e-5)
    a = ops.moe_gemm(r["xg"], wgu, r, S, k, swiglu=True, row_norm=r["rn"], eps=1e-5)
    y = ops.moe_gemm(a, wd, r, S, k)
    return x, wgu, wd, r, a, y


@pytest.mark.parametrize("S,D,I,E,k,two", [(945, 4096, 14336, 8, 2, False), (1, 4096, 14336, 8, 2, False), (7, 4096, 14336, 8, 2, False),
                                           (300, 4096, 14336, 8, 2, True), (64, 256, 512, 8, 2, False), (64, 256, 512, 16, 4, False)])
def test_grouped_gemm_equals_dense_gemm_per_expert(S, D, I, E, k, two):
    """Every expert's rows of the grouped gate/up (+SwiGLU) and down equal ops.gemm on the gathered rows forced to the same 16x16x32
    tile family -- bit for bit -- and the fp32 product to TOL_BF16_OUT."""
    from videollama2_amd import ops
    x, wgu, wd, r, a, y = _grouped_case(S, D, I, E, k, seed=S + E, two_experts=two)
    torch.cuda.synchronize()
    counts, offs = r["counts"].cpu().tolist(), r["offs"].cpu().tolist()
    for e in range(E):
        n = counts[e]
        if n == 0:
            continue
        rows = slice(offs[e], offs[e] + n)
        xe = r["xg"][rows].contiguous()
        ad = ops.gemm(xe, wgu[e], swiglu=True, norm=(ops.NORM_RMS, r["rn"][rows].contiguous(), 1e-5, None), mfma16=True)
        assert torch.equal(a[rows], ad), f"gate/up expert {e}"
        yd = ops.gemm(a[rows].contiguous(), wd[e], mfma16=True)
        assert torch.equal(y[rows], yd), f"down expert {e}"
        h = xe.float() * r["rn"][rows, 1:2]
        g, u = h @ wgu[e].float().view(-1, 2, 32, D)[:, 0].reshape(-1, D).T, h @ wgu[e].float().view(-1, 2, 32, D)[:, 1].reshape(-1, D).T
        assert rel(a[rows], torch.nn.functional.silu(g) * u) < TOL_BF16_OUT
        assert rel(y[rows], a[rows].float() @ wd[e].float().T) < TOL_BF16_OUT


def _full_width_sd(n_layers, seed=5, vocab=32000):
    """Seeded bf16 weights of a full-width Mixtral decoder (D 4096, I 14336, 8 experts, top 2) generated on the device."""
    D, I, E, nh, nkv, hd = 4096, 14336, 8, 32, 8, 128
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g, device=DEV)
    sd = {"model.embed_tokens.weight": (0.5 * rn(vocab, D)).bfloat16(), "model.norm.weight": (1 + 0.1 * rn(D)).bfloat16(),
          "lm_head.weight": (rn(vocab, D) * D ** -0.5).bfloat16()}
    for i in range(n_layers):
        p = f"model.layers.{i}."
        sd.update({p + "self_attn.q_proj.weight": (rn(nh * hd, D) * D ** -0.5).bfloat16(),
                   p + "self_attn.k_proj.weight": (rn(nkv * hd, D) * D ** -0.5).bfloat16(),
                   p + "self_attn.v_proj.weight": (rn(nkv * hd, D) * D ** -0.5).bfloat16(),
                   p + "self_attn.o_proj.weight": (rn(D, nh * hd) * D ** -0.5).bfloat16(),
                   p + "input_layernorm.weight": (1 + 0.1 * rn(D)).bfloat16(), p + "post_attention_layernorm.weight": (1 + 0.1 * rn(D)).bfloat16(),
                   p + "mlp.gate.weight": (rn(E, D) * D ** -0.5 * 4).bfloat16(),
                   p + "mlp.experts.gate_up_proj": (rn(E, 2 * I, D) * D ** -0.5).bfloat16(),
                   p + "mlp.experts.down_proj": (rn(E, D, I) * I ** -0.5).bfloat16()})
    cfg = dict(llm=dict(family="mixtral", hidden_size=D, intermediate_size=I, num_hidden_layers=n_layers, num_attention_heads=nh,
                        num_key_value_heads=nkv, head_dim=hd, vocab_size=vocab, rms_norm_eps=1e-5, rope_theta=1e6,
                        num_local_experts=E, num_experts_per_tok=2))
    return cfg, sd


def test_full_width_moe_block_against_fp32_oracle():
    """One full-width MoE block (route, grouped gate/up + SwiGLU, grouped down, combine) at S = 945 on the same bf16 x1 as the oracle."""
    from videollama2_amd.decoder import HipMixtralDecoder
    cfg, sd = _full_width_sd(1)
    dec = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=1024)
    torch.manual_seed(1)
    S = 945
    x1 = (0.5 * torch.randn(S, 4096, device=DEV)).bfloat16()
    rn = torch.empty((S, 2), dtype=torch.float32, device=DEV)
    out = dec.moe_block(dec.w["layers"][0], x1.clone(), rn)
    torch.cuda.synchronize()
    sdf = {k: v.float() for k, v in sd.items() if k.startswith("model.layers.")}
    ref = x1.float() + MO.moe_block(sdf, cfg, 0, x1.float(), ids=dec.last_route["ids"], follow_below=1e-3)
    assert rel(out, ref) < TOL_BF16_OUT
    want_rstd = torch.rsqrt(out.float().pow(2).mean(-1) + 1e-5)
    assert rel(rn[:, 1], want_rstd) < 1e-5 and (rn[:, 0] == 0).all()


@pytest.mark.parametrize("n_layers", [1, 4])
def test_full_width_moe_prefill_against_fp32_oracle(n_layers):
    """Full-width Mixtral layers (attention + MoE) in prefill against the fp32 oracle.  The router input here carries the attention's bf16
    error (~1e-3 relative, i.e. a few 1e-3 on logits of size ~4), so a row whose fp32 top-k margin is below 2e-2 is undecidable at this
    precision: the oracle follows the kernel's choice there (and only there).  Criterion of the dense path's full-width parity tests
    (test_gpu_stages.stage_ok): rel-L2 <= max(2 x the floor of the same oracle run in bf16, 4e-3).  The MoE block on identical inputs is
    held to TOL_BF16_OUT with the 1e-3 rule (test_full_width_moe_block_against_fp32_oracle)."""
    from videollama2_amd.decoder import HipMixtralDecoder
    cfg, sd = _full_width_sd(n_layers)
    S = 945 if n_layers == 1 else 256
    dec = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=1024)
    routes = []
    orig = dec.moe_block
    dec.moe_block = lambda lw, x1, rn: (lambda out: (routes.append(dec.last_route["ids"].clone()), out)[1])(orig(lw, x1, rn))
    torch.manual_seed(1)
    x = (0.5 * torch.randn(S, 4096, device=DEV)).bfloat16()
    dec.prefill(x)
    torch.cuda.synchronize()
    from oracle import vl2_oracle as O
    outs = {}
    followed_rows = [0, 0]
    orig_block = MO.moe_block

    def counting_block(sd_, cfg_, i_, x1_, ids=None, follow_below=None):
        if x1_.dtype == torch.float32:              # count on the fp32 pass: rows whose routing the oracle takes from the kernel
            l_ = cfg_["llm"]
            h = O.rmsnorm(x1_, sd_[f"model.layers.{i_}.post_attention_layernorm.weight"], l_["rms_norm_eps"])
            rid, _, probs = MO.route(h, sd_[f"model.layers.{i_}.mlp.gate.weight"], l_["num_experts_per_tok"])
            low = MO.margins(probs, l_["num_experts_per_tok"]) < follow_below
            followed_rows[0] += int(low.sum())
            same = (rid.sort(1).values == ids.long().sort(1).values).all(1)
            followed_rows[1] += int((low & ~same).sum())
        return orig_block(sd_, cfg_, i_, x1_, ids, follow_below)

    MO.moe_block = counting_block
    for dt in (torch.float32, torch.bfloat16):
        sdt = {k: v.to(dt) for k, v in sd.items() if k.startswith("model.layers.")}
        cos, sin = O.rope_cos_sin(cfg, torch.arange(S), dt)
        xo = x.to(dt)
        for i in range(n_layers):
            xo, _ = MO.mixtral_layer(sdt, cfg, i, xo, cos.to(DEV), sin.to(DEV), ids=routes[i], follow_below=2e-2)
        outs[dt] = xo.float()
        del sdt
    MO.moe_block = orig_block
    err, floor = rel(dec.last_hidden, outs[torch.float32]), rel(outs[torch.bfloat16], outs[torch.float32])
    followed, disagree = followed_rows
    print(f"{n_layers} layer(s), S = {S}: rel-L2 {err:.3e}, bf16 floor {floor:.3e}; rows under the follow rule {followed} of {S * n_layers}, "
          f"of them routed differently from the fp32 oracle's own choice {disagree}")
    # With this seeded router (softmax of logits ~ N(0, 4^2)) about 30 % of the rows have a top-2 / top-3 gap below 2e-2, so the rule
    # REACHES many rows; what would hide a kernel that routes near-ties wrongly is the rows where the kernel's choice differs from the
    # oracle's own fp32 choice.  Measured 6 of 945 (1 layer) and 5 of 1024 (4 layers); bound: 1 %.
    assert disagree <= 0.01 * S * n_layers
    assert err <= max(2.0 * floor, 4e-3)


def _small_decoder(seed=9, n_layers=2, max_seq_len=128):
    from videollama2_amd.decoder import HipMixtralDecoder
    cfg = MO.small_mixtral_cfg(n_layers=n_layers)
    sd = MO.seeded_state_dict(cfg, seed=seed, router_scale=4.0)
    return cfg, sd, HipMixtralDecoder(cfg, sd, DEV, max_seq_len=max_seq_len)


def test_decode_step_matches_prefill_and_graph_replays_bitwise():
    from videollama2_amd import ops
    cfg, sd, dec = _small_decoder()
    torch.manual_seed(2)
    S, D = 20, cfg["llm"]["hidden_size"]
    emb = sd["model.embed_tokens.weight"]
    ids = torch.randint(0, cfg["llm"]["vocab_size"], (S + 1,))
    x = emb[ids].to(DEV)
    full = dec.prefill(x, return_all_logits=True).clone()             # logits of positions 0..S
    dec.prefill(x[:S])
    dec.tok.fill_(int(ids[S]))
    step = dec.decode_step().clone()
    assert rel(step, full[S]) < 1e-2
    # graph replay == eager step, bit for bit
    dec.prefill(x[:S])
    eager = []
    for _ in range(3):
        ops.argmax(dec.logits, dec.tok)
        eager.append(dec.decode_step().clone())
    dec.prefill(x[:S])
    g = dec.capture_graph()
    dec.state.copy_(torch.tensor([S - 1, 0], dtype=torch.int32))
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(dec.logits, eager[i]), i
    dec.prefill(x[:S])
    dec.u_buf = torch.rand(cfg["llm"]["vocab_size"], device=DEV)
    dec.capture_graph(sampler=(0.7, 20, 0.9)).replay()
    torch.cuda.synchronize()
    assert torch.isfinite(dec.logits).all()


def test_generate_greedy_equals_oracle_tokens():
    """Greedy tokens (graph-replayed decode) against the fp32 oracle; a differing token is allowed only on a near-tie (tests.util.token_tie_ok)."""
    from tests.util import token_tie_ok
    cfg, sd, dec = _small_decoder(seed=13)
    torch.manual_seed(4)
    x = (0.5 * torch.randn(24, cfg["llm"]["hidden_size"])).bfloat16().float()
    out, mine = dec.generate(x.to(DEV), max_new_tokens=6, use_graph=True, return_logits=True)
    out = out[0].tolist()
    ref, lg, pos = [], [], 24
    logits, caches = MO.mixtral_forward(sd, cfg, x)
    for _ in range(6):
        lg.append(logits[0])
        t = int(logits[0].argmax())
        ref.append(t)
        logits, caches = MO.mixtral_forward(sd, cfg, sd["model.embed_tokens.weight"][t:t + 1], pos, caches)
        pos += 1
    s_div = next((i for i, (a, b) in enumerate(zip(out, ref)) if a != b), len(ref))
    for s in range(min(s_div + 1, len(ref))):
        assert rel(mine[s], lg[s]) < 2e-2, s
    if s_div < len(ref):
        ok, margin, dmax = token_tie_ok(mine[s_div], lg[s_div])
        assert ok, f"step {s_div}: token differs although fp32 top-2 margin {margin:.3e} >= 2 x max|dlogit| {dmax:.3e}"


def test_moe_prefill_captures_into_a_graph():
    cfg, sd, dec = _small_decoder(seed=21)
    torch.manual_seed(5)
    x = torch.randn(40, cfg["llm"]["hidden_size"], device=DEV).bfloat16()
    eager = dec.prefill(x).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.prefill(x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dec.prefill(x)
    dec.logits.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(dec.logits, eager)


def test_moe_decoder_refuses_what_it_does_not_build():
    cfg, sd, dec = _small_decoder(seed=1)
    for fn in (dec.enable_fp8_decode, dec.enable_fp8_prefill, lambda: dec.generate_batch([torch.zeros(4, 256)]),
               lambda: dec.prefill_batch([], [], None)):
        with pytest.raises(NotImplementedError, match="MoE"):
            fn()
    from videollama2_amd.serving import ContinuousBatcher
    with pytest.raises(NotImplementedError, match="MoE"):
        ContinuousBatcher(dec)


def test_model_init_and_mm_infer_give_the_reference_golden_tokens(tmp_path):
    """GPU test 9 of the issue: a local videollama2_mixtral checkpoint written from the fixture's seed, loaded by api.model_init, serves
    frames -> tokens -> text; the greedy tokens are those of the reference's own Videollama2MixtralForCausalLM (tests/golden/
    small_mixtral_T4.pt, scripts/make_golden_mixtral.py; every router decision of the fixture has a margin >= 1e-2)."""
    import os
    from tests.util import ToyTokenizer
    from videollama2_amd import api
    from videollama2_amd.decoder import HipMixtralDecoder
    g = torch.load(os.path.join(os.path.dirname(__file__), "golden", "small_mixtral_T4.pt"), weights_only=False)
    cfg = g["cfg"]
    MO.write_mixtral_checkpoint(tmp_path, g)
    tok = ToyTokenizer(cfg["llm"]["vocab_size"])
    model, processor, _ = api.model_init(str(tmp_path), device=DEV, max_seq_len=192, tokenizer=tok)
    assert isinstance(model.decoder, HipMixtralDecoder)
    frames = processor["video"](g["frames_u8"].numpy())
    assert torch.allclose(frames, g["frames"], atol=1e-6)
    ids = g["input_ids"][None].to(DEV)
    n = len(g["new_tokens"])
    for use_graph in (False, True):
        out = model.generate(ids, attention_mask=torch.ones_like(ids), images=[(g["frames"].to(DEV), "video")], do_sample=False,
                             max_new_tokens=n, use_graph=use_graph)
        assert out[0].tolist() == g["new_tokens"].tolist(), use_graph
    text = api.mm_infer(frames, "what happens in the clip ?", model, tok, modal="video", max_new_tokens=6)
    assert [m["role"] for m in tok.prompts[-1]] == ["system", "user"]                  # videollama2_mixtral takes the system prompt
    prompt = tok.apply_chat_template(tok.prompts[-1])
    pids = api.tokenizer_multimodal_token(prompt, tok, "<video>", return_tensors="pt")[None].to(DEV)
    ref = model.generate(pids, attention_mask=torch.ones_like(pids), images=[(frames.half().to(DEV), "video")], do_sample=False,
                         max_new_tokens=6, eos_token_id=2, use_graph=False)
    assert len(text) > 0 and text == tok.batch_decode(ref)[0].strip()


def test_moe_kernels_on_the_fp16_build():
    """The same MoE block on libvl2hip_f16.so (-DVL2_ELEM_F16): routing tables and the block against the fp32 oracle."""
    from videollama2_amd import _lib, ops
    from videollama2_amd.decoder import HipMixtralDecoder
    _lib.set_elem("fp16")
    try:
        cfg = MO.small_mixtral_cfg(n_layers=1)
        sd = MO.seeded_state_dict(cfg, seed=17, router_scale=4.0)
        dec = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=128)
        torch.manual_seed(6)
        S = 100
        x1 = (0.5 * torch.randn(S, cfg["llm"]["hidden_size"], device=DEV)).half()
        rn = torch.empty((S, 2), dtype=torch.float32, device=DEV)
        out = dec.moe_block(dec.w["layers"][0], x1.clone(), rn)
        torch.cuda.synchronize()
        r = dec.last_route
        counts, offs, gather, inv = _tables(r["ids"], cfg["llm"]["num_local_experts"])
        assert torch.equal(r["gather"].cpu(), gather) and torch.equal(r["inv"].cpu(), inv)
        sdf = {k: v.float().to(DEV) for k, v in sd.items() if k.startswith("model.layers.")}
        ref = x1.float() + MO.moe_block(sdf, cfg, 0, x1.float(), ids=r["ids"], follow_below=1e-3)
        assert rel(out, ref) < TOL_BF16_OUT
        dec.prefill(x1[:20].clone())
        dec.tok.fill_(5)
        assert torch.isfinite(dec.decode_step()).all()
    finally:
        _lib.set_elem("bf16")
