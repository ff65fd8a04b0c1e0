"""Prefix reuse across chat turns on the device: the append attention (vl2_attn_append, csrc/k_attn_append.h) against torch fp32 and
vl2_attn_fwd(causal_off = P), `HipMistralDecoder.extend` / `HipMixtralDecoder.extend` against the fp32 oracles, and
`VideoLLaMA2Hip.generate(..., prefix_cache=True)` on the small_T4 fixture (eager, graph-replayed, sampled)."""
import os

import pytest
import torch

from oracle import vl2_oracle as O
from tests import moe_oracle as MO
from tests.util import TOL_BF16_OUT, rel, token_tie_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as ge
    ge.build()


# ------------------------------------------------------------------------------------------------ kernel
def _attn_case(n, P, nh, nkv, smax=4160, seed=0, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed + 131 * n + P + nh)
    q = torch.randn(n, nh * 128, generator=g, device=DEV).to(dtype)
    kc = torch.zeros(nkv, smax, 128, device=DEV, dtype=dtype)
    vc = torch.zeros(nkv, smax, 128, device=DEV, dtype=dtype)
    kc[:, :P + n] = torch.randn(nkv, P + n, 128, generator=g, device=DEV).to(dtype)
    vc[:, :P + n] = torch.randn(nkv, P + n, 128, generator=g, device=DEV).to(dtype)
    kc[:, P + n:] = float("nan")                  # rows past the sequence must not be read
    vc[:, P + n:] = float("nan")
    return q, kc, vc


def _attn_ref(q, kc, vc, P, nh, nkv):
    n, grp = q.shape[0], nh // nkv
    qf = q.float().view(n, nh, 128).transpose(0, 1)                       # [nh, n, 128]
    k = kc[:, :P + n].float().repeat_interleave(grp, 0)                    # [nh, P+n, 128]
    v = vc[:, :P + n].float().repeat_interleave(grp, 0)
    s = qf @ k.transpose(1, 2) * 128 ** -0.5
    mask = torch.arange(P + n, device=q.device)[None, :] > (P + torch.arange(n, device=q.device))[:, None]
    s = s.masked_fill(mask[None], float("-inf"))
    return (s.softmax(-1) @ v).transpose(0, 1).reshape(n, nh * 128)


def _attn_fwd(q, kc, vc, P, nh, nkv):
    from videollama2_amd import ops
    n, smax = q.shape[0], kc.shape[1]
    o = torch.empty_like(q)
    ops.attn_fwd(q, kc, vc, o, (0, 128, nh * 128), (0, smax * 128, 128), (0, smax * 128, 128), (0, 128, nh * 128), 1, nh, n, P + n,
                 nh // nkv, 128 ** -0.5, True, P, 128)
    return o


@pytest.mark.parametrize("nh,nkv", [(32, 8), (28, 4), (32, 32)])
@pytest.mark.parametrize("P", [0, 63, 64, 1650, 4000])
@pytest.mark.parametrize("n", [1, 7, 32, 64])
def test_attn_append_against_fp32_and_attn_fwd(n, P, nh, nkv):
    """Within TOL_BF16_OUT of torch fp32 (the output is rounded to 16 bits once and P rides through the MFMA in 16 bits, as in every
    attention kernel of the library: TOL_F32_OUT = 1e-3 is below that rounding's own floor of 1.1e-3), within twice that of
    vl2_attn_fwd(causal_off = P) (each of the two carries its own 16-bit error), and two runs bit-identical."""
    from videollama2_amd import ops
    q, kc, vc = _attn_case(n, P, nh, nkv)
    o1 = ops.attn_append(q, kc, vc, torch.empty_like(q), P, nh, nkv, 128 ** -0.5)
    o2 = ops.attn_append(q, kc, vc, torch.empty_like(q), P, nh, nkv, 128 ** -0.5)
    ref = _attn_ref(q, kc, vc, P, nh, nkv)
    fwd = _attn_fwd(q, kc, vc, P, nh, nkv)
    torch.cuda.synchronize()
    assert torch.isfinite(o1.float()).all()
    assert torch.equal(o1, o2)
    e_app, e_fwd, d = rel(o1, ref), rel(fwd, ref), rel(o1, fwd)
    print(f"[attn_append] n={n} P={P} nh={nh} nkv={nkv}: vs fp32 {e_app:.2e} (attn_fwd {e_fwd:.2e}), vs attn_fwd {d:.2e}")
    assert e_app < TOL_BF16_OUT
    # two kernels that each round P and the output to 16 bits differ by up to the sum of their errors
    assert d < 2 * TOL_BF16_OUT


def test_attn_append_fp16_build():
    from videollama2_amd import _lib, ops
    P, n, nh, nkv = 1650, 32, 32, 8
    _lib.set_elem("fp16")
    try:
        q, kc, vc = _attn_case(n, P, nh, nkv, dtype=torch.float16)
        o = ops.attn_append(q, kc, vc, torch.empty_like(q), P, nh, nkv, 128 ** -0.5)
        fwd = _attn_fwd(q, kc, vc, P, nh, nkv)
        ref = _attn_ref(q, kc, vc, P, nh, nkv)
        torch.cuda.synchronize()
    finally:
        _lib.set_elem("bf16")
    assert rel(o, ref) < TOL_BF16_OUT and rel(o, fwd) < TOL_BF16_OUT


def test_attn_append_refuses_bad_arguments():
    from videollama2_amd import _lib, ops
    q, kc, vc = _attn_case(8, 100, 32, 8, smax=128)
    with pytest.raises(_lib.Vl2HipError, match="outside the cache"):
        ops.attn_append(q, kc, vc, torch.empty_like(q), 121, 32, 8, 0.1)
    with pytest.raises(_lib.Vl2HipError, match="nkv"):
        ops.attn_append(q, kc, vc, torch.empty_like(q), 100, 32, 5, 0.1)
    with pytest.raises(_lib.Vl2HipError, match="workspace"):
        ops.attn_append(q, kc, vc, torch.empty_like(q), 100, 32, 8, 0.1, ws=torch.empty(16, device=DEV))


# ------------------------------------------------------------------------------------------------ decoder
def test_mistral_extend_7b_width_against_fp32_oracle():
    """Two full-width Mistral-7B layers: prefill(x[:P]) then extend(x[P:]) (n = 32: append attention + skinny-M projections; n = 100: the
    attn_fwd / tiled-GEMM fall-back; n = 7 after n = 32: an extend on top of an extend) -> last-row logits within max(2 x bf16 floor,
    4e-3) of the fp32 oracle's, the floor being the same restatement run in bf16 on the device (tests/test_gpu_parity_full.py)."""
    from videollama2_amd.decoder import HipMistralDecoder
    cfg = O.config_videollama2_7b(16)
    cfg["llm"]["num_hidden_layers"] = 2
    keep = lambda n: n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))
    sd = O.seeded_state_dict(cfg, 31, only=keep)
    P, S = 1650, 1789
    x = (0.5 * torch.randn(S, cfg["llm"]["hidden_size"], generator=torch.Generator().manual_seed(3))).bfloat16().float()
    torch.set_num_threads(min(os.cpu_count() or 8, 16))
    with torch.no_grad():
        truth, _ = O.mistral_forward(sd, cfg, x, last_only=False)
        sd16 = {k: v.to(DEV).bfloat16() for k, v in sd.items()}
        floor_l, _ = O.mistral_forward(sd16, cfg, x.to(DEV).bfloat16(), last_only=False)
        floor_l = floor_l.float().cpu()
        del sd16
    torch.cuda.empty_cache()
    dec = HipMistralDecoder(cfg, sd, DEV, max_seq_len=2048)
    cases = []
    dec.prefill(x[:P].to(DEV))
    cases.append(("n=32", dec.extend(x[P:P + 32].to(DEV)).clone(), P + 31))
    cases.append(("n=7 after n=32", dec.extend(x[P + 32:P + 39].to(DEV)).clone(), P + 38))
    cases.append(("n=100 from P", dec.extend(x[P:P + 100].to(DEV), start_pos=P).clone(), P + 99))
    assert dec.pos == P + 100
    dec.prefill(x[:P + 39].to(DEV))
    cases.append(("n=150", dec.extend(x[P + 39:S].to(DEV)).clone(), S - 1))
    for name, mine, row in cases:
        err, fl = rel(mine, truth[row]), rel(floor_l[row], truth[row])
        print(f"[extend 7B] {name}: rel-L2 {err:.3e}, bf16 floor {fl:.3e}")
        assert err <= max(2.0 * fl, 4e-3), name
    with pytest.raises(ValueError):
        dec.extend(x[:10].to(DEV), start_pos=2040)


def test_extend_epoch_and_refusals():
    from videollama2_amd.decoder import HipMistralDecoder
    g = torch.load(os.path.join(ROOT, "tests", "golden", "small_T4.pt"), weights_only=False)
    cfg = g["cfg"]
    dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, g["seed"]), DEV, max_seq_len=64)
    x = torch.randn(40, cfg["llm"]["hidden_size"], device=DEV).bfloat16()
    e0 = dec.cache_epoch
    dec.prefill(x[:30])
    assert dec.cache_epoch == e0 + 1
    dec.extend(x[30:])
    assert dec.cache_epoch == e0 + 2 and dec.pos == 40
    with pytest.raises(ValueError):
        dec.extend(x[:30])                                 # 40 + 30 > 64
    with pytest.raises(ValueError):
        dec.extend(x[:3], start_pos=41)                    # past the resident rows
    dec.enable_fp8_prefill(True)
    assert dec.cache_epoch == e0 + 3
    with pytest.raises(NotImplementedError):
        dec.extend(x[:3])


def test_mixtral_extend_against_moe_oracle():
    """The small Mixtral fixture's weights (router margins >= 2.98e-2): prefill + extend of its golden inputs_embeds equals the fp32
    oracle's last-row logits to the bound of tests/test_gpu_moe.py's generate check, and the greedy token matches."""
    from videollama2_amd.decoder import HipMixtralDecoder
    g = torch.load(os.path.join(ROOT, "tests", "golden", "small_mixtral_T4.pt"), weights_only=False)
    cfg = g["cfg"]
    sd = MO.fixture_state_dict(g)
    x = g["inputs_embeds"].float()
    dec = HipMixtralDecoder(cfg, sd, DEV, max_seq_len=128)
    for P in (20, 36, 43):
        dec.prefill(x[:P].to(DEV))
        mine = dec.extend(x[P:].to(DEV)).clone()
        ref, _ = MO.mixtral_forward(sd, cfg, x)
        assert rel(mine, ref[0]) < 2e-2, P
        ok = int(mine.argmax()) == int(ref[0].argmax()) or token_tie_ok(mine, ref[0])[0]
        assert ok, P


# ------------------------------------------------------------------------------------------------ model, end to end
@pytest.fixture(scope="module")
def small():
    from videollama2_amd.model import VideoLLaMA2Hip
    g = torch.load(os.path.join(ROOT, "tests", "golden", "small_T4.pt"), weights_only=False)
    cfg = g["cfg"]
    sd = O.seeded_state_dict(cfg, g["seed"], round_bf16=True)
    model = VideoLLaMA2Hip(cfg, sd, DEV, max_seq_len=256)
    return g, cfg, sd, model


def _first_undecidable(a_toks, a_lg, b_toks, b_lg):
    """Tokens must agree up to the first step where they differ, and that step must be a near-tie (token_tie_ok)."""
    for s, (x, y) in enumerate(zip(a_toks, b_toks)):
        if x != y:
            ok, margin, dmax = token_tie_ok(a_lg[s], b_lg[s])
            assert ok, f"step {s}: {x} != {y} with margin {margin:.3e} >= 2 x {dmax:.3e}"
            return s
    return min(len(a_toks), len(b_toks))


@pytest.mark.parametrize("mode", ["eager", "graph", "sampled"])
def test_generate_prefix_cache_turn2(small, mode):
    g, cfg, sd, model = small
    frames = g["frames"].to(DEV)
    images = [(frames, "video")]
    ids1 = g["input_ids"]
    kw = dict(max_new_tokens=6, use_graph=mode == "graph", return_logits=True)
    if mode == "sampled":
        kw.update(do_sample=True, temperature=0.8, top_k=20, top_p=0.95)
    n_vis = model.encode_images_or_videos(images)[0].shape[0]
    S1 = ids1.numel() - 1 + n_vis
    # turn 1: graph mode stops on an EOS (the replay has fed it); eager / sampled on max_new_tokens (the last token is not fed)
    probe = model.generate(ids1[None].to(DEV), images=images, max_new_tokens=6, use_graph=False)[0].tolist()
    eos = probe[3] if mode == "graph" and probe[3] not in probe[:3] else None
    torch.manual_seed(11)
    out1, _ = model.generate(ids1[None].to(DEV), images=images, prefix_cache=True, eos_token_id=eos, **kw)
    out1 = out1[0].tolist()
    assert model.prefix_cache_stats == dict(reused_rows=0, prefilled_rows=S1, encoder_ran=True)
    fed = len(out1) if (mode == "graph" and eos is not None and out1[-1] == eos) else len(out1) - 1
    assert model.decoder.pos == S1 + fed
    new_text = [5, 17, 33]
    ids2 = torch.tensor(ids1.tolist() + out1 + new_text)
    S2 = S1 + len(out1) + len(new_text)
    calls = (model.vision_tower, model.mm_projector)
    n_enc = [0]
    hooks = [m.register_forward_hook(lambda *a: n_enc.__setitem__(0, n_enc[0] + 1)) for m in calls]
    try:
        torch.manual_seed(12)
        out_c, lg_c = model.generate(ids2[None].to(DEV), images=images, prefix_cache=True, **kw)
    finally:
        for h in hooks:
            h.remove()
    assert n_enc[0] == 0
    assert model.prefix_cache_stats == dict(reused_rows=S1 + fed, prefilled_rows=S2 - S1 - fed, encoder_ran=False)
    torch.manual_seed(12)
    out_p, lg_p = model.generate(ids2[None].to(DEV), images=images, **kw)
    out_c, out_p = out_c[0].tolist(), out_p[0].tolist()
    _first_undecidable(out_c, lg_c, out_p, lg_p)
    if mode != "sampled":
        # the fp32 oracle's greedy steps on turn 2 (its own tokens fed: teacher-forced where ours agree)
        sdf = O.seeded_state_dict(cfg, g["seed"], round_bf16=True)
        toks, lg = O.generate(sdf, cfg, ids2, g["frames"], len(out_c))
        _first_undecidable(out_c, lg_c, toks, lg)
