"""VideoLLaMA2-8x7B (Mixtral sparse MoE) on the host side: checkpoint config -> cfg, weight packing of both key layouts, and the fp32
MoE oracle against the live HF Mixtral modules.  No GPU needed."""
import json

import pytest
import torch

from tests import moe_oracle as MO
from videollama2_amd import api
from videollama2_amd.config import check_supported, videollama2_8x7b


def _config_8x7b(**over):
    """config.json of VideoLLaMA2-8x7B as `save_pretrained` writes it (Videollama2MixtralConfig = MixtralConfig + the multimodal keys)."""
    c = dict(model_type="videollama2_mixtral", architectures=["Videollama2MixtralForCausalLM"], hidden_size=4096, intermediate_size=14336,
             num_hidden_layers=32, num_attention_heads=32, num_key_value_heads=8, head_dim=128, vocab_size=32000, rms_norm_eps=1e-5,
             rope_theta=1e6, sliding_window=None, max_position_embeddings=32768, num_local_experts=8, num_experts_per_tok=2,
             router_aux_loss_coef=0.02, mm_projector_type="stc_connector", mm_vision_tower="openai/clip-vit-large-patch14-336",
             mm_vision_select_layer=-2, num_frames=8)
    c.update(over)
    return c


def test_8x7b_checkpoint_config_maps_to_the_builtin_config(tmp_path):
    json.dump(_config_8x7b(), open(tmp_path / "config.json", "w"))
    cfg, _ = api.config_from_checkpoint(str(tmp_path))
    want = videollama2_8x7b(8)
    assert cfg["llm"] == want["llm"] and cfg["vision"] == want["vision"] and cfg["projector"] == "stc_connector" and cfg["num_frames"] == 8
    check_supported(cfg)
    keyless = {k: v for k, v in _config_8x7b().items() if k not in ("num_local_experts", "num_experts_per_tok")}
    json.dump(keyless, open(tmp_path / "config.json", "w"))
    with pytest.raises(ValueError, match="not built"):
        api.config_from_checkpoint(str(tmp_path))


def test_moe_limits_and_sliding_window_refused():
    for E, k in ((65, 2), (8, 5), (2, 3), (8, 0)):
        cfg = videollama2_8x7b(8)
        cfg["llm"].update(num_local_experts=E, num_experts_per_tok=k)
        with pytest.raises(ValueError, match="MoE"):
            check_supported(cfg)
    cfg = videollama2_8x7b(8)
    cfg["llm"].update(sliding_window=4096, max_position_embeddings=32768)
    with pytest.raises(ValueError, match="sliding_window"):
        check_supported(cfg)


def test_both_key_layouts_pack_to_identical_tensors():
    from videollama2_amd.weights import pack_decoder, state_dict_names
    cfg = MO.small_mixtral_cfg()
    sd5 = MO.seeded_state_dict(cfg, seed=7)
    assert {n for n, _ in state_dict_names(cfg)} <= set(sd5)                      # every weight the packer names is in the oracle's set
    assert {n for n in sd5 if n.startswith("model.layers.")} <= {n for n, _ in state_dict_names(cfg)}
    sd4 = MO.to_v4_keys(sd5, cfg)
    assert not any(k.startswith("model.layers.") and ".mlp." in k for k in sd4)
    p5, p4 = pack_decoder(sd5, cfg, "cpu"), pack_decoder(sd4, cfg, "cpu")
    l = cfg["llm"]
    E, D, I = l["num_local_experts"], l["hidden_size"], l["intermediate_size"]
    for a, b in zip(p5["layers"], p4["layers"]):
        assert set(a) == set(b) and "wgu" in a and "wr" in a
        assert a["wgu"].shape == (E, 2 * I, D) and a["wd"].shape == (E, D, I) and a["wr"].shape == (E, D)
        for key in a:
            if a[key] is not None:
                assert torch.equal(a[key], b[key]), key
    # expert e's gate/up = the dense packing of (gate_e, up_e) with the post-attention norm folded in
    from videollama2_amd.weights import fold_norm, pack_gate_up
    gu = sd5["model.layers.1.mlp.experts.gate_up_proj"]
    ref = fold_norm(pack_gate_up(gu[3, :I], gu[3, I:]), sd5["model.layers.1.post_attention_layernorm.weight"])[0]
    assert torch.equal(p5["layers"][1]["wgu"][3], ref)


def _hf_mixtral(cfg, sd):
    from transformers import MixtralConfig, MixtralForCausalLM
    l = cfg["llm"]
    hc = MixtralConfig(hidden_size=l["hidden_size"], intermediate_size=l["intermediate_size"], num_hidden_layers=l["num_hidden_layers"],
                       num_attention_heads=l["num_attention_heads"], num_key_value_heads=l["num_key_value_heads"], head_dim=l["head_dim"],
                       vocab_size=l["vocab_size"], rms_norm_eps=l["rms_norm_eps"], rope_theta=l["rope_theta"], sliding_window=None,
                       num_local_experts=l["num_local_experts"], num_experts_per_tok=l["num_experts_per_tok"], tie_word_embeddings=False)
    hc._attn_implementation = "eager"
    m = MixtralForCausalLM(hc).float().eval()
    llm = {k: v for k, v in sd.items() if k.startswith(("model.layers.", "model.embed_tokens", "model.norm", "lm_head"))}
    missing, unexpected = m.load_state_dict(llm, strict=False)
    assert not unexpected and not [k for k in missing if "rotary" not in k], (missing, unexpected)
    return m


def test_moe_oracle_equals_hf_mixtral_fp32():
    torch.manual_seed(0)
    cfg = MO.small_mixtral_cfg(n_layers=2)
    sd = MO.seeded_state_dict(cfg, seed=11)
    m = _hf_mixtral(cfg, sd)
    S, D = 13, cfg["llm"]["hidden_size"]
    x = torch.randn(S, D)
    with torch.no_grad():
        blk = m.model.layers[1].mlp                                      # MixtralSparseMoeBlock on the normalised rows
        h = m.model.layers[1].post_attention_layernorm(x[None])
        ref = blk(h)[0]
        ours = MO.moe_block(sd, cfg, 1, x)
        assert ((ours - ref).norm() / ref.norm()).item() <= 1e-6
        ref_logits = m(inputs_embeds=x[None]).logits[0]
        ours_logits, _ = MO.mixtral_forward(sd, cfg, x, last_only=False)
        assert ((ours_logits - ref_logits).norm() / ref_logits.norm()).item() <= 1e-6


def _golden():
    import os
    return torch.load(os.path.join(os.path.dirname(__file__), "golden", "small_mixtral_T4.pt"), weights_only=False)


def test_moe_oracle_reproduces_the_reference_golden():
    """The fixture minted from the reference's own Videollama2MixtralForCausalLM (scripts/make_golden_mixtral.py): the oracle's encode +
    splice gives the reference's inputs_embeds, and its greedy decode gives the reference's tokens and step logits.  The weights the
    fixture names are the oracle's (same keys), and every router decision of the fixture is decidable (margin >= 1e-2)."""
    from oracle import vl2_oracle as O
    g = _golden()
    cfg = g["cfg"]
    assert g["min_router_margin"] >= 1e-2
    sd = MO.fixture_state_dict(g)
    assert set(g["state_dict_keys"]) <= set(sd)
    assert any(".mlp.experts.gate_up_proj" in k for k in g["state_dict_keys"])          # the reference's layout under transformers 5
    with torch.no_grad():
        feats = O.encode_images_or_videos(sd, cfg, [(g["frames"], "video")])
        emb = O.splice_inputs_embeds(sd, g["input_ids"], [feats[0]])
        assert ((emb - g["inputs_embeds"]).norm() / g["inputs_embeds"].norm()).item() <= 1e-5
        logits, caches = MO.mixtral_forward(sd, cfg, emb)
        pos, toks = emb.shape[0], []
        for s in range(len(g["new_tokens"])):
            ref = g["step_logits"][s]
            assert ((logits[0] - ref).norm() / ref.norm()).item() <= 1e-5, s
            t = int(logits[0].argmax())
            toks.append(t)
            logits, caches = MO.mixtral_forward(sd, cfg, sd["model.embed_tokens.weight"][t:t + 1], pos, caches)
            pos += 1
    assert toks == g["new_tokens"].tolist()


def test_moe_oracle_equals_live_reference_mixtral():
    """Where the reference tree is importable: its Videollama2MixtralForCausalLM forward on the fixture's embeddings == the oracle's
    (fp32, 1e-6), and its encode / splice of the fixture's request == the oracle's.  Skipped without the tree, as test_oracle_pin does."""
    from oracle import ref_harness as RH
    if not RH.reference_available():
        pytest.skip("reference tree not present")
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_golden_mixtral", os.path.join(os.path.dirname(os.path.dirname(__file__)), "scripts",
                                                                                      "make_golden_mixtral.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    g = _golden()
    cfg = g["cfg"]
    sd = MO.fixture_state_dict(g)
    model = mk.build_reference_mixtral(cfg, sd)
    with torch.no_grad():
        ids = g["input_ids"]
        _, _, _, emb, _ = model.prepare_inputs_labels_for_multimodal(ids[None], torch.ones_like(ids)[None], None, None, [(g["frames"], "video")])
        assert ((emb[0] - g["inputs_embeds"]).norm() / g["inputs_embeds"].norm()).item() <= 1e-6
        ref = model(inputs_embeds=emb).logits[0]
        ours, _ = MO.mixtral_forward(sd, cfg, emb[0], last_only=False)
        assert ((ours - ref).norm() / ref.norm()).item() <= 1e-6


def test_moe_abi_rejects_short_row_strides():
    """Argument checks of the MoE entry points run before any launch (no GPU needed): a row stride below the row width is refused."""
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    rc = lib.vl2_moe_route(p, 64, p, 4, 128, 8, 2, 1e-5, p, p, p, None, p, p, p, p, 1024, None, None, None)
    assert rc == -2 and b"ldx>=D" in lib.vl2_last_error_string()
    rc = lib.vl2_moe_combine(p, 128, p, 64, p, p, 4, 2, 128, 1e-5, p, 128, None, None)
    assert rc == -2 and b">= D" in lib.vl2_last_error_string()
    rc = lib.vl2_moe_route(p, 128, p, 4, 128, 65, 2, 1e-5, p, p, p, None, p, p, p, p, 1024 * 16, None, None, None)
    assert rc == -3
