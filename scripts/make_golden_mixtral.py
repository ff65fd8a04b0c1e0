"""TEST INFRASTRUCTURE ONLY.  Mints tests/golden/small_mixtral_T4.pt by running the REAL reference's Videollama2MixtralForCausalLM
(videollama2/model/videollama2_mixtral.py, imported in place through oracle.ref_harness) on a tiny VideoLLaMA2-8x7B-shaped config:
CLIP-small + stc_connector + a 2-layer Mixtral with 8 experts, top 2.  Run where the reference tree is present:

    python scripts/make_golden_mixtral.py

Weights are not stored: they are tests.moe_oracle.seeded_state_dict(cfg, seed, router_scale, structured=True) (name-keyed generators,
rounded once to bf16; the router built so that its top-k calls can be decidable),
so the GPU tests rebuild them.  The seed is the first one from SEED0 whose every router decision -- prefill and each greedy step, every
layer -- has a top-k / top-(k+1) probability margin >= MIN_MARGIN, so the fixture's routing is decidable in bf16; the margin is recorded."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as RH  # noqa: E402
from tests import moe_oracle as MO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "small_mixtral_T4.pt")
SEED0, ROUTER_SCALE, MIN_MARGIN, N_NEW = 1234, 40.0, 1e-2, 8


def build_reference_mixtral(cfg, sd):
    """Videollama2MixtralForCausalLM(config) with a CLIP tower and stc_connector, fp32, eval, the given weights (strict load)."""
    RH.import_reference()
    from videollama2.model.videollama2_mixtral import Videollama2MixtralConfig, Videollama2MixtralForCausalLM
    l = cfg["llm"]
    hf_cfg = Videollama2MixtralConfig(
        hidden_size=l["hidden_size"], intermediate_size=l["intermediate_size"], num_hidden_layers=l["num_hidden_layers"],
        num_attention_heads=l["num_attention_heads"], num_key_value_heads=l["num_key_value_heads"], head_dim=l["head_dim"],
        vocab_size=l["vocab_size"], rms_norm_eps=l["rms_norm_eps"], rope_theta=l["rope_theta"], max_position_embeddings=32768,
        sliding_window=None, num_local_experts=l["num_local_experts"], num_experts_per_tok=l["num_experts_per_tok"],
        tie_word_embeddings=False, attn_implementation="eager", mm_vision_tower=RH.write_clip_dir(cfg), mm_projector_type="stc_connector",
        mm_hidden_size=cfg["vision"]["hidden_size"], mm_vision_select_layer=cfg["vision"]["select_layer"], mm_vision_select_feature="patch",
        num_frames=cfg["num_frames"], bos_token_id=1, eos_token_id=2, pad_token_id=0)
    model = Videollama2MixtralForCausalLM(hf_cfg).float().eval()
    want = {k for k, v in model.state_dict().items() if torch.is_floating_point(v)}
    missing = want - set(sd)
    assert not missing, sorted(missing)[:8]
    model.load_state_dict({k: sd[k] for k in want}, strict=False)
    return model


def run(cfg, seed):
    """The reference's generate on the seeded request -> (fixture dict, smallest router margin seen)."""
    sd = MO.seeded_state_dict(cfg, seed, router_scale=ROUTER_SCALE, structured=True)
    model = build_reference_mixtral(cfg, sd)
    k = cfg["llm"]["num_experts_per_tok"]
    margins = []

    def hook(mod, inp, out):                      # MixtralTopKRouter.forward -> (router_logits, scores, indices)
        margins.append(MO.margins(torch.softmax(out[0].float(), -1), k).min().item())

    hooks = [layer.mlp.gate.register_forward_hook(hook) for layer in model.model.layers]
    from videollama2.mm_utils import process_video
    proc = model.get_vision_tower().image_processor
    T, S, V = cfg["num_frames"], cfg["vision"]["image_size"], cfg["llm"]["vocab_size"]
    rng = np.random.default_rng(seed)
    frames_u8 = rng.integers(0, 256, (T, S, S, 3), dtype=np.uint8)
    frames = process_video(frames_u8, proc, aspect_ratio=None, num_frames=T)
    ids = torch.tensor([1] + list(rng.integers(3, V, 7)) + [-201] + list(rng.integers(3, V, 9)))
    with torch.no_grad():
        _, mask, _, emb, _ = model.prepare_inputs_labels_for_multimodal(ids[None], torch.ones_like(ids)[None], None, None, [(frames, "video")])
        out = model.generate(ids[None], attention_mask=torch.ones_like(ids)[None], images=[(frames, "video")], do_sample=False,
                             max_new_tokens=N_NEW, use_cache=True, pad_token_id=0, eos_token_id=None, output_scores=True,
                             return_dict_in_generate=True)
    for h in hooks:
        h.remove()
    g = dict(cfg=cfg, seed=seed, router_scale=ROUTER_SCALE, structured_router=True, frames_u8=torch.from_numpy(frames_u8), frames=frames, input_ids=ids,
             inputs_embeds=emb[0], new_tokens=out.sequences[0], step_logits=torch.stack([s[0] for s in out.scores]),
             state_dict_keys=sorted(k_ for k_, v in model.state_dict().items() if torch.is_floating_point(v)))
    return g, min(margins)


def main():
    cfg = MO.small_mixtral_cfg(num_frames=4, n_layers=2, E=8, k=2)
    for seed in range(SEED0, SEED0 + 200):
        g, m = run(cfg, seed)
        print(f"seed {seed}: smallest router margin {m:.3e}")
        if m >= MIN_MARGIN:
            g["min_router_margin"] = m
            torch.save(g, OUT)
            print("wrote", OUT, "tokens", g["new_tokens"].tolist())
            return
    raise SystemExit(f"no seed in [{SEED0}, {SEED0 + 200}) with every router margin >= {MIN_MARGIN}")


if __name__ == "__main__":
    main()
