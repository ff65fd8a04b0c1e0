"""Pins the oracle (oracle/vl2_oracle.py): (a) against golden tensors minted from the REAL reference, (b) against the
reference's own encode + greedy tokens on unrounded seeded weights (tests/golden/reference_checks.pt, minted from it)."""
import os

import numpy as np
import pytest
import torch

from oracle import vl2_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_names_cover_golden_config(golden_small):
    names = dict(O.state_dict_names(golden_small["cfg"]))
    assert len(names) == 189


def test_oracle_matches_reference_goldens(golden_small):
    g = golden_small
    cfg = g["cfg"]
    sd = O.seeded_state_dict(cfg, g["seed"], round_bf16=True)
    with torch.no_grad():
        assert torch.allclose(O.normalise_frames_u8(g["frames_u8"].numpy()), g["frames"], atol=1e-6)
        out, hs = O.clip_tower(sd, cfg, g["frames"], return_hidden=True)
        for a, b in zip(hs, g["vit_hidden"]):
            assert torch.allclose(a, b, atol=2e-5, rtol=1e-5)
        assert torch.allclose(out, g["tower_out"], atol=2e-5, rtol=1e-5)
        feats, st = O.stc_connector(sd, out.view(1, *out.shape), return_stages=True)
        assert torch.allclose(st["s1"], g["stc_s1"], atol=2e-5, rtol=1e-5)
        assert torch.allclose(st["sampler"], g["stc_sampler"], atol=2e-5, rtol=1e-5)
        assert torch.allclose(st["s2"], g["stc_s2"], atol=2e-5, rtol=1e-5)
        assert torch.allclose(feats, g["mm_features"], atol=2e-5, rtol=1e-5)
        emb = O.splice_inputs_embeds(sd, g["input_ids"], [feats[0]])
        assert torch.allclose(emb, g["inputs_embeds"], atol=2e-5, rtol=1e-5)
        logits, _ = O.mistral_forward(sd, cfg, emb, last_only=False)
        assert torch.allclose(logits, g["prefill_logits"], atol=1e-4, rtol=1e-4)
        toks, step_logits = O.greedy_generate(sd, cfg, emb, 8)
        assert toks == g["new_tokens"].tolist()
        assert torch.allclose(step_logits, g["step_logits"], atol=1e-4, rtol=1e-4)


def test_token_count_law():
    assert [O.n_visual_tokens(t) for t in (8, 16, 32)] == [845, 1521, 2873]


def test_frame_sample_golden(golden_small):
    for (d, n), ids in golden_small["frame_sample"].items():
        assert np.array_equal(O.frame_sample_uniform(d, n), ids.numpy())


@pytest.fixture(scope="module")
def reference_checks():
    """The reference's own outputs for the two checks below (unrounded seeded weights, seeded frames and ids), minted from the live
    reference by oracle/make_golden.py (mint_reference_checks)."""
    return torch.load(os.path.join(ROOT, "tests", "golden", "reference_checks.pt"), weights_only=False)


def test_oracle_matches_live_reference(reference_checks):
    r = reference_checks["v2"]
    cfg = O.config_small(4)
    sd = O.seeded_state_dict(cfg, r["seed"], round_bf16=False)
    assert set(r["state_dict_keys"]) == set(dict(O.state_dict_names(cfg)))
    rng = np.random.default_rng(r["frames_seed"])
    fr = O.normalise_frames_u8(rng.integers(0, 256, (4, 56, 56, 3), dtype=np.uint8))
    with torch.no_grad():
        b = O.encode_images_or_videos(sd, cfg, [(fr, "video")])
        assert torch.allclose(r["encode"], b, atol=1e-5, rtol=1e-5)
        ids = torch.tensor([1] + list(rng.integers(3, 512, 5)) + [-201] + list(rng.integers(3, 512, 4)))
        toks, _ = O.generate(sd, cfg, ids, fr, 5)
        assert r["tokens"] == toks


# ---------------------------------------------------------------- VideoLLaMA2.1 family

def test_oracle_v21_matches_reference_goldens(golden_small_v21):
    g = golden_small_v21
    cfg = g["cfg"]
    assert O.vision_family(cfg) == "siglip" and O.llm_family(cfg) == "qwen2" and O.conv3d_padding(cfg) == 0
    sd = O.seeded_state_dict(cfg, g["seed"], round_bf16=True)
    with torch.no_grad():
        assert torch.allclose(O.normalise_frames_u8_siglip(g["frames_u8"].numpy()), g["frames"], atol=1e-6)
        out, hs = O.siglip_tower(sd, cfg, g["frames"], return_hidden=True)
        for a, b in zip(hs, g["vit_hidden"]):
            assert torch.allclose(a, b, atol=2e-5, rtol=1e-5)
        assert torch.allclose(out, g["tower_out"], atol=2e-5, rtol=1e-5)
        feats, st = O.stc_connector(sd, out.view(1, *out.shape), return_stages=True, padding=0)
        assert torch.allclose(st["sampler"], g["stc_sampler"], atol=2e-5, rtol=1e-5)
        assert torch.allclose(feats, g["mm_features"], atol=2e-5, rtol=1e-5)
        assert feats.shape[1] == O.n_visual_tokens(4, 4, padding=0) == 8
        emb = O.splice_inputs_embeds(sd, g["input_ids"], [feats[0]])
        assert torch.allclose(emb, g["inputs_embeds"], atol=2e-5, rtol=1e-5)
        logits, _ = O.mistral_forward(sd, cfg, emb, last_only=False)
        assert torch.allclose(logits, g["prefill_logits"], atol=1e-4, rtol=1e-4)
        toks, step_logits = O.greedy_generate(sd, cfg, emb, 8)
        assert toks == g["new_tokens"].tolist()
        assert torch.allclose(step_logits, g["step_logits"], atol=1e-4, rtol=1e-4)
    assert O.n_visual_tokens(16, 27, padding=0) == 1352          # SURVEY 8f row 1 [probe]


def test_oracle_v21_matches_live_reference(reference_checks):
    r = reference_checks["v21"]
    cfg = O.config_small_v21(4)
    sd = O.seeded_state_dict(cfg, r["seed"], round_bf16=False)
    assert set(r["state_dict_keys"]) == set(dict(O.state_dict_names(cfg)))
    rng = np.random.default_rng(r["frames_seed"])
    fr = O.normalise_frames_u8_siglip(rng.integers(0, 256, (4, 56, 56, 3), dtype=np.uint8))
    with torch.no_grad():
        b = O.encode_images_or_videos(sd, cfg, [(fr, "video")])
        assert torch.allclose(r["encode"], b, atol=1e-5, rtol=1e-5)
        ids = torch.tensor([1] + list(rng.integers(3, 512, 5)) + [-201] + list(rng.integers(3, 512, 4)))
        toks, _ = O.generate(sd, cfg, ids, fr, 5)
        assert r["tokens"] == toks
