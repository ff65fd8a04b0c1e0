"""Sampled requests in continuous batching, host side only (emulated kernels, no decode step): `ContinuousBatcher.submit(do_sample=True, ...)`
resolves HF's settings and checks and draws the request's uniform numbers at submission exactly as a solo `generate(sampler=...)` of that request
does; `ModelBatcher.submit` resolves against the model's generation_config; admission writes the settings into the slot; the batched draw entry
point is part of the library's export table."""
import types

import pytest
import torch

from oracle import vl2_oracle as O
from tests.emu.backend import emulated_backend


@pytest.fixture(scope="module")
def model(golden_small):
    with emulated_backend():
        from videollama2_amd.model import VideoLLaMA2Hip
        cfg = golden_small["cfg"]
        m = VideoLLaMA2Hip(cfg, O.seeded_state_dict(cfg, golden_small["seed"], round_bf16=True), "cpu", max_seq_len=48)
    return m


def _emb(model, n, seed=0):
    D = model.decoder.D
    return (torch.randn(n, D, generator=torch.Generator().manual_seed(seed)) * 0.5).bfloat16()


def test_submit_accepts_sampling_and_keeps_the_resolved_settings(model):
    from videollama2_amd.serving import ContinuousBatcher
    b = ContinuousBatcher(model.decoder, max_slots=2, use_graph=False)
    g = torch.Generator().manual_seed(3)
    rid = b.submit(_emb(model, 10), max_new_tokens=6, do_sample=True, temperature=0.2, top_p=0.7, generator=g)
    r = b.waiting[-1]
    assert r.rid == rid and r.sampler == (0.2, 50, 0.7)                # HF's default top_k = 50
    assert torch.equal(r.u, torch.rand((6,), generator=torch.Generator().manual_seed(3)))
    b.submit(_emb(model, 10), max_new_tokens=6, do_sample=True)
    assert b.waiting[-1].sampler == (1.0, 50, 1.0)
    b.submit(_emb(model, 10), max_new_tokens=6, do_sample=True, temperature=1.3, top_k=0, top_p=None)
    assert b.waiting[-1].sampler == (1.3, 0, 1.0)
    # greedy requests carry no settings and draw nothing; the sampling keywords are ignored without do_sample, as in HF
    state = torch.get_rng_state()
    b.submit(_emb(model, 10), max_new_tokens=6, temperature=0.5, repetition_penalty=1.2)
    assert b.waiting[-1].sampler is None and b.waiting[-1].u is None and torch.equal(torch.get_rng_state(), state)
    # the row is as long as the decode can run: max_new_tokens capped by the cache
    b.submit(_emb(model, 40), max_new_tokens=100, do_sample=True, generator=torch.Generator().manual_seed(4))
    assert b.waiting[-1].u.shape == (48 - 40 + 1,)


def test_submit_refuses_what_generate_refuses(model):
    from videollama2_amd.serving import ContinuousBatcher
    b = ContinuousBatcher(model.decoder, max_slots=2, use_graph=False)
    x = _emb(model, 8)
    ids = torch.tensor([1, 5, 9, 11], dtype=torch.long)
    cases = [(dict(temperature=0.0), ValueError, "temperature"), (dict(temperature=-1.0), ValueError, "temperature"),
             (dict(top_k=-1), ValueError, "top_k"), (dict(top_p=0.0), ValueError, "top_p"), (dict(top_p=1.5), ValueError, "top_p"),
             (dict(repetition_penalty=1.1), NotImplementedError, "repetition_penalty"), (dict(typical_p=0.5), NotImplementedError, "typical_p")]
    with emulated_backend():
        for kw, err, msg in cases:
            with pytest.raises(err, match=msg) as gen_err:
                model.generate(ids, do_sample=True, max_new_tokens=2, **kw)
            with pytest.raises(err, match=msg) as sub_err:
                b.submit(x, do_sample=True, **kw)
            assert str(sub_err.value) == str(gen_err.value)
    with pytest.raises(TypeError, match="no_such_warper"):
        b.submit(x, do_sample=True, no_such_warper=1)
    assert not b.waiting


def test_uniform_row_equals_the_solo_generate_draw(model):
    """The solo decode draws its numbers into `u_buf` in one torch.rand call at the start; the batcher's row is that call, at submission."""
    from videollama2_amd.serving import ContinuousBatcher
    dec = model.decoder
    x = _emb(model, 12, seed=5)
    with emulated_backend():
        for max_new in (4, 100):
            dec.generate(x, max_new_tokens=max_new, sampler=(0.9, 20, 0.8, torch.Generator().manual_seed(21)))
            n = min(max_new, dec.max_seq_len - 12 + 1)
            solo = dec.u_buf[:n].clone()
            b = ContinuousBatcher(dec, max_slots=2, use_graph=False)
            b.submit(x, max_new_tokens=max_new, do_sample=True, temperature=0.9, top_k=20, top_p=0.8, generator=torch.Generator().manual_seed(21))
            assert torch.equal(b.waiting[-1].u, solo), max_new


def test_model_batcher_resolves_against_the_generation_config(model):
    ids = torch.tensor([1, 5, 9, 11, 4], dtype=torch.long)
    with emulated_backend():
        b = model.batcher(max_slots=2, use_graph=False)
        b.submit(ids, do_sample=True, temperature=0.2, top_p=0.7)
        assert b.inner.waiting[-1].sampler == (0.2, 50, 0.7)
        model.generation_config = types.SimpleNamespace(temperature=0.6, top_k=7, top_p=None, repetition_penalty=1.0)
        try:
            b.submit(ids, do_sample=True)
            assert b.inner.waiting[-1].sampler == (0.6, 7, 1.0)
            b.submit(ids, do_sample=True, top_k=3, top_p=0.9)
            assert b.inner.waiting[-1].sampler == (0.6, 3, 0.9)
            b.submit(ids)
            assert b.inner.waiting[-1].sampler is None
            model.generation_config.repetition_penalty = 1.3
            with pytest.raises(NotImplementedError, match="repetition_penalty"):
                b.submit(ids, do_sample=True)
            b.submit(ids, max_new_tokens=3, do_sample=True, generator=torch.Generator().manual_seed(8), repetition_penalty=1.0)
            assert torch.equal(b.inner.waiting[-1].u, torch.rand((3,), generator=torch.Generator().manual_seed(8)))
        finally:
            del model.generation_config


def test_admission_writes_the_slot_settings(model):
    """Admission prefills the request into its slot and writes its settings, its uniform row and a zero step there; a greedy request
    parks its slot as greedy (temperature 0)."""
    from videollama2_amd.serving import ContinuousBatcher
    dec = model.decoder
    with emulated_backend():
        b = ContinuousBatcher(dec, max_slots=2, use_graph=False)
        bb = b.bb
        bb["samp_T"].fill_(5.0); bb["sstep"].fill_(9)
        b.submit(_emb(model, 9), max_new_tokens=5, do_sample=True, temperature=0.4, top_k=12, top_p=0.6,
                 generator=torch.Generator().manual_seed(2))
        b.submit(_emb(model, 7, seed=1), max_new_tokens=5)
        u = b.waiting[0].u.clone()
        b._admit()
        assert [r.slot for r in b.slots] == [0, 1] and not b.waiting
        assert bb["samp_T"][:2].tolist() == pytest.approx([0.4, 0.0]) and bb["samp_k"][0] == 12 and bb["samp_p"][0].item() == pytest.approx(0.6)
        assert bb["sstep"][:2].tolist() == [0, 0] and torch.equal(bb["u"][0, :5], u)
        assert b.slots[0].u is None and bb["pos"][:2].tolist() == [9, 7]
        b.slots = [None, None]                              # drop the admitted requests without stepping
        b.dec._bb_busy = None


def test_sample_tokens_is_exported_and_bound():
    from videollama2_amd import _lib
    assert "vl2_sample_tokens" in _lib.EXPORTS and "vl2_sample_tokens" not in _lib.SIGNATURES    # the emulator's symbol set is unchanged
    lib = _lib.load()
    assert lib.vl2_sample_tokens.argtypes == _lib.SAMPLE_ROWS_SIGNATURES["vl2_sample_tokens"]
