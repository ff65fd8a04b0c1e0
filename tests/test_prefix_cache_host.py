"""Prefix reuse across chat turns (VideoLLaMA2Hip.generate(..., prefix_cache=True)), host logic only: the model runs with a stub
vision tower / connector (they count their calls) and a stub decoder that records which rows it was asked to prefill and from which
position; embed_rows is a table lookup.  Checks the common-prefix arithmetic in cache rows across the media sentinel, the cases that
must take the full path, and `prefix_cache_stats`."""
import pytest
import torch
import torch.nn as nn

from videollama2_amd import ops
from videollama2_amd.constants import MODAL_INDEX_MAP
from videollama2_amd.dist import FrameSharder
from videollama2_amd.model import VideoLLaMA2Hip

VID = MODAL_INDEX_MAP["<video>"]
D, V, T, NVIS = 16, 64, 4, 6        # hidden, vocab, frames, visual rows per video


class StubTower(nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, frames):                      # [T, 3, H, W] -> [T, 2, D]: a function of the pixels
        self.calls += 1
        return frames.float().mean(dim=(1, 2, 3))[:, None, None].expand(-1, 2, D) + torch.arange(D, dtype=torch.float32)


class StubConnector(nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, feats):                       # [b, t, 2, D] -> [b, NVIS, D]
        self.calls += 1
        b = feats.shape[0]
        return (feats.mean(dim=(1, 2))[:, None, :] + torch.arange(NVIS, dtype=torch.float32)[None, :, None]).bfloat16().expand(b, NVIS, D)


class StubDecoder:
    """The decoder surface the model uses: prefill (via generate) bumps the epoch; generate(start_pos=...) = extend.  Emits `answer`
    and leaves the last token unfed (the eager loop) unless feed_last."""

    def __init__(self, answer, feed_last=False):
        self.D, self.V, self.tp = D, V, 1
        self.w = {"embed": (torch.arange(V * D, dtype=torch.float32).view(V, D) / (V * D)).bfloat16()}
        self.cache_epoch, self.pos = 0, 0
        self.answer, self.feed_last = answer, feed_last
        self.calls = []

    def generate(self, emb, start_pos=None, max_new_tokens=2048, **kw):
        self.cache_epoch += 1
        P = 0 if start_pos is None else start_pos
        assert 0 <= P <= self.pos
        self.calls.append((start_pos, emb.clone()))
        toks = self.answer[:max_new_tokens]
        self.pos = P + emb.shape[0] + len(toks) - (0 if self.feed_last else 1)
        return torch.tensor([toks], dtype=torch.long)


@pytest.fixture
def model(monkeypatch):
    monkeypatch.setattr(ops, "embed_rows", lambda ids, table, out: out.copy_(table[ids.long()]))
    m = VideoLLaMA2Hip.__new__(VideoLLaMA2Hip)
    nn.Module.__init__(m)
    m.cfg = {"num_frames": T}
    m.mm_projector_type = "stc_connector"
    m._dev = torch.device("cpu")
    m.vision_tower, m.mm_projector = StubTower(), StubConnector()
    m.decoder = StubDecoder([7, 8, 9])
    m.sharder = FrameSharder()
    return m


def frames(seed=0):
    return torch.rand((T, 3, 4, 4), generator=torch.Generator().manual_seed(seed))


def full_rows(m, ids, video):
    """The spliced prompt of `ids` as the plain path builds it."""
    feats = m.encode_images_or_videos([(video, "video")])
    _, _, _, emb, _ = m.prepare_inputs_labels_for_multimodal(torch.tensor([ids]), None, None, None, [(video, "video")], mm_features=feats)
    return emb[0]


def run(m, ids, video, modal="video", **kw):
    return m.generate(torch.tensor([ids]), images=[(video, modal)], prefix_cache=True, max_new_tokens=3, **kw)


TURN1 = [1, 2, VID, 3, 4]            # rows: 2 + NVIS + 2 = 10


def test_prefix_stops_inside_the_prompt(model):
    vid = frames()
    run(model, TURN1, vid)
    assert model.prefix_cache_stats == dict(reused_rows=0, prefilled_rows=10, encoder_ran=True)
    assert model.vision_tower.calls == 1 and model.decoder.pos == 10 + 2          # answer 7 8 9: 7 and 8 fed, 9 not
    turn2 = TURN1 + [7, 8, 9, 10, 11]
    out = run(model, turn2, vid)
    assert out.tolist() == [[7, 8, 9]]
    # resident: the prompt's 10 rows + 7, 8 -> the common prefix in rows is 12; 9, 10, 11 are prefilled from row 12
    assert model.prefix_cache_stats == dict(reused_rows=12, prefilled_rows=3, encoder_ran=False)
    assert model.vision_tower.calls == 1 and model.mm_projector.calls == 1
    start, emb = model.decoder.calls[-1]
    assert start == 12 and torch.equal(emb, full_rows(model, turn2, vid)[12:])
    # a prompt that diverges inside the first turn's text: the rows up to the difference
    turn3 = TURN1[:4] + [5, 6]
    run(model, turn3, vid)
    assert model.prefix_cache_stats == dict(reused_rows=2 + NVIS + 1, prefilled_rows=2, encoder_ran=False)
    assert model.decoder.calls[-1][0] == 2 + NVIS + 1


def test_prefix_stops_before_the_sentinel_runs_the_full_path(model):
    vid = frames()
    run(model, TURN1, vid)
    run(model, [1, 5, VID, 3, 4], vid)
    assert model.prefix_cache_stats == dict(reused_rows=0, prefilled_rows=10, encoder_ran=True)
    assert model.vision_tower.calls == 2 and model.decoder.calls[-1][0] is None


def test_changed_frames_run_the_full_path(model):
    vid = frames()
    run(model, TURN1, vid)
    vid2 = vid.clone()
    vid2[1, 2, 3, 0] += 0.5                              # same shape, one pixel differs
    run(model, TURN1 + [7, 8, 5], vid2)
    assert model.prefix_cache_stats == dict(reused_rows=0, prefilled_rows=13, encoder_ran=True)
    assert model.vision_tower.calls == 2
    # ... and the new call was recorded: its own follow-up reuses it
    run(model, TURN1 + [7, 8, 5, 7, 8, 9, 1], vid2)
    assert model.prefix_cache_stats == dict(reused_rows=15, prefilled_rows=2, encoder_ran=False)


def test_changed_modal_runs_the_full_path(model):
    vid = frames()
    run(model, TURN1, vid)
    run(model, TURN1 + [7], vid, modal="image")
    assert model.prefix_cache_stats["encoder_ran"] and model.prefix_cache_stats["reused_rows"] == 0


def test_identical_prompt_backs_off_one_row(model):
    vid = frames()
    run(model, TURN1, vid)
    run(model, TURN1, vid)
    assert model.prefix_cache_stats == dict(reused_rows=9, prefilled_rows=1, encoder_ran=False)
    start, emb = model.decoder.calls[-1]
    assert start == 9 and torch.equal(emb, full_rows(model, TURN1, vid)[9:])
    # a prompt ending in its sentinel: the row backed off to is a visual row, taken from the recorded features
    p = [1, 2, VID]
    run(model, p, vid)
    run(model, p, vid)
    assert model.prefix_cache_stats == dict(reused_rows=1 + NVIS, prefilled_rows=1, encoder_ran=False)
    assert torch.equal(model.decoder.calls[-1][1], full_rows(model, p, vid)[-1:])


def test_intervening_plain_generate_takes_the_full_path(model):
    vid = frames()
    run(model, TURN1, vid)
    model.generate(torch.tensor([TURN1]), images=[(vid, "video")], max_new_tokens=3)      # plain: a prefill, new epoch
    run(model, TURN1 + [7, 8, 9], vid)
    assert model.prefix_cache_stats == dict(reused_rows=0, prefilled_rows=13, encoder_ran=True)
    assert model.decoder.calls[-1][0] is None


def test_graph_mode_resident_rows_follow_the_decoder(model):
    """A graph replay feeds the token it has just picked: the resident rows come from decoder.pos, not from the loop."""
    model.decoder.feed_last = True
    vid = frames()
    run(model, TURN1, vid)
    assert model.decoder.pos == 13
    run(model, TURN1 + [7, 8, 9, 10], vid)
    assert model.prefix_cache_stats == dict(reused_rows=13, prefilled_rows=1, encoder_ran=False)


def test_prefix_cache_refuses_batches(model):
    vid = frames()
    with pytest.raises(NotImplementedError):
        model.generate(torch.tensor([TURN1, TURN1]), images=[(vid, "video"), (vid, "video")], prefix_cache=True)
