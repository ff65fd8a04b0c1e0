"""The fp8 KV cache of the decode step on MI355X (include/vl2hip.h vl2_kv_quant / vl2_attn_decode_kv8 / vl2_attn_decode_kv8_batched,
csrc/k_kv8.h; definition: tests/fp8kv_oracle.py).  Kernels at nkv = 2, smax = 256: the row quantiser is the oracle's byte for byte; the
attention on the fp8 cache is bit for bit vl2_attn_decode on the dequantised cache (bf16 build) and appends the oracle's quantisation of the
row that call appends; both builds meet the fp32 definition; a batched row is the single-sequence call and a replayed graph the eager call.
Decoder and serving on the small golden config (head_dim 128): unchanged prefill, solo / batched / continuous decoding on every decode
weight format, toggling, slot memory, and the measured accuracy against the definition's own error."""
import json
import os

import pytest
import torch

from oracle import vl2_oracle as O
from tests import fp8kv_oracle as KV
from tests.util import TOL_BF16_OUT, rel, token_tie_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"
NKV, SMAX, HD = 2, 256, 128
SCALE = HD ** -0.5
POSITIONS = (0, 15, 16, 62, 63, 64, 65, 128, 255)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib, ops as o
    _lib.load()
    return o


def _tables():
    inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2, dtype=torch.int64).float() / HD))
    fr = torch.arange(SMAX, dtype=torch.float32)[:, None] * inv[None, :]
    return fr.cos().contiguous().to(DEV), fr.sin().contiguous().to(DEV)


def _random_cache(seed, elem):
    """[NKV, SMAX, 128] with row magnitudes spread over 2^-8 .. 2^8, so that the rows' scales differ."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(NKV, SMAX, HD, generator=g) * torch.exp2(torch.randint(-8, 9, (NKV, SMAX, 1), generator=g).float())
    return x.to(elem)


class Ref:
    """Computed once per element type and left unchanged: a random cache pair, its quantisation by the oracle and the dequantised copy."""

    def __init__(self, elem):
        self.elem = elem
        self.k16, self.v16 = _random_cache(1, elem), _random_cache(2, elem)
        (self.k8, self.ks), (self.v8, self.vs) = KV.quant_cache_rows(self.k16), KV.quant_cache_rows(self.v16)
        self.kd, self.vd = KV.dequant_cache(self.k8, self.ks), KV.dequant_cache(self.v8, self.vs)
        self.cos, self.sin = _tables()

    def kv8(self, roll=0):
        """A fresh device copy of the fp8 cache (rolled along the positions: another sequence's rows)."""
        return tuple(t.roll(roll, 1).contiguous().to(DEV) for t in (self.k8, self.v8, self.ks, self.vs))

    def kv16(self, roll=0):
        return tuple(t.roll(roll, 1).to(self.elem).contiguous().to(DEV) for t in (self.kd, self.vd))


@pytest.fixture(scope="module")
def ref(ops):
    r = Ref(torch.bfloat16)
    assert torch.equal(r.kd.bfloat16().float(), r.kd) and torch.equal(r.vd.bfloat16().float(), r.vd)       # code * 2^e is exact in bf16
    return r


def _qkv(nh, seed, elem=torch.bfloat16, rows=None):
    g = torch.Generator().manual_seed(seed)
    shape = ((nh + 2 * NKV) * HD,) if rows is None else (rows, (nh + 2 * NKV) * HD)
    return (torch.randn(shape, generator=g) * 1.5).to(elem).to(DEV)


def _partial(nh, B=1):
    return torch.empty((B * nh * ((SMAX + 63) // 64) * 130,), dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. the quantiser
@pytest.mark.parametrize("p0,p1", [(0, 1), (0, 64), (63, 66), (200, 256)])
def test_kv_quant_is_the_oracle_byte_for_byte(ops, ref, p0, p1):
    k16, v16 = ref.k16.clone(), ref.v16.clone()
    for c, base in ((k16, 0), (v16, 1)):                     # planted rows inside every range: all-zero, amax = 448 * 2^e exactly, 1e-30
        for p in sorted({p0, (p0 + p1) // 2, p1 - 1}):
            kind = (p + base) % 3
            if kind == 0:
                c[0, p] = 0
            elif kind == 1:
                c[0, p] = c[0, p].float().clamp(-1, 1).to(c.dtype)
                c[0, p, 77] = -448.0 * 2.0 ** -3
            else:
                c[0, p] = 1e-30
            c[1, p] = 0 if kind == 2 else c[1, p]
    (qk, sk), (qv, sv) = KV.quant_cache_rows(k16), KV.quant_cache_rows(v16)
    assert sk[0, p0].item() in (1.0, 2.0 ** -3, 2.0 ** -100)
    k8 = torch.full((NKV, SMAX, HD), 0xAB, dtype=torch.uint8, device=DEV)
    v8 = torch.full((NKV, SMAX, HD), 0xCD, dtype=torch.uint8, device=DEV)
    ks = torch.full((NKV, SMAX), -7.0, dtype=torch.float32, device=DEV)
    vs = torch.full((NKV, SMAX), -9.0, dtype=torch.float32, device=DEV)
    ops.kv_quant(k16.to(DEV), v16.to(DEV), (k8, v8, ks, vs), p0, p1)
    torch.cuda.synchronize()
    k8, v8, ks, vs = k8.cpu(), v8.cpu(), ks.cpu(), vs.cpu()
    assert torch.equal(k8[:, p0:p1], qk[:, p0:p1]) and torch.equal(v8[:, p0:p1], qv[:, p0:p1])
    assert torch.equal(ks[:, p0:p1], sk[:, p0:p1]) and torch.equal(vs[:, p0:p1], sv[:, p0:p1])
    out = torch.ones(SMAX, dtype=torch.bool)
    out[p0:p1] = False
    assert bool((k8[:, out] == 0xAB).all()) and bool((v8[:, out] == 0xCD).all())
    assert bool((ks[:, out] == -7.0).all()) and bool((vs[:, out] == -9.0).all())


# ---------------------------------------------------------------------------------------------------------------- 2. the bits contract
def _check_appended_row(kv8_after, kv8_before, k16_after, v16_after, pos):
    """Row `pos` of the fp8 cache = the oracle's quantisation of the row the 16-bit call appended; no other row changed."""
    k8, v8, ks, vs = (t.cpu() for t in kv8_after)
    (qk, sk), (qv, sv) = KV.quant_cache_rows(k16_after.cpu()[:, pos:pos + 1]), KV.quant_cache_rows(v16_after.cpu()[:, pos:pos + 1])
    assert torch.equal(k8[:, pos:pos + 1], qk) and torch.equal(ks[:, pos:pos + 1], sk), pos
    assert torch.equal(v8[:, pos:pos + 1], qv) and torch.equal(vs[:, pos:pos + 1], sv), pos
    keep = torch.ones(SMAX, dtype=torch.bool)
    keep[pos] = False
    for a, b in zip((k8, v8, ks, vs), kv8_before):
        assert torch.equal(a[:, keep], b.cpu()[:, keep]), pos


@pytest.mark.parametrize("group", [4, 7], ids=["group4_mistral", "group7_qwen2"])
def test_attention_on_the_fp8_cache_equals_the_16bit_kernel_on_the_dequantised_cache(ops, ref, group):
    """Both kernels append the new token's row before they attend, and the 16-bit kernel appends it UNQUANTISED: on a general qkv row the two
    outputs differ by exactly that row's quantisation (seen: every position below 63, where the new row carries weight).  So per position:
    (a) a general random qkv row: the row the fp8 kernel appends is, byte for byte, the oracle's quantisation of the row vl2_attn_decode
        appends (rope, round, then quantise), and no other row changes;
    (b) the same random q with a new row that is on the fp8 grid already (V: a dequantised row; K: a dequantised row at pos 0, where RoPE is
        the identity, the zero row elsewhere): quantising it is exact, and then the outputs are torch.equal and the two caches hold the same
        values in every row -- on any resident cache and any q, which is what the shared attn_slice_compute guarantees;
    (c) the step after (a), at pos + 1, with an on-grid new row: the general row (a) appended is now a resident row with a non-trivial K, and
        the output equals the 16-bit kernel's on the dequantised post-append cache."""
    nh = NKV * group
    partial = _partial(nh)
    before = (ref.k8, ref.v8, ref.ks, ref.vs)
    for pos in POSITIONS:
        qkv = _qkv(nh, seed=100 * group + pos)
        kv8, (kd, vd) = ref.kv8(), ref.kv16()
        out8 = torch.zeros(nh * HD, dtype=torch.bfloat16, device=DEV)
        out16 = torch.ones(nh * HD, dtype=torch.bfloat16, device=DEV)
        ops.attn_decode_kv8(qkv, kv8, ref.cos, ref.sin, partial, out8, nh, NKV, pos, SCALE)
        ops.attn_decode(qkv, kd, vd, ref.cos, ref.sin, partial, out16, nh, NKV, pos, SCALE)
        torch.cuda.synchronize()
        _check_appended_row(kv8, before, kd, vd, pos)
        vgrid = ref.vd[:, (pos + 7) % SMAX].reshape(-1).bfloat16().to(DEV)
        if pos + 1 < SMAX:
            # (c) the next step on the cache (a) left: row pos is now a GENERAL roped, rounded, quantised row; the 16-bit kernel reads its
            # dequantised copy.  The step's own new row is on the grid (K zero, V a dequantised row), so the outputs must be equal.
            kd2 = KV.dequant_cache(kv8[0], kv8[2]).bfloat16().to(DEV)
            vd2 = KV.dequant_cache(kv8[1], kv8[3]).bfloat16().to(DEV)
            q2 = _qkv(nh, seed=100 * group + pos + 5000)
            q2[nh * HD:(nh + NKV) * HD] = 0
            q2[(nh + NKV) * HD:] = vgrid
            ops.attn_decode_kv8(q2, kv8, ref.cos, ref.sin, partial, out8, nh, NKV, pos + 1, SCALE)
            ops.attn_decode(q2, kd2, vd2, ref.cos, ref.sin, partial, out16, nh, NKV, pos + 1, SCALE)
            torch.cuda.synchronize()
            assert torch.equal(out8, out16), ("after a general row", group, pos, int((out8 != out16).sum()))
        # (b) the new row on the grid
        qkv[nh * HD:(nh + NKV) * HD] = ref.kd[:, (pos + 3) % SMAX].reshape(-1).bfloat16().to(DEV) if pos == 0 else 0
        qkv[(nh + NKV) * HD:] = vgrid
        kv8, (kd, vd) = ref.kv8(), ref.kv16()
        ops.attn_decode_kv8(qkv, kv8, ref.cos, ref.sin, partial, out8, nh, NKV, pos, SCALE)
        ops.attn_decode(qkv, kd, vd, ref.cos, ref.sin, partial, out16, nh, NKV, pos, SCALE)
        torch.cuda.synchronize()
        assert torch.equal(out8, out16), (group, pos, int((out8 != out16).sum()))
        _check_appended_row(kv8, before, kd, vd, pos)
        assert torch.equal(KV.dequant_cache(kv8[0], kv8[2]), kd.float().cpu()) and torch.equal(KV.dequant_cache(kv8[1], kv8[3]), vd.float().cpu()), pos


# ---------------------------------------------------------------------------------------------------------------- 3. the definition
def _against_definition(ops, r, nh, pos):
    qkv = _qkv(nh, seed=7 + pos, elem=r.elem)
    kv8 = r.kv8()
    out = torch.zeros(nh * HD, dtype=r.elem, device=DEV)
    ops.attn_decode_kv8(qkv, kv8, r.cos, r.sin, _partial(nh), out, nh, NKV, pos, SCALE)
    torch.cuda.synchronize()
    q = KV.rope_row(qkv[:nh * HD].float().cpu().view(nh, HD), r.cos[pos].cpu(), r.sin[pos].cpu()).to(r.elem).float()    # roped q is a 16-bit tensor
    kd, vd = KV.dequant_cache(kv8[0], kv8[2]), KV.dequant_cache(kv8[1], kv8[3])                 # the cache WITH the appended row
    return rel(out, KV.attn_decode_ref(q, kd[:, :pos + 1], vd[:, :pos + 1], SCALE))


@pytest.mark.parametrize("pos", [0, 64, 255])
def test_attention_meets_the_definition_bf16(ops, ref, pos):
    for group in (4, 7):
        e = _against_definition(ops, ref, NKV * group, pos)
        assert e < TOL_BF16_OUT, (group, pos, e)


def test_attention_meets_the_definition_fp16_build(ops):
    from videollama2_amd import _lib
    _lib.set_elem("fp16")
    try:
        r = Ref(torch.float16)
        # the quantiser in this build: the oracle's bytes as well
        kv8 = tuple(torch.zeros_like(t) for t in r.kv8())
        ops.kv_quant(r.k16.to(DEV), r.v16.to(DEV), kv8, 0, SMAX)
        for a, b in zip(kv8, (r.k8, r.v8, r.ks, r.vs)):
            assert torch.equal(a.cpu(), b)
        for pos in (0, 64, 255):
            for group in (4, 7):
                e = _against_definition(ops, r, NKV * group, pos)
                assert e < TOL_BF16_OUT, (group, pos, e)
    finally:
        _lib.set_elem("bf16")


# ---------------------------------------------------------------------------------------------------------------- 4. batched, graph
def _stack(ref, rolls):
    per = [ref.kv8(r) for r in rolls]
    return tuple(torch.stack([p[i] for p in per]).contiguous() for i in range(4))


def test_batched_rows_equal_the_single_sequence_call_and_the_graph_the_eager_calls(ops, ref):
    nh, B = NKV * 4, 3
    pos0 = (0, 65, 200)
    rolls = (0, 5, 11)
    cos, sin = ref.cos, ref.sin
    qkvs = [_qkv(nh, seed=40 + s, rows=B) for s in range(3)]
    # eager single-sequence calls: three steps per slot, positions advancing
    singles, outs = [ref.kv8(r) for r in rolls], torch.zeros(3, B, nh * HD, dtype=torch.bfloat16, device=DEV)
    p1 = _partial(nh)
    for s in range(3):
        for b in range(B):
            ops.attn_decode_kv8(qkvs[s][b], singles[b], cos, sin, p1, outs[s, b], nh, NKV, pos0[b] + s, SCALE)
    single_caches = tuple(torch.stack([sg[i] for sg in singles]) for i in range(4))
    # batched, eager: the same three steps
    pB = _partial(nh, B)
    kvb = _stack(ref, rolls)
    pos = torch.tensor(pos0, dtype=torch.int32, device=DEV)
    out_b = torch.zeros(3, B, nh * HD, dtype=torch.bfloat16, device=DEV)
    for s in range(3):
        ops.attn_decode_kv8_batched(qkvs[s], kvb, cos, sin, pB, out_b[s], nh, NKV, pos, SMAX, SCALE)
        pos += 1
    torch.cuda.synchronize()
    assert torch.equal(out_b, outs)
    for a, b in zip(kvb, single_caches):
        assert torch.equal(a, b)
    # step 0 eager, then steps 1 and 2 as two replays of ONE captured graph whose position advances on the device
    kvg = _stack(ref, rolls)
    fresh = tuple(t.clone() for t in kvg)
    pos = torch.tensor(pos0, dtype=torch.int32, device=DEV)
    qbuf, obuf = qkvs[0].clone(), torch.zeros(B, nh * HD, dtype=torch.bfloat16, device=DEV)

    def step():
        ops.attn_decode_kv8_batched(qbuf, kvg, cos, sin, pB, obuf, nh, NKV, pos, SMAX, SCALE)
        pos.add_(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                 # warm-up = step 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(obuf, outs[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for s in (1, 2):
        qbuf.copy_(qkvs[s])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(obuf, outs[s]), s
    assert pos.tolist() == [p + 3 for p in pos0]
    for a, b in zip(kvg, single_caches):
        assert torch.equal(a, b)
    # a position at or past the cache end writes nothing to its sequence's cache
    kvx = tuple(t.clone() for t in fresh)
    pos = torch.tensor([SMAX, 65, SMAX + 3], dtype=torch.int32, device=DEV)
    ox = torch.zeros(B, nh * HD, dtype=torch.bfloat16, device=DEV)
    ops.attn_decode_kv8_batched(qkvs[0], kvx, cos, sin, pB, ox, nh, NKV, pos, SMAX, SCALE)
    torch.cuda.synchronize()
    for a, b in zip(kvx, fresh):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    one = ref.kv8(rolls[1])
    o1 = torch.zeros(nh * HD, dtype=torch.bfloat16, device=DEV)
    ops.attn_decode_kv8(qkvs[0][1], one, cos, sin, p1, o1, nh, NKV, 65, SCALE)
    assert torch.equal(ox[1], o1)
    for a, b in zip(kvx, one):
        assert torch.equal(a[1], b)


# ---------------------------------------------------------------------------------------------------------------- 5. decoder and serving
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


@pytest.fixture(scope="module")
def small(ops, golden_small):
    cfg = golden_small["cfg"]
    assert cfg["llm"]["head_dim"] == 128
    from videollama2_amd.decoder import HipMistralDecoder
    dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, golden_small["seed"], only=_keep), DEV, max_seq_len=256)
    g = torch.Generator().manual_seed(21)
    embeds = [golden_small["inputs_embeds"].to(DEV).bfloat16()] + \
             [(torch.randn(n, dec.D, generator=g) * 0.5).bfloat16().to(DEV) for n in (70, 5, 129)]
    yield dec, embeds
    del dec
    torch.cuda.empty_cache()


def _solo_and_batched(dec, embeds, n_new=8):
    """On whatever weights are selected, fp8 KV on: the graph-replayed solo run == the eager decode_step run, and generate_batch of the first
    three (ragged) prompts == their solo runs, tokens and logits.  Returns the solo runs."""
    solo = [dec.generate(e, max_new_tokens=n_new, use_graph=True, return_logits=True) for e in embeds]
    toks, logits = dec.generate(embeds[0], max_new_tokens=n_new, use_graph=False, return_logits=True)          # eager decode_step
    assert toks.tolist() == solo[0][0].tolist() and torch.equal(logits, solo[0][1])
    outs, bl = dec.generate_batch(embeds[:3], max_new_tokens=n_new, return_logits=True)
    for b in range(3):
        assert outs[b].tolist() == solo[b][0][0].tolist(), b
        assert torch.equal(bl[:, b], solo[b][1]), b
    return solo


def test_decoder_and_serving_on_the_fp8_kv_cache(small):
    from videollama2_amd.serving import ContinuousBatcher
    dec, embeds = small
    assert dec.fp8_kv is False
    p16 = dec.prefill(embeds[0]).clone()
    dec._ensure_batch(3)
    bytes16 = sum(t.element_size() * t.numel() for t in dec._bb["k"] + dec._bb["v"])
    dec.enable_fp8_kv()
    try:
        assert torch.equal(dec.prefill(embeds[0]), p16)                       # the prefill keeps its bits
        solo = _solo_and_batched(dec, embeds)
        bytes8 = sum(t.element_size() * t.numel() for kv8 in dec._bb["kv8"] for t in kv8)
        assert bytes8 <= 0.52 * bytes16, (bytes8, bytes16)
        # a decode step does not touch the 16-bit cache: after a prefill, eager steps leave it as the prefill wrote it
        dec.prefill(embeds[0])
        k16 = [k.clone() for k in dec.kcache]
        dec.tok.fill_(3)
        dec.decode_step(); dec.decode_step()
        assert all(torch.equal(a, b) for a, b in zip(k16, dec.kcache))
        # continuous batching: staggered admission, an early retirement (request 1: 2 tokens), its slot reused by request 3
        n_new = [8, 2, 8, 8]
        for use_graph in (True, False):
            b = ContinuousBatcher(dec, max_slots=3, use_graph=use_graph)
            rid = [b.submit(embeds[0], max_new_tokens=n_new[0]), b.submit(embeds[1], max_new_tokens=n_new[1])]
            b.step()
            rid.append(b.submit(embeds[2], max_new_tokens=n_new[2]))
            b.step(); b.step()
            assert b.slots[1] is None                                           # request 1 has left; a hole below slot 2
            rid.append(b.submit(embeds[3], max_new_tokens=n_new[3]))
            b.step()
            assert b.slots[1] is not None and b.slots[1].rid == rid[3]
            done = b.run()
            assert [done[r].tolist() for r in rid] == [solo[i][0][0, :n_new[i]].tolist() for i in range(4)], use_graph
        # toggling: off restores the 16-bit bits, on again reproduces the first run
        dec.enable_fp8_kv(False)
        assert torch.equal(dec.prefill(embeds[0]), p16)
        t16 = dec.generate(embeds[0], max_new_tokens=8, use_graph=True, return_logits=True)
        dec.enable_fp8_kv()
        again = dec.generate(embeds[0], max_new_tokens=8, use_graph=True, return_logits=True)
        assert again[0].tolist() == solo[0][0].tolist() and torch.equal(again[1], solo[0][1])
        assert not torch.equal(t16[1][1:], again[1][1:])                       # ... and it is another arithmetic
    finally:
        dec.enable_fp8_kv(False)


@pytest.mark.parametrize("fmt", ["fp8", "mxfp4"])
def test_fp8_kv_under_the_quantised_decode_weights(small, fmt):
    dec, embeds = small
    switch = dec.enable_fp8_decode if fmt == "fp8" else dec.enable_mxfp4_decode
    switch()
    dec.enable_fp8_kv()
    try:
        assert dec.decode_format == fmt and dec.fp8_kv
        _solo_and_batched(dec, embeds[:3], n_new=5)
    finally:
        dec.enable_fp8_kv(False)
        switch(False)


def test_model_level_switch_padded_batch_and_model_batcher(ops, golden_small):
    """VideoLLaMA2Hip.enable_fp8_kv forwards to the decoder and forgets the prefix record; the padded-batch generate and ModelBatcher decode on
    the fp8 slots and give each row's solo fp8-KV tokens."""
    from videollama2_amd.model import VideoLLaMA2Hip
    cfg = golden_small["cfg"]
    model = VideoLLaMA2Hip(cfg, O.seeded_state_dict(cfg, golden_small["seed"], round_bf16=True), "cuda:0", max_seq_len=128)
    model._prefix_rec = dict(ids=[1])
    assert model.enable_fp8_kv() is model and model.decoder.fp8_kv and model._prefix_rec is None
    with pytest.raises(NotImplementedError, match="fp8 KV cache is on"):
        model.generate(torch.tensor([[1, 5, 9]]), prefix_cache=True)
    g = torch.Generator().manual_seed(5)
    rows = [torch.randint(3, cfg["llm"]["vocab_size"], (n,), generator=g) for n in (11, 6)]
    ids = torch.zeros((2, 11), dtype=torch.long)
    mask = torch.zeros((2, 11), dtype=torch.long)
    for b, r in enumerate(rows):
        ids[b, :r.numel()], mask[b, :r.numel()] = r, 1
    solo = [model.generate(r[None], max_new_tokens=5)[0].tolist() for r in rows]
    both = model.generate(ids, attention_mask=mask, max_new_tokens=5)
    assert [both[b].tolist() for b in range(2)] == solo
    mb = model.batcher(max_slots=2)
    rid = [mb.submit(r[None], max_new_tokens=5) for r in rows]
    done = mb.run()
    assert [done[r].tolist() for r in rid] == solo
    model.enable_fp8_kv(False)
    assert not model.decoder.fp8_kv and model.decoder.kv8 is None
    del model
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- 6. accuracy, measured
def test_accuracy_against_the_definitions_own_error(small, golden_small, capsys):
    """8 teacher-forced decode steps on the small golden config (the tokens are the 16-bit-KV run's).  Bar: rel-L2 of the fp8-KV logits
    against the 16-bit-KV logits <= the definition's own error (fp32 oracle with its cached rows quantised -> dequantised, against the plain
    fp32 oracle) + the 16-bit path's distance from the plain oracle: the kernel may add the 16-bit path's rounding noise to the format's
    error and nothing else.  The figures are printed (and written to $VL2_FP8KV_PARITY_OUT when set): profiles/r14_fp8kv_parity.json."""
    dec, embeds = small
    x = embeds[0]
    steps = 8
    toks16, l16 = dec.generate(x, max_new_tokens=steps + 1, use_graph=False, return_logits=True)
    forced = toks16[0, :steps].tolist()
    dec.enable_fp8_kv()
    try:
        rows = [dec.prefill(x).clone()]
        for t in forced:
            dec.tok.fill_(t)
            rows.append(dec.decode_step().clone())
        l8 = torch.stack(rows)
    finally:
        dec.enable_fp8_kv(False)
    assert torch.equal(l8[0], l16[0])
    cfg = golden_small["cfg"]
    sd = {k: v.float() for k, v in O.seeded_state_dict(cfg, golden_small["seed"], only=_keep).items()}
    xf = x.float().cpu()
    plain = KV.teacher_forced_logits(sd, cfg, xf, forced, kv8=False)
    quant = KV.teacher_forced_logits(sd, cfg, xf, forced, kv8=True)
    ours = rel(l8[1:], l16[1:])
    definition = rel(quant[1:], plain[1:])
    base16 = rel(l16[1:], plain[1:])
    ours_vs_def = rel(l8[1:], quant[1:])
    undecidable, differ = 0, 0
    for s in range(1, steps + 1):
        if int(l8[s].argmax()) != int(l16[s].argmax()):
            differ += 1
            ok, margin, dmax = token_tie_ok(l8[s], plain[s])
            undecidable += int(ok)
            assert ok, (s, margin, dmax)
    fig = dict(config="tests/golden/small_T4.pt decoder, 8 teacher-forced steps", fp8kv_vs_16bitkv_rel_l2=ours,
               definition_vs_plain_oracle_rel_l2=definition, kv16_vs_plain_oracle_rel_l2=base16, fp8kv_vs_definition_rel_l2=ours_vs_def,
               bar=definition + base16, greedy_tokens_differing=differ, of_which_undecidable=undecidable)
    with capsys.disabled():
        print("\nfp8kv parity:", json.dumps(fig))
    if os.environ.get("VL2_FP8KV_PARITY_OUT"):
        json.dump(fig, open(os.environ["VL2_FP8KV_PARITY_OUT"], "w"), indent=1)
    assert definition > 0
    assert ours <= definition + base16, fig
