"""Batched decode over a shared prompt prefix on the device: vl2_attn_decode_shared (csrc/k_attn_shared.h, the SHARED
form of csrc/k_attn_append.h) against the fp32 definition, its row stability, its agreement with the unshared kernel, graph = eager, the
decoder mode `generate_batch(shared_prefix=...)` on the small golden configs against the fp32 oracle with the plain batched path as the
floor, the model-level `generate_shared`, and the slot memory.  Every test needs the new entry points: none passes without them."""
import json
import os

import pytest
import torch

from oracle import vl2_oracle as O
from tests.util import TOL_BF16_OUT, rel, token_tie_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"
NKV, HD, CAP, PMAX, ROWS, NBMAX = 2, 128, 192, 256, 512, 33
SCALE = HD ** -0.5
OWN = (0, 1, 62, 63, 64, 65)                 # own rows before the step, mixed within one launch
ROPE_CFG = dict(llm=dict(head_dim=HD, rope_theta=1e6))
GUARD = 1024                                 # sentinel floats on each side of the partial region
SENT = 12345.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib, ops as o
    _lib.load()
    return o


class Ref:
    """Computed once per element type and left unchanged: the prefix caches, 33 private caches, un-roped qkv rows for both groups and the
    RoPE tables of the oracle."""

    def __init__(self, elem):
        g = torch.Generator().manual_seed(7)
        rnd = lambda *s: torch.randn(*s, generator=g).to(elem).to(DEV)
        self.elem = elem
        self.kpre, self.vpre = rnd(NKV, PMAX, HD), rnd(NKV, PMAX, HD)
        self.kown, self.vown = rnd(NBMAX, NKV, CAP, HD), rnd(NBMAX, NKV, CAP, HD)
        self.qkv = {grp: (torch.randn(NBMAX, (NKV * grp + 2 * NKV) * HD, generator=g) * 1.5).to(elem).to(DEV) for grp in (4, 7)}
        cos, sin = O.rope_cos_sin(ROPE_CFG, torch.arange(ROWS))
        self.cos_full, self.sin_full = cos.to(DEV), sin.to(DEV)                     # [ROWS, 128] (the oracle's cat(freqs, freqs))
        self.cos, self.sin = cos[:, :HD // 2].contiguous().to(DEV), sin[:, :HD // 2].contiguous().to(DEV)


_REFS = {}


def _ref(elem):
    if elem not in _REFS:
        _REFS[elem] = Ref(elem)
    return _REFS[elem]


def _owns(nb, shift):
    return [OWN[(b + shift) % len(OWN)] for b in range(nb)]


def _definition(r, grp, src, P, own):
    """fp32 truth of request `src` (its qkv row and private cache) with `own` rows before the step: the oracle's RoPE at position P + own
    (q and the new k rounded through the element type, as the cache holds them), softmax over prefix ++ own rows ++ the new row."""
    nh, pos = NKV * grp, P + own
    row = r.qkv[grp][src].float()
    q, kn, vn = row[:nh * HD].view(nh, HD), row[nh * HD:(nh + NKV) * HD].view(NKV, HD), row[(nh + NKV) * HD:].view(NKV, HD)
    c, s = r.cos_full[pos], r.sin_full[pos]
    qr = (q * c + O.rotate_half(q) * s).to(r.elem).float()
    kr = (kn * c + O.rotate_half(kn) * s).to(r.elem)
    k = torch.cat([r.kpre[:, :P], r.kown[src, :, :own], kr[:, None]], 1).float().repeat_interleave(grp, 0)
    v = torch.cat([r.vpre[:, :P], r.vown[src, :, :own], vn.to(r.elem)[:, None]], 1).float().repeat_interleave(grp, 0)
    p = torch.softmax(torch.einsum("hd,hsd->hs", qr, k) * SCALE, -1)
    return torch.einsum("hs,hsd->hd", p, v).reshape(-1), kr


def _run_shared(ops, r, grp, P, srcs, owns):
    """One shared step for the requests `srcs` (rows of r.qkv / slots of r.kown) placed at slots 0 .. len-1, with sentinels around the
    private caches and the partial region.  Returns (out [nb, nh*128], kown, vown after the step incl. guard slots, checks done)."""
    nh, nb = NKV * grp, len(srcs)
    idx = torch.tensor(srcs, device=DEV)
    kown = torch.full((nb + 2, NKV, CAP, HD), 3.0, dtype=r.elem, device=DEV)
    vown = torch.full((nb + 2, NKV, CAP, HD), -3.0, dtype=r.elem, device=DEV)
    kown[1:nb + 1], vown[1:nb + 1] = r.kown[idx], r.vown[idx]
    k0, v0 = kown.clone(), vown.clone()
    need = nb * ops.shared_partial_floats(P, CAP, nh)
    pbuf = torch.full((need + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
    qkv = r.qkv[grp][idx].contiguous()
    pos = torch.tensor([P + o for o in owns], dtype=torch.int32, device=DEV)
    out = torch.zeros(nb, nh * HD, dtype=r.elem, device=DEV)
    ops.attn_decode_shared(qkv, r.kpre, r.vpre, kown[1:nb + 1], vown[1:nb + 1], r.cos, r.sin, pbuf[GUARD:GUARD + need], out, nh, NKV, P, pos, SCALE)
    torch.cuda.synchronize()
    assert bool((pbuf[:GUARD] == SENT).all()) and bool((pbuf[GUARD + need:] == SENT).all()), "partial sentinels"
    for t, t0 in ((kown, k0), (vown, v0)):
        assert torch.equal(t[0], t0[0]) and torch.equal(t[nb + 1], t0[nb + 1]), "guard slots"
        for b, o in enumerate(owns):                          # only the appended row of a slot changes
            keep = torch.ones(CAP, dtype=torch.bool, device=DEV)
            keep[o] = False
            assert torch.equal(t[b + 1][:, keep], t0[b + 1][:, keep]), b
    return out, kown[1:nb + 1], vown[1:nb + 1], qkv, pos


def _check_case(ops, r, grp, P, nb):
    nh = NKV * grp
    srcs, owns = list(range(nb)), _owns(nb, P)
    out, kown, vown, qkv, pos = _run_shared(ops, r, grp, P, srcs, owns)
    from videollama2_amd import _lib
    assert ops.shared_partial_floats(P, CAP, nh) == int(_lib.load().vl2_attn_decode_shared_partial_floats(P, CAP, nh))
    worst = 0.0
    for b in range(nb):
        truth, kr = _definition(r, grp, srcs[b], P, owns[b])
        e = rel(out[b], truth)
        worst = max(worst, e)
        assert e <= TOL_BF16_OUT, (grp, P, nb, b, owns[b], e)
    # the appended private row: the bytes vl2_attn_decode appends for the same qkv row and position (the requests that cover every own length)
    scratch_k = torch.zeros(NKV, ROWS, HD, dtype=r.elem, device=DEV)
    scratch_v = torch.zeros(NKV, ROWS, HD, dtype=r.elem, device=DEV)
    p1 = torch.empty(nh * (ROWS // 64) * 130, dtype=torch.float32, device=DEV)
    o1 = torch.empty(nh * HD, dtype=r.elem, device=DEV)
    for b in range(min(nb, len(OWN))):
        ops.attn_decode(qkv[b], scratch_k, scratch_v, r.cos, r.sin, p1, o1, nh, NKV, P + owns[b], SCALE)
        assert torch.equal(kown[b][:, owns[b]], scratch_k[:, P + owns[b]]) and torch.equal(vown[b][:, owns[b]], scratch_v[:, P + owns[b]]), b
    # agreement with the unshared kernel on full private copies (to rounding: the prefix sums run on the matrix pipe in another order)
    kf = torch.zeros(nb, NKV, ROWS, HD, dtype=r.elem, device=DEV)
    vf = torch.zeros_like(kf)
    kf[:, :, :P], vf[:, :, :P] = r.kpre[:, :P], r.vpre[:, :P]
    for b in range(nb):
        kf[b, :, P:P + owns[b]], vf[b, :, P:P + owns[b]] = r.kown[srcs[b], :, :owns[b]], r.vown[srcs[b], :, :owns[b]]
    pB = torch.empty(nb * nh * (ROWS // 64) * 130, dtype=torch.float32, device=DEV)
    ob = torch.zeros_like(out)
    ops.attn_decode_batched(qkv, kf, vf, r.cos, r.sin, pB, ob, nh, NKV, pos, ROWS, SCALE)
    torch.cuda.synchronize()
    worst_u = max(rel(out[b], ob[b]) for b in range(nb))
    assert worst_u <= TOL_BF16_OUT, (grp, P, nb, worst_u)
    return worst, worst_u


@pytest.mark.parametrize("nb", [1, 2, 5, 33])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("grp", [4, 7], ids=["group4", "group7"])
@pytest.mark.parametrize("elem", ["bf16", "fp16"])
def test_operator_against_the_fp32_definition_and_the_unshared_kernel(ops, elem, grp, P, nb):
    """Both builds: rel <= TOL_BF16_OUT per request against the fp32 definition AND against vl2_attn_decode_batched on full private copies;
    sentinels around the private caches and the partial region untouched; the appended row byte-equal to vl2_attn_decode's."""
    from videollama2_amd import _lib
    _lib.set_elem(elem)
    try:
        worst, worst_u = _check_case(ops, _ref(torch.float16 if elem == "fp16" else torch.bfloat16), grp, P, nb)
    finally:
        _lib.set_elem("bf16")
    print(f"[shared-prefix {elem}] group {grp} P {P} nb {nb}: vs fp32 {worst:.2e}, vs unshared kernel {worst_u:.2e}")


@pytest.mark.parametrize("grp", [4, 7], ids=["group4", "group7"])
@pytest.mark.parametrize("P", [65, 200])
def test_row_stability(ops, grp, P):
    """A request's output bits do not depend on nb, on its slot or on the other requests' positions: alone, at slot 0 of 5, at slot 32 of 33."""
    r = _ref(torch.bfloat16)
    for src, own in ((3, 63), (4, 65)):
        alone = _run_shared(ops, r, grp, P, [src], [own])[0][0]
        others5 = [s for s in range(NBMAX) if s != src][:4]
        of5 = _run_shared(ops, r, grp, P, [src] + others5, [own] + _owns(4, 1))[0][0]
        others33 = [s for s in range(NBMAX) if s != src]
        of33 = _run_shared(ops, r, grp, P, others33 + [src], _owns(32, 2) + [own])[0][32]
        assert torch.equal(alone, of5) and torch.equal(alone, of33), (grp, P, src)


class _Peaky:
    """The bf16 Ref with ONE prefix key of kv head 0, in the SECOND 64-key tile of the first split, aligned with q head 0 of request `neigh`
    as roped at its position: that row's score there exceeds its first-tile maximum by more than the prefix phase's deferred-rescale
    threshold (6 in the exp2 domain), the case in which a decision taken over a whole wave would reach the rows of other requests."""
    KEY = 100

    def __init__(self, r, grp, P, neigh, own_n):
        self.__dict__.update(r.__dict__)
        self.kpre = r.kpre.clone()
        self.kpre[0, self.KEY] = (0.5 * self.roped_q(grp, neigh, P + own_n)[0]).to(r.elem)

    def roped_q(self, grp, src, pos):
        nh = NKV * grp
        q = self.qkv[grp][src].float()[:nh * HD].view(nh, HD)
        return (q * self.cos_full[pos] + O.rotate_half(q) * self.sin_full[pos]).to(self.elem).float()

    def tile_maxima(self, grp, src, pos):
        """exp2-domain maxima of the first and second 64-key tile for the q heads of kv head 0."""
        s = self.roped_q(grp, src, pos)[:grp] @ self.kpre[0, :128].float().T * (SCALE * 1.4426950408889634)
        return s[:, :64].max(1).values, s[:, 64:].max(1).values


@pytest.mark.parametrize("grp", [4, 7], ids=["group4", "group7"])
def test_row_stability_next_to_a_peaky_row_in_the_same_wave(ops, grp):
    """P = 200: the first prefix split holds two tiles.  A neighbour in the probed request's 32-row wave rescales in the second tile (its
    maximum jumps by more than 6); the probed request has a row whose second-tile maximum lies only slightly above its first, i.e. a row
    that must NOT rescale there.  Its bits alone, next to the neighbour at slot 0 / 1 of 5, and at slots 30 / 29 of 33 (one wave at both
    group sizes) must be equal."""
    P, neigh, own_n = 200, 7, 1
    r = _Peaky(_ref(torch.bfloat16), grp, P, neigh, own_n)
    m1, m2 = r.tile_maxima(grp, neigh, P + own_n)
    assert float(m2[0] - m1[0]) > 8.0                                            # the neighbour's jump
    probes = []
    for src in range(8, 20):
        for own in (63, 1):
            a, b = r.tile_maxima(grp, src, P + own)
            if bool(((b - a > 0.25) & (b - a < 5.0)).any()) and bool((b - a < 5.0).all()):
                probes.append((src, own))
                break
    assert len(probes) >= 3, probes
    for src, own in probes[:3]:
        alone = _run_shared(ops, r, grp, P, [src], [own])[0][0]
        rest = [s for s in range(NBMAX) if s not in (src, neigh)]
        of5 = _run_shared(ops, r, grp, P, [src, neigh] + rest[:3], [own, own_n] + _owns(3, 1))[0][0]
        srcs33 = rest[:29] + [neigh, src] + rest[29:31]
        of33 = _run_shared(ops, r, grp, P, srcs33, _owns(29, 2) + [own_n, own] + _owns(2, 4))[0][30]
        assert torch.equal(alone, of5), (grp, src, "slot 0 of 5")
        assert torch.equal(alone, of33), (grp, src, "slot 30 of 33")


def test_wrappers_and_library_refuse_bad_arguments(ops):
    r = _ref(torch.bfloat16)
    nh = 8
    qkv, pos = r.qkv[4][:2].contiguous(), torch.tensor([70, 71], dtype=torch.int32, device=DEV)
    out = torch.zeros(2, nh * HD, dtype=torch.bfloat16, device=DEV)
    part = torch.empty(2 * ops.shared_partial_floats(65, CAP, nh), dtype=torch.float32, device=DEV)
    good = dict(qkv=qkv, kprefix=r.kpre, vprefix=r.vpre, kown=r.kown[:2], vown=r.vown[:2], cos_t=r.cos, sin_t=r.sin, partial=part, out=out,
                nh=nh, nkv=NKV, P=65, pos_dev=pos, scale=SCALE)
    for kw, msg in ((dict(P=0), "outside the prefix cache"), (dict(P=PMAX + 1), "outside the prefix cache"), (dict(partial=part[:-1]), "partial holds"),
                    (dict(kown=r.kown[:2, :, :100], vown=r.vown[:2, :, :100]), "contiguous slots"), (dict(cos_t=r.cos[:100], sin_t=r.sin[:100]), "cos / sin"),
                    (dict(nh=7), "nh = nkv")):
        with pytest.raises(ValueError, match=msg):
            ops.attn_decode_shared(**{**good, **kw})
    from videollama2_amd import _lib
    lib = _lib.load()
    p = lambda t: t.data_ptr()
    rc = lib.vl2_attn_decode_shared(p(qkv), p(r.kpre), p(r.vpre), p(r.kown), p(r.vown), p(r.cos), p(r.sin), p(part), part.numel(), p(out), 2,
                                    qkv.stride(0), r.kown.stride(0), out.stride(0), nh, NKV, 65, PMAX, 100, ROWS, p(pos), SCALE, None)
    assert rc == -2 and "multiple of 64" in lib.vl2_last_error_string().decode()


# ---------------------------------------------------------------------------------------------------------------- decoder
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


def _decoder(golden, max_seq_len=256):
    from videollama2_amd.decoder import HipMistralDecoder
    cfg = golden["cfg"]
    assert cfg["llm"]["head_dim"] == 128
    sd = O.seeded_state_dict(cfg, golden["seed"], only=_keep)
    return HipMistralDecoder(cfg, sd, DEV, max_seq_len=max_seq_len), sd


def _prompts(golden, D, lens=(1, 5, 17), seed=31):
    g = torch.Generator().manual_seed(seed)
    prefix = golden["inputs_embeds"].bfloat16()
    return prefix, [(torch.randn(n, D, generator=g) * 0.5).bfloat16() for n in lens]


def test_graph_equals_eager_and_a_request_at_its_capacity_stops_writing(ops, golden_small):
    """Three steps of the shared step, eager and as three replays of ONE captured graph, from the same state: logits, tokens and private
    caches bit for bit.  Slot 0 sits one row below its private capacity (own_cap 64, 63 rows held): the first step writes its last row,
    the next two must write nothing (row 64 of its last kv head would be row 0 of slot 1)."""
    dec, _ = _decoder(golden_small)
    prefix, suf = _prompts(golden_small, dec.D, lens=(62, 1, 5))
    P = prefix.shape[0]
    dec.generate_batch([s.to(DEV) for s in suf], max_new_tokens=2, use_graph=False, shared_prefix=prefix.to(DEV))
    sp = dec._sp
    assert sp["own_cap"] == 64 and sp["pos"].tolist() == [P + 63, P + 2, P + 6]
    attend = dec._shared_attend(sp, 3)
    keys = ("tok", "pos", "logits")
    saved = {k: sp[k].clone() for k in keys}
    saved_kv = [(k.clone(), v.clone()) for k, v in zip(sp["k"], sp["v"])]

    def restore():
        for k in keys:
            sp[k].copy_(saved[k])
        for li, (k, v) in enumerate(saved_kv):
            sp["k"][li].copy_(k); sp["v"][li].copy_(v)

    def record():
        torch.cuda.synchronize()
        return sp["logits"].clone(), sp["tok"].clone()

    step = lambda: dec._batched_step(3, False, sp, attend)
    eager = []
    for _ in range(3):
        step()
        eager.append(record())
    assert sp["pos"].tolist() == [P + 66, P + 5, P + 9]
    eager_kv = [(k.clone(), v.clone()) for k, v in zip(sp["k"], sp["v"])]
    for li, (k, v) in enumerate(eager_kv):                  # slot 0: row 63 written by the first step, nothing past it
        assert not torch.equal(k[0, :, 63], saved_kv[li][0][0, :, 63])
        assert torch.equal(k[0, :, :63], saved_kv[li][0][0, :, :63]) and torch.equal(v[0, :, :63], saved_kv[li][1][0, :, :63])
        assert torch.equal(k[1, :, 0], saved_kv[li][0][1, :, 0]) and torch.equal(v[1, :, 0], saved_kv[li][1][1, :, 0])
    restore()
    g = dec._capture(step, step, (sp["tok"], sp["pos"], sp["logits"], sp["sstep"]))
    for s in range(3):
        g.replay()
        lg, tk = record()
        lo = 0 if s == 0 else 1                             # slot 0's first step is a valid one; its later steps are discarded ones
        assert torch.equal(lg[lo:], eager[s][0][lo:]) and torch.equal(tk[lo:], eager[s][1][lo:]), s
    for (k, v), (ke, ve) in zip(zip(sp["k"], sp["v"]), eager_kv):
        assert torch.equal(k, ke) and torch.equal(v, ve)


def test_sampled_shared_step_graph_equals_eager_and_repeats_with_the_seed(ops, golden_small):
    """The sampled step (one ops.sample_tokens launch on the shared mode's buffers): the graph-replayed run, the eager run and a second
    run from the same seed give the same tokens and logits; another seed draws from the same first-step logits."""
    dec, _ = _decoder(golden_small)
    prefix, suf = _prompts(golden_small, dec.D)
    runs = []
    for seed, graph in ((3, True), (3, False), (3, True), (4, True)):
        gen = torch.Generator(device=DEV).manual_seed(seed)
        outs, lg = dec.generate_batch([s.to(DEV) for s in suf], max_new_tokens=6, return_logits=True, use_graph=graph,
                                      sampler=(0.9, 20, 0.95, gen), shared_prefix=prefix.to(DEV))
        runs.append(([o.tolist() for o in outs], lg))
    for toks, lg in runs[1:3]:
        assert toks == runs[0][0] and torch.equal(lg, runs[0][1])
    assert torch.equal(runs[3][1][0], runs[0][1][0])
    greedy = dec.generate_batch([s.to(DEV) for s in suf], max_new_tokens=6, shared_prefix=prefix.to(DEV))
    assert runs[0][0] != [o.tolist() for o in greedy] or runs[3][0] != runs[0][0]      # the draws are draws, not the argmax


def _errors_against_the_oracle(logits, toks_ref, lg_ref):
    """Per request: worst rel-L2 of the free-running logits against the oracle's over the steps up to the first step whose token differs
    from the oracle's (that step included: its history is still the oracle's); a differing token must be a tie the logit error cannot
    resolve (token_tie_ok)."""
    worst = 0.0
    for b in range(len(toks_ref)):
        for s in range(logits.shape[0]):
            worst = max(worst, rel(logits[s, b], lg_ref[b][s]))
            if int(logits[s, b].argmax()) != toks_ref[b][s]:
                ok, margin, dmax = token_tie_ok(logits[s, b], lg_ref[b][s])
                assert ok, f"request {b} step {s}: token differs from the oracle's with margin {margin:.3e} >= 2 * {dmax:.3e}"
                break
    return worst


@pytest.mark.parametrize("fmt", ["16bit", "fp8"])
@pytest.mark.parametrize("which", ["small", "v21"])
def test_decoder_mode_against_the_fp32_oracle_with_the_plain_batched_path_as_the_floor(ops, golden_small, golden_small_v21, which, fmt, capsys):
    """Prompts = prefix ++ suffixes of 1, 5 and 17 rows.  Free-running per-step logits of the shared mode and of the plain generate_batch on
    the full prompts, both against the fp32 oracle (fp8: the oracle on the dequantised weights).  Bar: shared <= max(2 x plain, 4e-3)."""
    golden = golden_small if which == "small" else golden_small_v21
    dec, sd = _decoder(golden)
    cfg, n_new = golden["cfg"], 6
    prefix, suf = _prompts(golden, dec.D)
    sd_ref = sd
    if fmt == "fp8":
        from tests.test_gpu_parity_full import dequantised_llm_weights
        dec.enable_fp8_decode()
        sd_ref = dequantised_llm_weights(sd, cfg)
    toks_ref, lg_ref = [], []
    with torch.no_grad():
        for s in suf:
            t, lg = O.greedy_generate(sd_ref, cfg, torch.cat([prefix, s]).float(), n_new)
            toks_ref.append(t); lg_ref.append(lg)
    full = [torch.cat([prefix, s]).to(DEV) for s in suf]
    _, plain = dec.generate_batch(full, max_new_tokens=n_new, return_logits=True)
    outs, shared = dec.generate_batch([s.to(DEV) for s in suf], max_new_tokens=n_new, return_logits=True, shared_prefix=prefix.to(DEV))
    e_plain = _errors_against_the_oracle(plain, toks_ref, lg_ref)
    e_shared = _errors_against_the_oracle(shared, toks_ref, lg_ref)
    d = max(rel(shared[0, b], plain[0, b]) for b in range(3))
    fig = dict(config=f"{which} golden decoder, {fmt} decode weights, prefix {prefix.shape[0]} rows ++ suffixes 1 / 5 / 17, {n_new} free-running steps",
               shared_vs_fp32_oracle=e_shared, plain_batched_vs_fp32_oracle=e_plain, shared_vs_plain_first_step=d)
    with capsys.disabled():
        print(f"\n[shared-prefix parity] {json.dumps(fig)}")
    path = os.environ.get("VL2_SHARED_PREFIX_PARITY_OUT")          # e.g. profiles/r15_shared_prefix_parity.json: the figures are appended to it
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        rows = json.load(open(path)) if os.path.exists(path) else []
        json.dump(rows + [fig], open(path, "w"), indent=1)
    assert e_shared <= max(2.0 * e_plain, 4e-3), fig
    assert all(o.numel() == n_new for o in outs)


def test_slot_memory(ops, golden_small):
    dec, _ = _decoder(golden_small)
    prefix, suf = _prompts(golden_small, dec.D)
    dec.generate_batch([s.to(DEV) for s in suf], max_new_tokens=8, shared_prefix=prefix.to(DEV))
    own_cap = ops.shared_own_cap(17, 8)
    assert own_cap == 64 and dec._sp["own_cap"] == own_cap
    got = sum(t.numel() * t.element_size() for t in dec._sp["k"] + dec._sp["v"])
    assert got == 3 * dec.n_layers * 2 * dec.nkv * own_cap * 128 * 2
    assert got < 3 * dec.n_layers * 2 * dec.nkv * dec.max_seq_len * 128 * 2


def test_model_one_video_three_questions(ops, golden_small):
    """generate_shared: the tower is entered once, on one video's frames; the tokens equal the plain batched generate's wherever
    token_tie_ok does not excuse a step."""
    from videollama2_amd.model import VideoLLaMA2Hip
    g = golden_small
    cfg = g["cfg"]
    model = VideoLLaMA2Hip(cfg, O.seeded_state_dict(cfg, g["seed"], round_bf16=True), "cuda:0", max_seq_len=256)
    gen = torch.Generator().manual_seed(5)
    frames = g["frames"].to("cuda:0")
    reqs = [(torch.cat([g["input_ids"], torch.randint(3, cfg["llm"]["vocab_size"], (n,), generator=gen)]), [(frames, "video")]) for n in (1, 5, 17)]
    seen = []
    hook = model.vision_tower.register_forward_pre_hook(lambda m, a: seen.append(a[0].shape[0]))
    try:
        outs, lg = model.generate_shared(reqs, max_new_tokens=6, return_logits=True)
        assert seen == [frames.shape[0]], seen
    finally:
        hook.remove()
    assert model.decoder._sp["P"] == g["inputs_embeds"].shape[0]
    ref, lg_ref = model.generate_batch(reqs, max_new_tokens=6, return_logits=True)
    for b in range(3):
        for s, (a, c) in enumerate(zip(outs[b].tolist(), ref[b].tolist())):
            if a != c:
                ok, margin, dmax = token_tie_ok(lg[s, b], lg_ref[s, b])
                assert ok, (b, s, margin, dmax)
                break
    # different videos are not merged: the plain path answers, the same tokens as generate_batch
    other = [(reqs[0][0], [(frames.flip(0).contiguous(), "video")]), reqs[1]]
    sp_before = model.decoder._sp
    got = model.generate_shared(other, max_new_tokens=3)
    want = model.generate_batch(other, max_new_tokens=3)
    assert [o.tolist() for o in got] == [o.tolist() for o in want] and model.decoder._sp is sp_before
