"""The batched draw of a decode step on MI355X: `vl2_sample_tokens` (csrc/k_sample.h sample_rows_kernel, one launch for nb rows) against the
single-row kernels it shares its bodies with (every sampled row = `vl2_sample_token` at its u, every greedy row = `vl2_argmax`), eager and from a
captured graph; `generate_batch(sampler=...)`, the continuous batcher with mixed greedy and sampled requests, and the model-level
`generate_batch(do_sample=True)` against the solo decodes."""
import pytest
import torch

from oracle import sampling_oracle as SO
from oracle import vl2_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (temperature, top_k, top_p) per row; temperature <= 0 = greedy
ROWS = [(0.0, 0, 1.0), (0.2, 50, 1.0), (0.7, 0, 0.9), (1.3, 40, 0.8), (0.7, 1, 1.0), (-1.0, 50, 0.9), (1.0, 20, 0.95)]


def _mixed_batch(V, ld_pad=64, n_u=16):
    """Logits on a 0.5 grid (exact ties everywhere, the top-k / top-p boundaries and the greedy maximum included), in a buffer wider than V."""
    g = torch.Generator().manual_seed(V)
    nb = len(ROWS)
    x = torch.round(torch.randn(nb, V, generator=g) * 6) / 2
    x[0, 5] = x[0, V - 7] = x[0].max() + 1.0                       # a tied maximum: the first index wins
    x[4, 11] = x[4, 12] = x[4].max() + 0.5                          # top_k = 1 on a tie: both kept
    buf = torch.zeros(nb, V + ld_pad)
    buf[:, :V] = x
    u = torch.rand(nb, n_u, generator=g)
    u[1, 0], u[2, 1] = 0.0, 0.99999994
    T = torch.tensor([r[0] for r in ROWS], dtype=torch.float32)
    K = torch.tensor([r[1] for r in ROWS], dtype=torch.int32)
    P = torch.tensor([r[2] for r in ROWS], dtype=torch.float32)
    step0 = torch.tensor([0, 0, 1, 3, 2, 5, 7], dtype=torch.int32)
    return [t.to(DEV) for t in (buf, T, K, P, u, step0)]


def _single_row_tokens(ops, logits, u, steps):
    """What the single-row kernels give: vl2_sample_token at u[b, steps[b]] for a sampled row, vl2_argmax for a greedy one."""
    tok = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = []
    for b, (T, k, p) in enumerate(ROWS):
        if T > 0:
            ops.sample_token(logits[b].contiguous(), tok, u[b].contiguous(), T, k, p, step=int(steps[b]))
        else:
            ops.argmax(logits[b].contiguous(), tok)
        out.append(int(tok.item()))
    return out


@pytest.mark.parametrize("V", [32000, 152064])
def test_sample_tokens_equals_the_single_row_kernels(V):
    from videollama2_amd import ops
    buf, T, K, P, u, step0 = _mixed_batch(V)
    logits = buf[:, :V]
    sampled = (T > 0).to(torch.int32)
    tok = torch.full((len(ROWS),), -1, dtype=torch.int32, device=DEV)
    step = step0.clone()
    seq = []
    for i in range(4):                                             # consecutive draws: each reads and advances its own step
        ops.sample_tokens(logits, T, K, P, u, step, tok)
        ref = _single_row_tokens(ops, logits, u, (step0 + i * sampled).tolist())
        assert tok.tolist() == ref, (V, i)
        assert torch.equal(step, step0 + (i + 1) * sampled)
        seq.append(ref)
    assert tok[0] == 5 and int(tok[4]) in (11, 12)                  # argmax: the first of a tied maximum; top_k = 1 keeps the whole tie
    assert seq[0][0] == seq[3][0] and seq[0][5] == seq[3][5]        # greedy rows do not depend on the step
    for _ in range(20):                                            # deterministic: integer fixed-point mass
        step.copy_(step0)
        ops.sample_tokens(logits, T, K, P, u, step, tok)
        assert tok.tolist() == seq[0]


def test_captured_launch_reads_and_advances_the_step_on_the_device():
    from videollama2_amd import ops
    V = 32000
    buf, T, K, P, u, step0 = _mixed_batch(V)
    logits = buf[:, :V]
    sampled = (T > 0).to(torch.int32)
    tok = torch.zeros((len(ROWS),), dtype=torch.int32, device=DEV)
    step = step0.clone()
    eager = []
    for _ in range(5):
        ops.sample_tokens(logits, T, K, P, u, step, tok)
        eager.append(tok.tolist())
    step.copy_(step0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        ops.sample_tokens(logits, T, K, P, u, step, tok)
    assert torch.equal(step, step0)                                # capture ran nothing
    got = []
    for _ in range(5):
        g.replay()
        got.append(tok.tolist())
    assert got == eager and torch.equal(step, step0 + 5 * sampled)


@pytest.fixture(scope="module")
def small_model(golden_small):
    from videollama2_amd.model import VideoLLaMA2Hip
    g = golden_small
    cfg = g["cfg"]
    return VideoLLaMA2Hip(cfg, O.seeded_state_dict(cfg, g["seed"], round_bf16=True), DEV, max_seq_len=64)


@pytest.mark.parametrize("n_req", [3, 6])
def test_generate_batch_sampled_graph_and_eager_equal_the_per_request_draws(golden_small, small_model, n_req):
    """Every token = ops.sample_token on that request's returned logits of the step at its recomputed u row (the per-request loop this replaces);
    graph == eager; at nb >= GEMM_BATCH (the skinny-M step) also inside the oracle's kept set and CDF interval."""
    from videollama2_amd import ops
    m = small_model
    emb = golden_small["inputs_embeds"].to(DEV)
    reqs = [emb, emb[:30], emb[:37], emb[:25], emb[:41], emb[:33]][:n_req]
    T, K, Pp, n_new = 1.1, 20, 0.9, 6
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)
    runs = {}
    for use_graph in (True, False):
        runs[use_graph] = m.decoder.generate_batch(reqs, max_new_tokens=n_new, return_logits=True, use_graph=use_graph, sampler=(T, K, Pp, gen()))
    (tg, lg), (te, le) = runs[True], runs[False]
    assert [t.tolist() for t in tg] == [t.tolist() for t in te] and torch.equal(lg, le)
    g2 = gen()
    n_u = min(n_new, m.decoder.max_seq_len) + 1
    us = torch.stack([torch.rand((n_u,), device=DEV, generator=g2) for _ in reqs])
    tok = torch.zeros(1, dtype=torch.int32, device=DEV)
    for b in range(n_req):
        assert tg[b].numel() == n_new
        for s in range(n_new):
            ops.sample_token(lg[s, b].contiguous(), tok, us[b], T, K, Pp, step=s)
            assert int(tg[b][s]) == int(tok.item()), (b, s)
            if n_req >= m.decoder.GEMM_BATCH:
                pr = SO.probs(lg[s, b].cpu(), T, K, Pp)
                t = int(tg[b][s])
                assert pr[t] > 0 or t in SO.boundary_tokens(lg[s, b].cpu(), T, K, Pp), (b, s)
                cdf = pr.double().cumsum(0)
                lo, hi = (float(cdf[t - 1]) if t > 0 else 0.0), float(cdf[t])
                assert lo - 2e-5 <= float(us[b, s]) * float(cdf[-1]) <= hi + 2e-5, (b, s)
    assert (n_req, True) in m.decoder._batch_graphs                 # the sampled step's own graph
    greedy = m.decoder.generate_batch(reqs, max_new_tokens=n_new)
    k1 = m.decoder.generate_batch(reqs, max_new_tokens=n_new, sampler=(0.7, 1, 1.0))
    assert [t.tolist() for t in greedy] == [t.tolist() for t in k1]


def test_continuous_batching_mixes_greedy_and_sampled_requests(golden_small, small_model):
    """max_slots = 4 (multi-row GEMV rows are bit-identical to the solo step): staggered admission, early retirement, slot reuse and holes;
    every sampled request equals its solo generate(do_sample=True) under its own seed, every greedy one its solo greedy decode."""
    m = small_model
    g = golden_small
    idsA = g["input_ids"].to(DEV)
    variants = [idsA, torch.cat([idsA[:3], idsA[6:]]), torch.cat([idsA[:2], idsA[5:]]), idsA[:4], torch.cat([idsA[:4], idsA[8:]]), idsA[:6]]
    fr = [g["frames"].to(DEV), torch.flip(g["frames"], dims=[0]).contiguous().to(DEV)]
    samp = [dict(do_sample=True, temperature=1.2, top_k=30, top_p=0.85), None, dict(do_sample=True, temperature=0.7, top_k=0, top_p=0.9), None,
            dict(do_sample=True, temperature=1.5, top_k=50, top_p=1.0), dict(do_sample=True, temperature=0.9)]
    ims = [[(fr[0], "video")], [(fr[1], "video")], [(fr[0], "video")], None, [(fr[1], "video")], None]
    n_new = [9, 3, 6, 4, 7, 5]
    seed = lambda i: torch.Generator(device=DEV).manual_seed(100 + i)
    kw = lambda i: dict(samp[i], generator=seed(i)) if samp[i] else {}
    solo = [m.generate(variants[i][None], attention_mask=torch.ones(1, variants[i].numel(), dtype=torch.long, device=DEV), images=ims[i],
                       max_new_tokens=n_new[i], **kw(i))[0].tolist() for i in range(6)]
    for use_graph in (True, False):
        b = m.batcher(max_slots=4, use_graph=use_graph)
        sub = lambda i: b.submit(variants[i], ims[i], max_new_tokens=n_new[i], **kw(i))
        rid = [sub(0), sub(1)]
        b.step()
        rid += [sub(2), sub(3)]
        b.step(); b.step(); b.step()                                  # request 1 retires: a hole below slot 3
        rid += [sub(4), sub(5)]                                       # one fills the hole, one waits for a slot
        done = b.run()
        assert [done[r].tolist() for r in rid] == solo, use_graph
        assert b.inner.steps < sum(n_new)


def test_model_generate_batch_do_sample(golden_small, small_model):
    m = small_model
    g = golden_small
    ids = g["input_ids"].to(DEV)
    reqs = [(ids, [(g["frames"].to(DEV), "video")]), (torch.cat([ids[:3], ids[6:]]), [(torch.flip(g["frames"], dims=[0]).contiguous().to(DEV), "video")])]
    greedy = m.generate_batch(reqs, max_new_tokens=5)
    k1 = m.generate_batch(reqs, max_new_tokens=5, do_sample=True, temperature=0.6, top_k=1)
    assert [t.tolist() for t in k1] == [t.tolist() for t in greedy]
    out = m.generate_batch(reqs, max_new_tokens=5, do_sample=True, temperature=1.2, top_k=30, top_p=0.9,
                           generator=torch.Generator(device=DEV).manual_seed(4))
    solo = m.generate(ids[None], images=reqs[0][1], attention_mask=torch.ones(1, ids.numel(), dtype=torch.long, device=DEV), max_new_tokens=5,
                      do_sample=True, temperature=1.2, top_k=30, top_p=0.9, generator=torch.Generator(device=DEV).manual_seed(4))
    assert out[0].tolist() == solo[0].tolist()
    with pytest.raises(ValueError, match="temperature"):
        m.generate_batch(reqs, max_new_tokens=2, do_sample=True, temperature=0.0)


def test_sample_tokens_fp16_library_and_bad_arguments():
    from videollama2_amd import _lib, ops
    V = 32000
    buf, T, K, P, u, step0 = _mixed_batch(V)
    logits = buf[:, :V]
    tok = torch.zeros((len(ROWS),), dtype=torch.int32, device=DEV)
    step = step0.clone()
    ops.sample_tokens(logits, T, K, P, u, step, tok)
    bf16 = tok.tolist()
    _lib.set_elem("fp16")
    try:
        _lib.load()
        step.copy_(step0)
        ops.sample_tokens(logits, T, K, P, u, step, tok)             # fp32 logits in, the same kernel in the fp16 build
        assert tok.tolist() == bf16 == _single_row_tokens(ops, logits, u, step0.tolist())
    finally:
        _lib.set_elem("bf16")
    p = lambda t: t.data_ptr()
    good = [p(logits), logits.stride(0), V, len(ROWS), p(T), p(K), p(P), p(u), u.stride(0), p(step), p(tok), None]
    for i, bad in ((0, None), (4, None), (5, None), (6, None), (7, None), (9, None), (10, None), (2, 0), (3, 0), (1, V - 1), (8, 0)):
        args = list(good)
        args[i] = bad
        with pytest.raises(_lib.Vl2HipError, match="vl2_sample_tokens"):
            _lib.call("vl2_sample_tokens", *args)
    with pytest.raises(ValueError):
        ops.sample_tokens(logits, T[:3], K, P, u, step, tok)         # fewer settings than rows
