"""The sampled batched decode step: one vl2_sample_tokens launch over all nb rows (captured with the step) against the per-request path it
replaces (one vl2_sample_token launch per request and step, the step run eagerly), with the greedy step beside them.  HIP events, warm-up +
repeats (median, min, max):
  1. the decoder alone (seeded random weights, every layer), 7B widths (Mistral-7B, V = 32000) and VideoLLaMA2.1 widths (Qwen2-7B, V = 152064),
     nb = 1, 4, 16, 64 requests at a context of --ctx rows: ms per decode step for the greedy graph, the sampled graph and today's eager
     per-request sampling;
  2. the kernel alone at both vocabularies: one vl2_sample_tokens launch over nb rows against nb vl2_sample_token launches.
Sampling settings: temperature 0.7, top_k 50, top_p 0.9 for every request.  Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T_, K_, P_ = 0.7, 50, 0.9


def timed(fn, warmup, reps, inner=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    ts.sort()
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), reps=reps)


def emit(rows, out, **kw):
    print(json.dumps(kw), flush=True)
    rows.append(kw)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


def bench_kernel(rows, a):
    from videollama2_amd import ops
    for V in (32000, 152064):
        for nb in a.nb:
            g = torch.Generator(device="cuda").manual_seed(nb)
            logits = torch.randn(nb, V, device="cuda", generator=g) * 3
            u = torch.rand(nb, 64, device="cuda", generator=g)
            T = torch.full((nb,), T_, device="cuda")
            K = torch.full((nb,), K_, dtype=torch.int32, device="cuda")
            P = torch.full((nb,), P_, device="cuda")
            step = torch.zeros(nb, dtype=torch.int32, device="cuda")
            tok = torch.zeros(nb, dtype=torch.int32, device="cuda")

            def rows_launch():
                step.zero_()
                ops.sample_tokens(logits, T, K, P, u, step, tok)

            def per_row():
                for b in range(nb):
                    ops.sample_token(logits[b], tok[b:b + 1], u[b], T_, K_, P_, step=0)

            t_one = timed(rows_launch, a.warmup, a.reps, inner=10)
            t_per = timed(per_row, a.warmup, a.reps, inner=10)
            rows_launch()
            one = tok.clone()
            per_row()
            emit(rows, a.out, what="sampling kernel alone", V=V, nb=nb, sample_tokens_one_launch=t_one, sample_token_per_row=t_per,
                 same_tokens=bool(torch.equal(one, tok)))


def bench_step(rows, a, family):
    from videollama2_amd import ops
    from videollama2_amd.config import videollama2_1_7b_16f, videollama2_7b
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.weights import LazyRandomStateDict
    cfg = videollama2_7b() if family == "7b" else videollama2_1_7b_16f()
    sd = LazyRandomStateDict(cfg, "cuda", seed=1234)
    dec = HipMistralDecoder(cfg, sd, "cuda", max_seq_len=a.ctx + 256)
    del sd
    torch.cuda.empty_cache()
    V, D = cfg["llm"]["vocab_size"], cfg["llm"]["hidden_size"]
    bb = dec._ensure_batch(max(a.nb))
    x = (0.5 * torch.randn(a.ctx, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))).bfloat16()
    for b in range(max(a.nb)):                            # one prompt in every slot's cache
        dec.prefill(x, cache=([k[b] for k in bb["k"]], [v[b] for v in bb["v"]]), logits_out=bb["logits"][b])
    logits0 = bb["logits"].clone()
    bb["u"].uniform_()
    for nb in a.nb:
        def reset():
            bb["pos"][:nb].fill_(a.ctx)
            bb["sstep"][:nb].zero_()
            bb["logits"].copy_(logits0)

        bb["samp_T"][:nb].fill_(T_); bb["samp_k"][:nb].fill_(K_); bb["samp_p"][:nb].fill_(P_)
        reset()
        g_greedy = dec.capture_batch_graph(nb, False)
        g_sampled = dec.capture_batch_graph(nb, True)
        u = bb["u"]

        def today():                                          # per-request sample_token launches + the eager step (generate_batch before)
            for b in range(nb):
                ops.sample_token(bb["logits"][b], bb["tok"][b:b + 1], u[b], T_, K_, P_, step=0)
            dec._decode_kernels_batched(nb)

        res = {}
        for name, fn in (("greedy_graph", g_greedy.replay), ("sampled_graph", g_sampled.replay), ("sampled_eager_per_request", today),
                         ("greedy_eager", lambda: dec._batched_step(nb, False))):
            reset()
            res[name] = timed(fn, a.warmup, a.reps)
        emit(rows, a.out, what="batched decode step", family=family, V=V, nb=nb, ctx=a.ctx, **res,
             sampled_graph_minus_greedy_graph_ms=round(res["sampled_graph"]["median_ms"] - res["greedy_graph"]["median_ms"], 4),
             today_minus_greedy_graph_ms=round(res["sampled_eager_per_request"]["median_ms"] - res["greedy_graph"]["median_ms"], 4))
    del dec, bb
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", default="1,4,16,64")
    ap.add_argument("--ctx", type=int, default=1650)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="kernel,7b,v21")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.nb = [int(n) for n in a.nb.split(",")]
    assert torch.cuda.is_available(), "batch_sample_bench.py measures on the GPU"
    rows = []
    only = a.only.split(",")
    if "kernel" in only:
        bench_kernel(rows, a)
    for family in ("7b", "v21"):
        if family in only:
            bench_step(rows, a, family)


if __name__ == "__main__":
    with torch.no_grad():
        main()
