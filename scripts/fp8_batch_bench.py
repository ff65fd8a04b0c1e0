"""Batched decode on the fp8 decode weights against the 16-bit weights.  HIP events, warm-up + repeats (median, min, max):
  1. kernel: vl2_gemm_skinny_fp8 (GEMM + ordered reduce) at M = 8, 16, 64 and vl2_gemv_batched_fp8 at MB = 4 on the 7B decode shapes, with
     the 16-bit kernels beside them: us per call and the weight-stream rate (fp8 bytes + row scales, or 16-bit bytes, per second);
  2. step: the 7B decoder at full width (weights generated on the device from a seed), every request with the same --ctx-row prompt in its
     cache slot, nb requests: the graph-replayed batched step on the 16-bit weights and on the fp8 copies, captured once each and alternated
     round by round in one process.  Per point: ms per step, tokens per second, bytes per step from the shapes (weights, row scales, KV cache
     read) and the implied TB/s.  Output check: the replayed fp8 step gives the logits (bit for bit) and next tokens of an eager fp8 step
     from the same state.
Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


SHAPES = [("qkv", 6144, 4096, {}), ("o", 4096, 4096, dict(res=True)), ("gate_up", 28672, 4096, dict(swiglu=True)),
          ("down", 4096, 14336, dict(res=True)), ("lm_head", 32000, 4096, dict(out_f32=True))]


def bench_kernel(rows, a):
    from videollama2_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, N, K, kw in SHAPES:
        w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16()
        q, sc = ops.quant_fp8(w)
        n_out = N // 2 if kw.get("swiglu") else N
        b8, b16 = N * K + 4 * N, 2 * N * K
        for M in a.kernel_m:
            x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
            res = torch.randn(M, n_out, device="cuda", generator=g).bfloat16() if kw.get("res") else None
            kk = dict(swiglu=bool(kw.get("swiglu")), out_f32=bool(kw.get("out_f32")), res=res)
            y = ops.gemm_skinny_fp8(x, q, sc, **kk)
            t8 = timed(lambda: ops.gemm_skinny_fp8(x, q, sc, out=y, **kk), a.warmup, a.reps, inner=20)
            t16 = timed(lambda: ops.gemm_skinny(x, w, out=y, **kk), a.warmup, a.reps, inner=20)
            emit(rows, a.out, what="skinny-M GEMM (+ reduce)", shape=name, N=N, K=K, M=M, fp8_us=round(t8["median_ms"] * 1e3, 2),
                 bf16_us=round(t16["median_ms"] * 1e3, 2), fp8_weight_TBps=round(b8 / (t8["median_ms"] * 1e-3) / 1e12, 3),
                 bf16_weight_TBps=round(b16 / (t16["median_ms"] * 1e-3) / 1e12, 3))
        MB = 4
        x = torch.randn(MB, K, device="cuda", generator=g).bfloat16()
        res = torch.randn(MB, n_out, device="cuda", generator=g).bfloat16() if kw.get("res") else None
        kk = dict(swiglu=bool(kw.get("swiglu")), out_f32=bool(kw.get("out_f32")), res=res)
        y = ops.gemv_batched_fp8(q, sc, x, **kk)
        t8 = timed(lambda: ops.gemv_batched_fp8(q, sc, x, out=y, **kk), a.warmup, a.reps, inner=20)
        t16 = timed(lambda: ops.gemv_batched(w, x, out=y, **kk), a.warmup, a.reps, inner=20)
        emit(rows, a.out, what="multi-row GEMV", shape=name, N=N, K=K, MB=MB, fp8_us=round(t8["median_ms"] * 1e3, 2),
             bf16_us=round(t16["median_ms"] * 1e3, 2), fp8_weight_TBps=round(b8 / (t8["median_ms"] * 1e-3) / 1e12, 3),
             bf16_weight_TBps=round(b16 / (t16["median_ms"] * 1e-3) / 1e12, 3))
        del w, q, sc
        torch.cuda.empty_cache()


def step_bytes(cfg, nb, ctx, fp8):
    """Bytes one batched step moves, from the shapes: the projections and lm_head (fp8: one byte per weight + a 4-byte scale per row, streamed
    once per call of at most 64 rows; 16-bit: two bytes, once), and every request's K and V rows up to its position."""
    l = cfg["llm"]
    D, I, V, L, hd = l["hidden_size"], l["intermediate_size"], l["vocab_size"], l["num_hidden_layers"], l["head_dim"]
    nh, nkv = l["num_attention_heads"], l["num_key_value_heads"]
    mats = [((nh + 2 * nkv) * hd, D), (D, nh * hd), (2 * I, D), (D, I)]
    n_w = L * sum(N * K for N, K in mats) + V * D
    n_rows = L * sum(N for N, _ in mats) + V
    w = (n_w + 4 * n_rows) * math.ceil(nb / 64) if fp8 else 2 * n_w
    kv = nb * L * 2 * nkv * (ctx + 1) * hd * 2
    return w, kv


def bench_step(rows, a):
    from videollama2_amd.config import videollama2_7b
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.weights import LazyRandomStateDict
    cfg = videollama2_7b()
    sd = LazyRandomStateDict(cfg, "cuda", seed=1234)
    dec = HipMistralDecoder(cfg, sd, "cuda", max_seq_len=a.ctx + 256)
    del sd
    torch.cuda.empty_cache()
    dec.enable_fp8_decode()
    D = cfg["llm"]["hidden_size"]
    bb = dec._ensure_batch(max(a.nb))
    x = (0.5 * torch.randn(a.ctx, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))).bfloat16()
    for b in range(max(a.nb)):                            # the same prompt in every slot's cache
        dec.prefill(x, cache=([k[b] for k in bb["k"]], [v[b] for v in bb["v"]]), logits_out=bb["logits"][b])
    logits0 = bb["logits"].clone()
    for nb in a.nb:
        def reset():
            bb["pos"][:nb].fill_(a.ctx)
            bb["logits"].copy_(logits0)

        graphs = {}
        for fp8 in (False, True):
            dec.enable_fp8_decode(fp8)
            reset()
            graphs[fp8] = dec.capture_batch_graph(nb, False)
            reset()
            timed(graphs[fp8].replay, a.warmup, 1)        # warm-up of the captured shape
        # output check: one replayed fp8 step == one eager fp8 step from the same state
        reset()
        graphs[True].replay()
        g_logits, g_tok = bb["logits"][:nb].clone(), bb["tok"][:nb].clone()
        reset()
        dec.enable_fp8_decode(True)
        dec._batched_step(nb, False)
        same_logits = bool(torch.equal(bb["logits"][:nb], g_logits))
        same_tok = bool(torch.equal(bb["tok"][:nb], g_tok))
        # alternate the two graphs round by round (the measuring guide: interleave A and B in one process)
        ts = {False: [], True: []}
        for _ in range(a.rounds):
            for fp8 in (False, True):
                reset()
                ts[fp8].append(timed(graphs[fp8].replay, 1, a.reps)["median_ms"])
        res = {}
        for fp8 in (False, True):
            t = sorted(ts[fp8])
            ms = t[len(t) // 2]
            w, kv = step_bytes(cfg, nb, a.ctx, fp8)
            res["fp8" if fp8 else "bf16"] = dict(ms_per_step=round(ms, 4), min_ms=round(t[0], 4), max_ms=round(t[-1], 4),
                                                 tokens_per_s=round(nb / (ms * 1e-3), 1), weight_GB=round(w / 1e9, 3), kv_GB=round(kv / 1e9, 3),
                                                 implied_TBps=round((w + kv) / (ms * 1e-3) / 1e12, 3))
        emit(rows, a.out, what="batched decode step (graph replay)", model="7B", nb=nb, ctx=a.ctx, rounds=a.rounds, **res,
             fp8_speedup=round(res["bf16"]["ms_per_step"] / res["fp8"]["ms_per_step"], 3), fp8_graph_logits_equal_eager=same_logits,
             fp8_graph_tokens_equal_eager=same_tok)
        dec._batch_graphs.clear()
    del dec, bb
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", default="2,4,8,16,32,64,80")
    ap.add_argument("--kernel-m", default="8,16,64")
    ap.add_argument("--ctx", type=int, default=1650)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="kernel,step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.nb = [int(n) for n in a.nb.split(",")]
    a.kernel_m = [int(n) for n in a.kernel_m.split(",")]
    assert torch.cuda.is_available(), "fp8_batch_bench.py measures on the GPU"
    rows = []
    only = a.only.split(",")
    if "kernel" in only:
        bench_kernel(rows, a)
    if "step" in only:
        bench_step(rows, a)


if __name__ == "__main__":
    with torch.no_grad():
        main()
