"""Decode on the MXFP4 weights against the fp8 and the 16-bit weights.  HIP events, warm-up + repeats (median, min, max):
  1. kernel: the 7B decode shapes and Qwen2's down projection at M = 1 (GEMV), 4 (multi-row GEMV), 8 / 16 / 64 (skinny-M GEMM + ordered reduce),
     the MXFP4, fp8 and 16-bit kernels timed one after the other in the same process: us per call and the weight-stream rate (MXFP4: nibble
     bytes + scale bytes; fp8: bytes + row scales; 16-bit: two bytes per weight);
  2. step: the 7B decoder at full width (weights generated on the device from a seed), every request with the same --ctx-row prompt in its
     cache, nb requests (1 = the single-sequence step, more = the batched step): the graph-replayed step on the 16-bit weights, the fp8 copies
     and the MXFP4 copies, captured once each and alternated round by round in one process.  Per point: ms per step, tokens per second, bytes
     per step from the shapes and the implied TB/s.  Output check: the replayed MXFP4 step gives the logits of an eager MXFP4 step, bit for bit.
Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FORMATS = ("16bit", "fp8", "mxfp4")


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


SHAPES = [("qkv", 6144, 4096, dict(rms=True)), ("o", 4096, 4096, dict(res=True)), ("gate_up", 28672, 4096, dict(rms=True, swiglu=True)),
          ("down", 4096, 14336, dict(res=True)), ("qwen2_down", 3584, 18944, dict(res=True))]


def bench_kernel(rows, a):
    from videollama2_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, N, K, kw in SHAPES:
        w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16()
        q8, s8 = ops.quant_fp8(w)
        q4, s4 = ops.quant_mxfp4(w)
        ones = torch.ones(K, device="cuda")
        n_out = N // 2 if kw.get("swiglu") else N
        nbytes = {"16bit": 2 * N * K, "fp8": N * K + 4 * N, "mxfp4": N * K // 2 + N * K // 32}
        for M in a.kernel_m:
            x = torch.randn(M, K, device="cuda", generator=g).bfloat16()
            res = torch.randn(M, n_out, device="cuda", generator=g).bfloat16() if kw.get("res") else None
            kk = dict(swiglu=bool(kw.get("swiglu")), res=res)
            if M == 1:
                x, kk["res"] = x[0], None if res is None else res[0]
            if M <= 4:                                  # GEMV forms: the RMSNorm rides in the kernel as in the decode step
                n16 = dict(norm_w=ones, eps=1e-5) if kw.get("rms") else {}
                nq = dict(rms_plain=True, eps=1e-5) if kw.get("rms") else {}
                f16, f8, f4 = (ops.gemv, ops.gemv_fp8, ops.gemv_mxfp4) if M == 1 else (ops.gemv_batched, ops.gemv_batched_fp8, ops.gemv_batched_mxfp4)
                y = f16(w, x, **n16, **kk)
                calls = {"16bit": lambda: f16(w, x, out=y, **n16, **kk), "fp8": lambda: f8(q8, s8, x, out=y, **nq, **kk),
                         "mxfp4": lambda: f4(q4, s4, x, out=y, **nq, **kk)}
                what = "GEMV" if M == 1 else "multi-row GEMV"
            else:
                y = ops.gemm_skinny(x, w, **kk)
                calls = {"16bit": lambda: ops.gemm_skinny(x, w, out=y, **kk), "fp8": lambda: ops.gemm_skinny_fp8(x, q8, s8, out=y, **kk),
                         "mxfp4": lambda: ops.gemm_skinny_mxfp4(x, q4, s4, out=y, **kk)}
                what = "skinny-M GEMM (+ reduce)"
            r = dict(what=what, shape=name, N=N, K=K, M=M)
            for fmt in FORMATS:
                t = timed(calls[fmt], a.warmup, a.reps, inner=20)
                r[fmt + "_us"] = round(t["median_ms"] * 1e3, 2)
                r[fmt + "_min_max_us"] = [round(t["min_ms"] * 1e3, 2), round(t["max_ms"] * 1e3, 2)]
                r[fmt + "_weight_TBps"] = round(nbytes[fmt] / (t["median_ms"] * 1e-3) / 1e12, 3)
            emit(rows, a.out, **r)
        del w, q8, s8, q4, s4
        torch.cuda.empty_cache()


def step_bytes(cfg, nb, ctx, fmt):
    """Bytes one step moves, from the shapes: the projections (16-bit: two bytes per weight; fp8: one + a 4-byte scale per row; MXFP4: half a
    byte + one scale byte per 32; the quantised ones streamed once per call of at most 64 rows), lm_head (fp8 in the fp8 step, else 16-bit) and
    every request's K and V rows up to its position."""
    l = cfg["llm"]
    D, I, V, L, hd = l["hidden_size"], l["intermediate_size"], l["vocab_size"], l["num_hidden_layers"], l["head_dim"]
    nh, nkv = l["num_attention_heads"], l["num_key_value_heads"]
    mats = [((nh + 2 * nkv) * hd, D), (D, nh * hd), (2 * I, D), (D, I)]
    n_w, n_rows = L * sum(N * K for N, K in mats), L * sum(N for N, _ in mats)
    calls = math.ceil(nb / 64)
    if fmt == "16bit":
        w = 2 * (n_w + V * D)
    elif fmt == "fp8":
        w = (n_w + V * D + 4 * (n_rows + V)) * calls
    else:
        w = (n_w // 2 + n_w // 32) * calls + 2 * V * D
    kv = nb * L * 2 * nkv * (ctx + 1) * hd * 2
    return w, kv


def set_format(dec, fmt):
    dec.enable_fp8_decode(False)
    dec.enable_mxfp4_decode(False)
    if fmt == "fp8":
        dec.enable_fp8_decode()
    elif fmt == "mxfp4":
        dec.enable_mxfp4_decode()


def bench_step(rows, a):
    from videollama2_amd import ops
    from videollama2_amd.config import videollama2_7b
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.weights import LazyRandomStateDict
    cfg = videollama2_7b()
    sd = LazyRandomStateDict(cfg, "cuda", seed=1234)
    dec = HipMistralDecoder(cfg, sd, "cuda", max_seq_len=a.ctx + 256)
    del sd
    torch.cuda.empty_cache()
    D = cfg["llm"]["hidden_size"]
    x = (0.5 * torch.randn(a.ctx, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))).bfloat16()
    for nb in a.nb:
        if nb == 1:                                       # the single-sequence step: the decoder's own cache, position on the device
            logits0 = dec.prefill(x).clone()

            def reset():
                dec.pos = a.ctx
                dec.state.copy_(torch.tensor([a.ctx - 1, 0], dtype=torch.int32))
                dec.logits.copy_(logits0)

            def eager():
                ops.argmax(dec.logits, dec.tok, dec.hist, 0)
                dec._decode_kernels(dyn=False)
            capture, out = dec.capture_graph, lambda: dec.logits
        else:
            bb = dec._ensure_batch(nb)
            for b in range(nb):                           # the same prompt in every slot's cache
                dec.prefill(x, cache=([k[b] for k in bb["k"]], [v[b] for v in bb["v"]]), logits_out=bb["logits"][b])
            logits0 = bb["logits"].clone()

            def reset():
                bb["pos"][:nb].fill_(a.ctx)
                bb["logits"].copy_(logits0)

            eager = lambda: dec._batched_step(nb, False)
            capture, out = lambda: dec.capture_batch_graph(nb, False), lambda: bb["logits"][:nb]
        graphs = {}
        for fmt in FORMATS:                               # a toggle drops the decoder's handle on a captured graph; this dict keeps it alive
            set_format(dec, fmt)
            reset()
            graphs[fmt] = capture()
            reset()
            timed(graphs[fmt].replay, a.warmup, 1)
        # output check: one replayed MXFP4 step == one eager MXFP4 step from the same state (the decoder is on MXFP4 here)
        reset()
        graphs["mxfp4"].replay()
        g_logits = out().clone()
        reset()
        eager()
        same_logits = bool(torch.equal(out(), g_logits))
        # alternate the graphs round by round (interleave the candidates in one process)
        ts = {fmt: [] for fmt in FORMATS}
        for _ in range(a.rounds):
            for fmt in FORMATS:
                reset()
                ts[fmt].append(timed(graphs[fmt].replay, 1, a.reps)["median_ms"])
        res = {}
        for fmt in FORMATS:
            t = sorted(ts[fmt])
            ms = t[len(t) // 2]
            w, kv = step_bytes(cfg, nb, a.ctx, fmt)
            res[fmt] = dict(ms_per_step=round(ms, 4), min_ms=round(t[0], 4), max_ms=round(t[-1], 4), tokens_per_s=round(nb / (ms * 1e-3), 1),
                            weight_GB=round(w / 1e9, 3), kv_GB=round(kv / 1e9, 3), implied_TBps=round((w + kv) / (ms * 1e-3) / 1e12, 3))
        emit(rows, a.out, what="decode step (graph replay)", model="7B", nb=nb, ctx=a.ctx, rounds=a.rounds, **res,
             mxfp4_speedup_vs_fp8=round(res["fp8"]["ms_per_step"] / res["mxfp4"]["ms_per_step"], 3),
             mxfp4_speedup_vs_16bit=round(res["16bit"]["ms_per_step"] / res["mxfp4"]["ms_per_step"], 3), mxfp4_graph_logits_equal_eager=same_logits)
        graphs.clear()
        set_format(dec, "16bit")
    del dec
    torch.cuda.empty_cache()


def profile_step(a):
    """The single-request MXFP4 step replayed --profile-steps times, for a kernel trace of its own (run under the profiler, program after --)."""
    from videollama2_amd.config import videollama2_7b
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.weights import LazyRandomStateDict
    cfg = videollama2_7b()
    dec = HipMistralDecoder(cfg, LazyRandomStateDict(cfg, "cuda", seed=1234), "cuda", max_seq_len=a.ctx + 256)
    dec.enable_mxfp4_decode()
    x = (0.5 * torch.randn(a.ctx, cfg["llm"]["hidden_size"], device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))).bfloat16()
    dec.generate(x, max_new_tokens=a.profile_steps, use_graph=True)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", default="1,4,8,64")
    ap.add_argument("--kernel-m", default="1,4,8,16,64")
    ap.add_argument("--ctx", type=int, default=1650)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="kernel,step")
    ap.add_argument("--profile-steps", type=int, default=0, help="replay the single-request MXFP4 step this many times and exit (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.nb = [int(n) for n in a.nb.split(",")]
    a.kernel_m = [int(n) for n in a.kernel_m.split(",")]
    assert torch.cuda.is_available(), "mxfp4_bench.py measures on the GPU"
    if a.profile_steps:
        return profile_step(a)
    rows = []
    only = a.only.split(",")
    if "kernel" in only:
        bench_kernel(rows, a)
    if "step" in only:
        bench_step(rows, a)


if __name__ == "__main__":
    with torch.no_grad():
        main()
