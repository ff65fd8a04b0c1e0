"""The tiled W4A16 grouped GEMM on VideoLLaMA2-8x7B's Mixtral decoder at full shape (D 4096, I 14336, 8 experts, top 2):
the graph-replayed batched decode step at 5 .. 128 requests on a context of 945 rows per request, scripts/moe_fp8_tiled_bench.py's method (8 of
the 32 layers by default, weights generated ON the device by LazyRandomStateDict, median of `--repeats` windows of `--steps` steps, the variants
alternating inside every repeat).  One JSON line per size:
  bf16_step_ms     (a) the 16-bit default step (both switches off: the tiled 16-bit grouped GEMM), every repeat
  bf16_again_ms    (a) timed a second time inside every repeat: |median - median| is the spread a difference has to clear TWICE to count
  fp8_step_ms      (b) enable_moe_fp8(tiled=True): the tiled W8A16 grouped GEMM from MOE_FP8_TILED_FROM on
  skinny_step_ms   (c) enable_moe_mxfp4(): the MXFP4 grouped skinny-M GEMM, up to 64 requests (null beyond: refused)
  tiled_step_ms    (d) enable_moe_mxfp4(tiled=True) with MOE_MXFP4_TILED_FROM = 5 on the instance: the tiled W4A16 grouped GEMM
  tiled_vs_skinny / tiled_vs_bf16 / tiled_vs_fp8   "wins" / "ties" / "loses": the difference of the medians against twice the spread
  tiled_weight_TBps / fp8_weight_TBps / bf16_weight_TBps   implied expert-weight bytes per second: layers x active experts x expert bytes
                   (4.25 bits per weight for MXFP4) / step time
(a), (b) and (c) are the parent commit's code paths, timed in the same run; (d) is never compared against itself."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, default=945)
    ap.add_argument("--layers", type=int, default=8, help="layers of the 32 built (the JSON says so)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="5,6,8,12,16,24,32,48,64,96,128")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r25_moe_mxfp4_tiled_bench.jsonl"))
    a = ap.parse_args()
    from videollama2_amd.config import videollama2_8x7b
    from videollama2_amd.decoder import HipMixtralDecoder
    from videollama2_amd.weights import LazyRandomStateDict
    dev = "cuda"
    cfg = videollama2_8x7b(8)
    D, ctx = cfg["llm"]["hidden_size"], a.ctx
    sizes = [int(s) for s in a.sizes.split(",")]
    sd = LazyRandomStateDict(cfg, dev, seed=1234, n_llm_layers=a.layers)
    dec = HipMixtralDecoder(cfg, sd, dev, max_seq_len=ctx + a.steps + 8, n_layers=a.layers).enable_moe_batch()
    dec.MOE_MXFP4_TILED_FROM = dec.MOE_GEMM_BATCH                 # (d) runs the tiled form at every grouped size
    torch.cuda.synchronize()
    g = torch.Generator(device=dev).manual_seed(7)
    x = (0.5 * torch.randn(ctx, D, device=dev, generator=g)).bfloat16()
    bb = dec._ensure_batch(max(max(sizes), 2))
    dec.prefill_slot(0, x, bb["logits"][0])                       # one real context, copied into every slot
    for li in range(dec.n_layers):
        bb["k"][li][1:, :, :ctx] = bb["k"][li][0, :, :ctx]
        bb["v"][li][1:, :, :ctx] = bb["v"][li][0, :, :ctx]
    logits0 = torch.randn((bb["B"], dec.V), device=dev, generator=g)         # every slot draws its own first token
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def window(graph, reset):
        reset()
        graph.replay()                                            # warm
        reset()
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(a.steps):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    def select(fmt, tiled):
        """Both switches off, then the one asked for (they refuse each other)."""
        dec.enable_moe_fp8(False)
        dec.enable_moe_mxfp4(False)
        if fmt == "fp8":
            dec.enable_moe_fp8(tiled=tiled)
        elif fmt == "mxfp4":
            dec.enable_moe_mxfp4(tiled=tiled)

    lw = dec.w["layers"][0]
    expert_elems = lw["wgu"][0].numel() + lw["wd"][0].numel()
    lines = []
    for nb in sizes:
        def reset():
            bb["pos"][:nb].fill_(ctx)
            bb["logits"][:nb].copy_(logits0[:nb])
        variants = [("bf16_step_ms", (None, False)), ("fp8_step_ms", ("fp8", True))] + \
                   ([("skinny_step_ms", ("mxfp4", False))] if nb <= dec.MOE_MXFP4_ROWS else []) + [("tiled_step_ms", ("mxfp4", True))]
        graphs, routes = {}, {}
        for name, sel in variants:
            select(*sel)                                          # (drops the decoder's graph table; the graphs held here stay valid)
            reset()
            graphs[name] = dec.capture_batch_graph(nb, False, None, (name,))
            routes[name] = dec.last_route["ids"]
        select(None, False)
        order = [(name, name) for name, _ in variants] + [("bf16_again_ms", "bf16_step_ms")]
        times = {name: [] for name, _ in order}
        for _ in range(a.repeats):                                # alternate the variants inside every repeat
            for name, gname in order:
                times[name].append(window(graphs[gname], reset))
        window(graphs["tiled_step_ms"], reset)                    # the tiled step last: its routing is what is read back below
        active = int(routes["tiled_step_ms"][:nb].cpu().unique().numel())
        med = {name: statistics.median(ts) for name, ts in times.items()}
        spread = abs(med["bf16_step_ms"] - med["bf16_again_ms"])

        def verdict(ref):
            if ref not in med:
                return None
            d = med[ref] - med["tiled_step_ms"]
            return "ties" if abs(d) <= 2 * spread else "wins" if d > 0 else "loses"
        tbps = lambda ms, bytes_per_elem: round(a.layers * active * expert_elems * bytes_per_elem / (ms * 1e-3) / 1e12, 3)
        res = dict(model="videollama2_8x7b", layers=a.layers, valid=a.layers == 32, ctx=ctx, nb=nb,
                   **{name: [round(t, 4) for t in ts] for name, ts in times.items()},
                   bf16_median_ms=round(med["bf16_step_ms"], 4), bf16_again_median_ms=round(med["bf16_again_ms"], 4),
                   fp8_median_ms=round(med["fp8_step_ms"], 4),
                   skinny_median_ms=round(med["skinny_step_ms"], 4) if "skinny_step_ms" in med else None,
                   tiled_median_ms=round(med["tiled_step_ms"], 4), spread_ms=round(spread, 4),
                   tiled_vs_skinny=verdict("skinny_step_ms"), tiled_vs_bf16=verdict("bf16_step_ms"), tiled_vs_fp8=verdict("fp8_step_ms"),
                   active_experts_last_layer=active, expert_bytes_per_layer_bf16=int(active * expert_elems * 2),
                   expert_bytes_per_layer_fp8=int(active * expert_elems), expert_bytes_per_layer_mxfp4=int(active * expert_elems * 4.25 / 8),
                   bf16_weight_TBps=tbps(med["bf16_step_ms"], 2), fp8_weight_TBps=tbps(med["fp8_step_ms"], 1),
                   tiled_weight_TBps=tbps(med["tiled_step_ms"], 4.25 / 8))
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        if a.out:
            with open(a.out, "w") as fh:                          # rewritten after every size: a run cut short keeps what it measured
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
