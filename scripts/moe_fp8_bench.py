"""fp8 expert weights on VideoLLaMA2-8x7B's Mixtral decoder at full shape (D 4096, I 14336, 8 experts, top 2): the
graph-replayed decode step at 1 / 2 / 4 / 5 / 8 / 16 / 64 requests on a context of 945 rows per request with enable_moe_fp8 off (the
decoder's default 16-bit regimes: the parent commit's step) and on, weights generated ON the device (LazyRandomStateDict: its random router
spreads the tokens almost evenly over the experts).  8 of the 32 layers by default (the JSON says so).  One JSON line per size:
  bf16_step_ms     the 16-bit step as the decoder dispatches it, every repeat
  bf16_again_ms    the same graph timed a second time inside every repeat: the run-to-run spread the comparison has to clear
  fp8_step_ms      the step with the switch on (rows kernels below MOE_GEMM_BATCH, the grouped skinny-M GEMM from there to 64)
  speedup          median bf16_step_ms / median fp8_step_ms (below 1: fp8 loses at that size), spread = the relative spread of the 16-bit medians
  active_experts of the last layer (read back AFTER the timing) and the expert bytes per layer each step streams.
nb = 1 is the solo decode_step's graph, the others the batched step's.  The variants are timed alternately inside every repeat; each window
replays `--steps` steps from the same positions."""
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
    ap.add_argument("--sizes", default="1,2,4,5,8,16,64")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r22_moe_fp8_bench.jsonl"))
    a = ap.parse_args()
    from videollama2_amd.config import videollama2_8x7b
    from videollama2_amd.decoder import HipMixtralDecoder
    from videollama2_amd.weights import LazyRandomStateDict
    dev = "cuda"
    cfg = videollama2_8x7b(8)
    l = cfg["llm"]
    D, k, ctx = l["hidden_size"], l["num_experts_per_tok"], a.ctx
    sizes = [int(s) for s in a.sizes.split(",")]
    sd = LazyRandomStateDict(cfg, dev, seed=1234, n_llm_layers=a.layers)
    dec = HipMixtralDecoder(cfg, sd, dev, max_seq_len=ctx + a.steps + 8, n_layers=a.layers).enable_moe_batch()
    torch.cuda.synchronize()
    g = torch.Generator(device=dev).manual_seed(7)
    x = (0.5 * torch.randn(ctx, D, device=dev, generator=g)).bfloat16()
    bb = dec._ensure_batch(max(max(sizes), 2))
    dec.prefill_slot(0, x, bb["logits"][0])                       # one real context, copied into every slot
    for li in range(dec.n_layers):
        bb["k"][li][1:, :, :ctx] = bb["k"][li][0, :, :ctx]
        bb["v"][li][1:, :, :ctx] = bb["v"][li][0, :, :ctx]
    logits0 = torch.randn((bb["B"], dec.V), device=dev, generator=g)         # every slot draws its own first token
    dec.prefill(x)
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

    lw = dec.w["layers"][0]
    expert_elems = lw["wgu"][0].numel() + lw["wd"][0].numel()
    lines = []
    for nb in sizes:
        if nb == 1:
            def reset():
                dec.pos = ctx
                dec.state.copy_(torch.tensor([ctx - 1, 0], dtype=torch.int32))
                dec.logits.copy_(logits0[0])
        else:
            def reset():
                bb["pos"][:nb].fill_(ctx)
                bb["logits"][:nb].copy_(logits0[:nb])
        graphs, routes = {}, {}
        for name, on in (("bf16_step_ms", False), ("fp8_step_ms", True)):
            dec.enable_moe_fp8(on)                                # (drops the decoder's graph table; the graphs held here stay valid)
            reset()
            graphs[name] = dec.capture_graph() if nb == 1 else dec.capture_batch_graph(nb, False, None, (name,))
            routes[name] = dec.moe_ids if nb == 1 else dec.last_route["ids"]
        dec.enable_moe_fp8(False)
        order = (("bf16_step_ms", "bf16_step_ms"), ("fp8_step_ms", "fp8_step_ms"), ("bf16_again_ms", "bf16_step_ms"))
        times = {name: [] for name, _ in order}
        for _ in range(a.repeats):                                # alternate the variants inside every repeat
            for name, gname in order:
                times[name].append(window(graphs[gname], reset))
        window(graphs["fp8_step_ms"], reset)                      # the fp8 step last: its routing is what is read back below
        ids = routes["fp8_step_ms"] if nb == 1 else routes["fp8_step_ms"][:nb]        # (nb = 1: the solo step's k ids)
        active = int(ids.cpu().unique().numel())
        grouped = nb >= HipMixtralDecoder.MOE_GEMM_BATCH
        streams = active if grouped else nb * k                   # below MOE_GEMM_BATCH every (token, slot) pair streams its expert
        med = {name: statistics.median(ts) for name, ts in times.items()}
        res = dict(model="videollama2_8x7b", layers=a.layers, valid=a.layers == 32, ctx=ctx, nb=nb,
                   form="solo" if nb == 1 else "grouped_skinny" if grouped else "rows",
                   **{name: [round(t, 4) for t in ts] for name, ts in times.items()},
                   bf16_median_ms=round(med["bf16_step_ms"], 4), fp8_median_ms=round(med["fp8_step_ms"], 4),
                   speedup=round(med["bf16_step_ms"] / med["fp8_step_ms"], 3),
                   spread=round(abs(med["bf16_step_ms"] - med["bf16_again_ms"]) / med["bf16_step_ms"], 4),
                   tokens_per_s_bf16=round(nb / med["bf16_step_ms"] * 1e3, 1), tokens_per_s_fp8=round(nb / med["fp8_step_ms"] * 1e3, 1),
                   active_experts_last_layer=active, expert_streams_per_layer=streams,
                   expert_bytes_per_layer_bf16=int(streams * expert_elems * 2), expert_bytes_per_layer_fp8=int(streams * expert_elems))
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
