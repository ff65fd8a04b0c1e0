"""Batched decoding on VideoLLaMA2-8x7B's Mixtral decoder at full shape (D 4096, I 14336, 8 experts, top 2): the
graph-replayed batched step at 1 / 4 / 8 / 16 / 64 requests on a context of 945 rows per request, weights generated ON the device
(LazyRandomStateDict: its random router spreads the tokens almost evenly over the experts -- a real checkpoint's load is less even, so fewer
experts are active per step than here).  One JSON line per batch size:
  step_ms          the step as the decoder dispatches it (class attributes MOE_GEMM_BATCH / MOE_SKINNY_ROWS), every repeat and the median
  gemv_step_ms     the same step forced onto the per-token GEMVs (regime a), up to 16 requests
  skinny_step_ms   forced onto the grouped skinny-M GEMM (regime b)
  tiled_step_ms    forced onto the prefill's tiled grouped GEMM (MOE_SKINNY_ROWS = 0: the kernels the parent commit has for these rows)
  nb_x_solo_ms     nb times the solo decode_step's graph: the only way to serve nb requests without the batched step
  tokens_per_s, active_experts (last layer of the last step, read back AFTER the timing), bytes_per_step and tb_s implied by them.
The variants of one size are timed alternately inside every repeat; each window replays `--steps` steps from the same positions."""
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
    ap.add_argument("--layers", type=int, default=32, help="fewer layers: quicker runs (the JSON says so)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="1,4,8,16,64")
    ap.add_argument("--out", default=None)
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
    bb = dec._ensure_batch(max(sizes))
    dec.prefill_slot(0, x, bb["logits"][0])                       # one real context, copied into every slot
    for li in range(dec.n_layers):
        bb["k"][li][1:, :, :ctx] = bb["k"][li][0, :, :ctx]
        bb["v"][li][1:, :, :ctx] = bb["v"][li][0, :, :ctx]
    logits0 = torch.randn((max(sizes), dec.V), device=dev, generator=g)      # every slot draws its own first token
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

    dec.prefill(x)
    solo = dec.capture_graph()
    lines = []
    lw = dec.w["layers"][0]
    expert_bytes = (lw["wgu"][0].numel() + lw["wd"][0].numel()) * 2
    dense_bytes = (lw["wqkv"].numel() + lw["wo"].numel()) * 2 + lw["wr"].numel() * 4
    defaults = (HipMixtralDecoder.MOE_GEMM_BATCH, HipMixtralDecoder.MOE_SKINNY_ROWS)
    for nb in sizes:
        def reset():
            bb["pos"][:nb].fill_(ctx)
            bb["logits"][:nb].copy_(logits0[:nb])

        def solo_reset():
            dec.pos = ctx
            dec.state.copy_(torch.tensor([ctx - 1, 0], dtype=torch.int32))
            dec.logits.copy_(logits0[0])
        variants = dict(step_ms=defaults, gemv_step_ms=(65, 64), skinny_step_ms=(1, 64), tiled_step_ms=(1, 0))
        if nb > 16:
            del variants["gemv_step_ms"]
        graphs, routes = {}, {}
        for name, (gb, rows) in variants.items():
            dec.MOE_GEMM_BATCH, dec.MOE_SKINNY_ROWS = gb, rows
            reset()
            graphs[name] = dec.capture_batch_graph(nb, False, None, (name,))
            routes[name] = dec.last_route                         # (device tensors the graph of this variant writes)
        dec.MOE_GEMM_BATCH, dec.MOE_SKINNY_ROWS = defaults
        times = {name: [] for name in variants}
        solo_ms = []
        for _ in range(a.repeats):                                # alternate the variants inside every repeat
            for name in variants:
                times[name].append(window(graphs[name], reset))
            solo_ms.append(window(solo, solo_reset))
        window(graphs["step_ms"], reset)                          # the default step last: its routing is what is read back below
        active = int(routes["step_ms"]["ids"][:nb].cpu().unique().numel())
        regime = "a" if nb < defaults[0] else "b" if nb <= defaults[1] else "c"
        streams = nb * k if regime == "a" else active             # regime a: every (token, slot) pair streams its expert
        bytes_step = (dense_bytes + streams * expert_bytes) * a.layers + dec.w["lm_head"].numel() * 2
        med = statistics.median(times["step_ms"])
        res = dict(model="videollama2_8x7b", layers=a.layers, valid=a.layers == 32, ctx=ctx, nb=nb, regime=regime,
                   **{name: [round(t, 4) for t in ts] for name, ts in times.items()}, step_ms_median=round(med, 4),
                   solo_step_ms=[round(t, 4) for t in solo_ms], nb_x_solo_ms=round(nb * statistics.median(solo_ms), 4),
                   speedup_over_solo=round(nb * statistics.median(solo_ms) / med, 2), tokens_per_s=round(nb / med * 1e3, 1),
                   active_experts_last_layer=active, expert_streams_per_layer=streams, bytes_per_step=int(bytes_step),
                   tb_s=round(bytes_step / med / 1e9, 3))
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
