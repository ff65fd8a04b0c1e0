"""VideoLLaMA2-8x7B's Mixtral decoder at full shape (D 4096, I 14336, 32 layers, 8 experts, top 2): prefill of S = 945 tokens (8 frames
+ the bench prompt) and the graph-replayed decode step, weights generated ON the device layer by layer (no 93 GB host copy).  Prints one
JSON line: prefill ms, decode ms/token, bytes streamed per token and the TB/s they imply, the grouped gate/up time of one layer against
the library's dense gate/up of the same FLOPs (M = S*k, N = 2I, K = D), and the prefill's MFMA-FLOP rate.  For kernel times, run it under
`rocprofv3 --kernel-trace --stats -- python scripts/moe_bench.py` and keep the stats under profiles/."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", type=int, default=945)
    ap.add_argument("--layers", type=int, default=32, help="fewer layers: profiling runs only (the JSON says so)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from videollama2_amd import ops
    from videollama2_amd.config import videollama2_8x7b
    from videollama2_amd.decoder import HipMixtralDecoder
    dev = "cuda"
    cfg = videollama2_8x7b(8)
    l = cfg["llm"]
    D, I, E, k, S = l["hidden_size"], l["intermediate_size"], l["num_local_experts"], l["num_experts_per_tok"], a.seq
    from videollama2_amd.weights import LazyRandomStateDict
    # every tensor generated on the device when packed, from a sha256-of-its-name seed: the same weights (and expert load) in every run
    sd = LazyRandomStateDict(cfg, dev, seed=1234, n_llm_layers=a.layers)
    dec = HipMixtralDecoder(cfg, sd, dev, max_seq_len=S + a.steps + 8, n_layers=a.layers)
    torch.cuda.synchronize()
    x = (0.5 * torch.randn(S, D, device=dev)).bfloat16()
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    prefill_ms = timed(lambda: dec.prefill(x), 3)
    dec.prefill(x)
    g = dec.capture_graph()
    dec.state.copy_(torch.tensor([dec.pos - 1, 0], dtype=torch.int32))
    e0, e1 = ev(), ev()
    e0.record()
    for _ in range(a.steps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    decode_ms = e0.elapsed_time(e1) / a.steps
    # bytes per token: attention + router + k experts of every layer, lm_head, embedding row (KV reads are small at this context)
    lw = dec.w["layers"][0]
    per_layer = (lw["wqkv"].numel() + lw["wo"].numel() + k * (lw["wgu"][0].numel() + lw["wd"][0].numel())) * 2 + lw["wr"].numel() * 4
    bytes_tok = per_layer * a.layers + dec.w["lm_head"].numel() * 2
    # grouped gate/up of layer 0 at S tokens against the dense gate/up with the same FLOPs (M = S*k, N = 2I, K = D)
    r = ops.moe_route(x, lw["wr"], k, dec.eps)
    grouped_ms = timed(lambda: ops.moe_gemm(r["xg"], lw["wgu"], r, S, k, swiglu=True, row_norm=r["rn"], eps=dec.eps), 10)
    xa = (0.5 * torch.randn(S * k, D, device=dev)).bfloat16()
    rn = ops.row_norm_finalize(ops.row_stats(xa), D, ops.NORM_RMS, dec.eps)
    dense_ms = timed(lambda: ops.gemm(xa, lw["wgu"][0], swiglu=True, norm=(ops.NORM_RMS, rn, dec.eps, None), mfma16=True), 10)
    # MFMA FLOPs of the prefill: projections + expert GEMMs + attention (causal half)
    nh, hd = l["num_attention_heads"], l["head_dim"]
    proj = 2 * S * (lw["wqkv"].shape[0] + lw["wo"].shape[0]) * D + 2 * S * k * (2 * I * D + D * I)
    attn = 2 * 2 * nh * hd * S * S / 2
    flops = (proj + attn) * a.layers
    res = dict(model="videollama2_8x7b", layers=a.layers, valid=a.layers == 32, S=S, prefill_ms=round(prefill_ms, 3),
               decode_ms_per_token=round(decode_ms, 4), bytes_per_token=int(bytes_tok), decode_tb_s=round(bytes_tok / decode_ms / 1e9, 3),
               prefill_tflops=round(flops / prefill_ms / 1e9, 1), prefill_mfma_fraction_of_2_5pf=round(flops / prefill_ms / 1e9 / 2500, 3),
               gate_up_grouped_us=round(grouped_ms * 1e3, 1), gate_up_dense_same_flops_us=round(dense_ms * 1e3, 1),
               grouped_over_dense=round(grouped_ms / dense_ms, 3))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
