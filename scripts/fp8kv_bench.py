"""The batched decode step on the fp8 KV cache against the 16-bit KV cache.  The 7B decoder at full width (weights
generated on the device from a seed), every slot holding the same --ctx-row prompt, nb requests: the graph-replayed batched step on the
16-bit slots and on the fp8 slots, captured once each and alternated round by round in one process (HIP events; median, min, max over the
rounds), once on the 16-bit decode weights and once on the fp8 copies.  Per point: ms per step for both graphs, bytes per step from the shapes
(weights + K/V rows + row scales) and the implied TB/s, and the slots' memory in both formats.  Output check: the replayed fp8-KV step gives
the logits (bit for bit) and next tokens of an eager fp8-KV step from the same state.
--only trace: nothing is timed; a few replays of both graphs at --trace-nb requests on the fp8 weights, for a kernel trace
(rocprofv3 --kernel-trace --stats -- python scripts/fp8kv_bench.py --only trace): attn_decode_kernel<false> against attn_decode_kv8_kernel.
Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.fp8_batch_bench import emit, step_bytes, timed      # noqa: E402  (the weights' bytes and the timing loop are that script's)


def kv_bytes(cfg, nb, rows, kv8):
    """Bytes of nb sequences' K and V rows [0, rows) over all layers: 16-bit elements, or one code byte per element + a 4-byte scale per row."""
    l = cfg["llm"]
    per_row = l["head_dim"] + 4 if kv8 else 2 * l["head_dim"]
    return nb * l["num_hidden_layers"] * 2 * l["num_key_value_heads"] * rows * per_row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", default="1,4,8,16,32,64")
    ap.add_argument("--ctx", type=int, default=1650)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="step")
    ap.add_argument("--trace-nb", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.nb = [int(n) for n in a.nb.split(",")]
    trace = a.only == "trace"
    if trace:
        a.nb = [a.trace_nb]
    assert torch.cuda.is_available(), "fp8kv_bench.py measures on the GPU"
    from videollama2_amd.config import videollama2_7b
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.weights import LazyRandomStateDict
    cfg = videollama2_7b()
    dec = HipMistralDecoder(cfg, LazyRandomStateDict(cfg, "cuda", seed=1234), "cuda", max_seq_len=a.ctx + 256)
    torch.cuda.empty_cache()
    dec.enable_fp8_decode()
    dec.enable_fp8_decode(False)
    nmax, smax = max(a.nb), dec.max_seq_len
    x = (0.5 * torch.randn(a.ctx, cfg["llm"]["hidden_size"], device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))).bfloat16()
    # both sets of slots stay alive side by side; the same prompt in every slot (prefilled once, then copied)
    bbs = {}
    for kv8 in (False, True):
        dec.enable_fp8_kv(kv8)
        bb = bbs[kv8] = dec._ensure_batch(nmax)
        dec.prefill_slot(0, x, bb["logits"][0])
        for t in ([t for kv in bb["kv8"] for t in kv] if kv8 else bb["k"] + bb["v"]):
            t[1:].copy_(t[0:1].expand_as(t[1:]))
        bb["logits"][1:].copy_(bb["logits"][0:1].expand_as(bb["logits"][1:]))
    assert torch.equal(bbs[True]["logits"], bbs[False]["logits"])             # the prefill does not depend on the cache format
    logits0 = bbs[False]["logits"].clone()

    def select(kv8):
        dec.enable_fp8_kv(kv8)             # (drops the captured graphs and the slot buffers of the other format ...)
        dec._bb = bbs[kv8]                 # ... which this script keeps: both graphs replay on their own buffers

    rows = []
    for w8 in ((True,) if trace else (False, True)):
        dec.enable_fp8_decode(w8)
        for nb in a.nb:
            def reset(kv8):
                bbs[kv8]["pos"][:nb].fill_(a.ctx)
                bbs[kv8]["logits"].copy_(logits0)

            graphs = {}
            for kv8 in (False, True):
                select(kv8)
                reset(kv8)
                graphs[kv8] = dec.capture_batch_graph(nb, False)
                reset(kv8)
                timed(graphs[kv8].replay, a.warmup, 1)
            if trace:
                for _ in range(5):
                    for kv8 in (False, True):
                        reset(kv8)
                        graphs[kv8].replay()
                torch.cuda.synchronize()
                print(json.dumps(dict(what="trace run", nb=nb, ctx=a.ctx, replays_each=5 + a.warmup + 1)), flush=True)
                continue
            bb8 = bbs[True]
            reset(True)
            graphs[True].replay()
            g_logits, g_tok = bb8["logits"][:nb].clone(), bb8["tok"][:nb].clone()
            reset(True)
            dec._batched_step(nb, False)                                          # fp8 KV is the selected format here
            same_logits, same_tok = bool(torch.equal(bb8["logits"][:nb], g_logits)), bool(torch.equal(bb8["tok"][:nb], g_tok))
            ts = {False: [], True: []}
            for _ in range(a.rounds):
                for kv8 in (False, True):
                    reset(kv8)
                    ts[kv8].append(timed(graphs[kv8].replay, 1, a.reps)["median_ms"])
            res = {}
            wbytes, _ = step_bytes(cfg, nb, a.ctx, w8)
            for kv8 in (False, True):
                t = sorted(ts[kv8])
                ms = t[len(t) // 2]
                kvb = kv_bytes(cfg, nb, a.ctx + 1, kv8)
                res["kv_fp8" if kv8 else "kv_16bit"] = dict(
                    ms_per_step=round(ms, 4), min_ms=round(t[0], 4), max_ms=round(t[-1], 4), weight_GB=round(wbytes / 1e9, 3),
                    kv_GB=round(kvb / 1e9, 3), implied_TBps=round((wbytes + kvb) / (ms * 1e-3) / 1e12, 3),
                    slot_memory_GB=round(kv_bytes(cfg, nb, smax, kv8) / 1e9, 3))
            emit(rows, a.out, what="batched decode step (graph replay), fp8 KV cache against 16-bit KV cache", model="7B",
                 weights="fp8" if w8 else "16bit", nb=nb, ctx=a.ctx, max_seq_len=smax, rounds=a.rounds, reps=a.reps, **res,
                 fp8kv_speedup=round(res["kv_16bit"]["ms_per_step"] / res["kv_fp8"]["ms_per_step"], 3),
                 fp8kv_graph_logits_equal_eager=same_logits, fp8kv_graph_tokens_equal_eager=same_tok)


if __name__ == "__main__":
    with torch.no_grad():
        main()
