"""The batched decode step over a SHARED prompt prefix against the plain batched step.  The 7B decoder at full width
(weights generated on the device from a seed); every request's prompt is the same --prefix rows followed by --own rows of its own (total
1650 = the section 16 table's context).  Plain: every slot holds a full private copy of all rows.  Shared: the prefix rows are held once (the
decoder's single-sequence cache), every request holds its own rows only.  Both steps are captured once per nb and replayed alternately,
round by round, in one process (HIP events; median, min, max over the rounds), on the 16-bit decode weights and on the fp8 copies.  Per
point: ms per step of each mode, K/V bytes per step of each mode from the shapes, the slot memory of each mode, and the prompt phase:
`prefill(all rows) x nb` against `prefill(prefix) + extend(own rows) x nb` (the encoder is not run by this script: it runs nb times in the
plain path and once in the shared one).  Output check: the shared step's first-step logits against the plain step's (rel-L2, and the tokens).
Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.fp8_batch_bench import emit, step_bytes, timed      # noqa: E402  (the weights' bytes and the timing loop are that script's)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", default="1,4,16,64")
    ap.add_argument("--prefix", type=int, default=1621)
    ap.add_argument("--own", type=int, default=29)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.nb = [int(n) for n in a.nb.split(",")]
    assert torch.cuda.is_available(), "shared_prefix_bench.py measures on the GPU"
    from videollama2_amd import ops
    from videollama2_amd.config import videollama2_7b
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.weights import LazyRandomStateDict
    cfg = videollama2_7b()
    l = cfg["llm"]
    P, ctx = a.prefix, a.prefix + a.own
    dec = HipMistralDecoder(cfg, LazyRandomStateDict(cfg, "cuda", seed=1234), "cuda", max_seq_len=ctx + 256)
    torch.cuda.empty_cache()
    dec.enable_fp8_decode()
    dec.enable_fp8_decode(False)
    nmax, smax = max(a.nb), dec.max_seq_len
    x = (0.5 * torch.randn(ctx, l["hidden_size"], device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))).bfloat16()
    own_cap = ops.shared_own_cap(a.own, 64 - a.own)                # room for every replay of a timed set
    row_bytes = l["num_hidden_layers"] * 2 * l["num_key_value_heads"] * l["head_dim"] * 2       # K and V of one position, all layers
    rows = []
    # ---- the prompt phase
    t_full = timed(lambda: dec.prefill(x), 1, 3)["median_ms"]
    t_pre = timed(lambda: dec.prefill(x[:P]), 1, 3)["median_ms"]
    t_ext = timed(lambda: dec.extend(x[P:], start_pos=P), 1, 3)["median_ms"]
    for nb in a.nb:
        emit(rows, a.out, what="prompt phase of nb requests over one prefix (decoder only; the encoder runs nb times against once)", model="7B",
             nb=nb, prefix=P, own=a.own, prefill_all_rows_ms=t_full, prefill_prefix_ms=t_pre, extend_own_rows_ms=t_ext,
             plain_ms=round(t_full * nb, 2), shared_ms=round(t_pre + t_ext * nb, 2))
    # ---- the slots of both modes, every request the same prompt
    bb = dec._ensure_batch(nmax)
    dec.prefill_slot(0, x, bb["logits"][0])
    for t in bb["k"] + bb["v"]:
        t[1:].copy_(t[0:1].expand_as(t[1:]))
    bb["logits"][1:].copy_(bb["logits"][0:1].expand_as(bb["logits"][1:]))
    sp = dec._ensure_shared(nmax, P, own_cap)
    dec.prefill(x[:P])
    dec.extend(x[P:], start_pos=P, logits_out=sp["logits"][0])
    for li in range(dec.n_layers):
        sp["k"][li][:, :, :a.own].copy_(dec.kcache[li][:, P:ctx])
        sp["v"][li][:, :, :a.own].copy_(dec.vcache[li][:, P:ctx])
    sp["logits"][1:].copy_(sp["logits"][0:1].expand_as(sp["logits"][1:]))
    logits0 = {"plain": bb["logits"].clone(), "shared": sp["logits"].clone()}
    bufs = {"plain": bb, "shared": sp}

    for w8 in (False, True):
        dec.enable_fp8_decode(w8)
        for nb in a.nb:
            attend = dec._shared_attend(sp, nb)
            steps = {"plain": lambda: dec._batched_step(nb, False), "shared": lambda: dec._batched_step(nb, False, sp, attend)}

            def reset(m):
                bufs[m]["pos"][:nb].fill_(ctx)
                bufs[m]["logits"].copy_(logits0[m])

            graphs, first = {}, {}
            for m in ("plain", "shared"):
                reset(m)
                b = bufs[m]
                graphs[m] = dec.capture_batch_graph(nb, False) if m == "plain" else \
                    dec._capture(steps[m], steps[m], (b["tok"], b["pos"], b["logits"], b["sstep"]))
                reset(m)
                graphs[m].replay()
                first[m] = (b["logits"][:nb].clone(), b["tok"][:nb].clone())
                reset(m)
                timed(graphs[m].replay, a.warmup, 1)
            rel = ((first["shared"][0] - first["plain"][0]).norm() / first["plain"][0].norm()).item()
            ts = {"plain": [], "shared": []}
            for _ in range(a.rounds):
                for m in ("plain", "shared"):
                    reset(m)
                    ts[m].append(timed(graphs[m].replay, 1, a.reps)["median_ms"])
            wbytes, _ = step_bytes(cfg, nb, ctx, w8)
            res = {}
            for m in ("plain", "shared"):
                t = sorted(ts[m])
                ms = t[len(t) // 2]
                kv_rows = nb * (ctx + 1) if m == "plain" else P + nb * (a.own + 1)          # positions whose K and V rows the step reads
                slot_rows = nb * smax if m == "plain" else nb * own_cap                     # (the shared mode also holds the prefix once: P rows)
                res[m] = dict(ms_per_step=round(ms, 4), min_ms=round(t[0], 4), max_ms=round(t[-1], 4), weight_GB=round(wbytes / 1e9, 3),
                              kv_GB=round(kv_rows * row_bytes / 1e9, 4), slot_memory_GB=round(slot_rows * row_bytes / 1e9, 4))
            emit(rows, a.out, what="batched decode step (graph replay), shared prompt prefix against the plain batched step", model="7B",
                 weights="fp8" if w8 else "16bit", nb=nb, prefix=P, own=a.own, own_cap=own_cap, max_seq_len=smax, rounds=a.rounds, reps=a.reps,
                 **res, shared_speedup=round(res["plain"]["ms_per_step"] / res["shared"]["ms_per_step"], 3),
                 shared_vs_plain_first_step_logits_rel_l2=rel, shared_first_step_tokens_equal_plain=bool(torch.equal(first["shared"][1], first["plain"][1])))


if __name__ == "__main__":
    with torch.no_grad():
        main()
