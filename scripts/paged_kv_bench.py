"""The batched decode step on the paged KV cache against the contiguous slots.  The 7B decoder at full width (weights
generated on the device from a seed), every slot holding the same --ctx-row prompt, nb requests: the graph-replayed batched step on the
contiguous slots and on pages of a shared pool (each request's pages dealt from a shuffled pool, so no two of its pages are neighbours),
captured once each and alternated round by round in one process after warm-up (HIP events around the replays, device synchronised; median,
min, max over the rounds).  The contiguous step is measured TWICE per round (before and after the paged one): the two contiguous series
give the run-to-run spread the paged figure is read against.  The bytes are equal by construction -- the paged step adds one dependent
4-byte load per workgroup -- so the contiguous step, unchanged code, is the yardstick.  Per point also: the pool bytes this request mix
(--ctx prompt rows + --max-new tokens) reserves against the contiguous slots' bytes at this max_seq_len and at 4096.  Output check: the
paged graph's logits and tokens equal the contiguous graph's bit for bit.
Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.fp8_batch_bench import emit, timed      # noqa: E402  (the timing loop is that script's)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", default="1,4,16,64")
    ap.add_argument("--ctx", type=int, default=1650)
    ap.add_argument("--max-new", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.nb = [int(n) for n in a.nb.split(",")]
    assert torch.cuda.is_available(), "paged_kv_bench.py measures on the GPU"
    from videollama2_amd import ops
    from videollama2_amd.config import videollama2_7b
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.paging import pages_needed, table_row
    from videollama2_amd.weights import LazyRandomStateDict
    cfg = videollama2_7b()
    dec = HipMistralDecoder(cfg, LazyRandomStateDict(cfg, "cuda", seed=1234), "cuda", max_seq_len=a.ctx + 256)
    torch.cuda.empty_cache()
    nmax, smax = max(a.nb), dec.max_seq_len
    need = pages_needed(a.ctx, a.max_new, smax)
    n_pages = nmax * need + 1
    x = (0.5 * torch.randn(a.ctx, cfg["llm"]["hidden_size"], device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))).bfloat16()
    # both sets of slots stay alive side by side; the same prompt in every slot (prefilled once, then copied / scattered)
    bbs = {}
    bb = bbs[False] = dec._ensure_batch(nmax)
    dec.prefill_slot(0, x, bb["logits"][0])
    for t in bb["k"] + bb["v"]:
        t[1:].copy_(t[0:1].expand_as(t[1:]))
    dec.enable_paged_kv(n_pages)
    bb = bbs[True] = dec._ensure_batch(nmax)
    ids = bb["pool"].alloc(nmax * need)
    perm = torch.randperm(len(ids), generator=torch.Generator().manual_seed(0)).tolist()
    pages = [[ids[perm[b * need + j]] for j in range(need)] for b in range(nmax)]
    dec._set_table_rows(0, [table_row(pg, bb["pages_per_seq"]) for pg in pages])
    dec.prefill_slot(0, x, bb["logits"][0])
    for b in range(1, nmax):
        for li in range(dec.n_layers):
            ops.kv_page_scatter(bb["stage"][0][li], bb["stage"][1][li], bb["kpool"][li], bb["vpool"][li], bb["table"][b], 0, a.ctx)
    for b_ in bbs.values():
        b_["logits"][1:].copy_(b_["logits"][0:1].expand_as(b_["logits"][1:]))
    assert torch.equal(bbs[True]["logits"], bbs[False]["logits"])             # the prefill does not depend on the slots' layout
    logits0 = bbs[False]["logits"].clone()
    page_bytes = dec.kv_page_bytes()
    slot_bytes = lambda rows: dec.n_layers * 2 * dec.nkv * rows * 128 * 2

    def select(paged):
        dec.enable_paged_kv(n_pages, paged)     # (drops the captured graphs and the slot buffers of the other layout ...)
        dec._bb = bbs[paged]                    # ... which this script keeps: both graphs replay on their own buffers

    rows = []
    for nb in a.nb:
        def reset(paged):
            bbs[paged]["pos"][:nb].fill_(a.ctx)
            bbs[paged]["logits"].copy_(logits0)

        graphs = {}
        for paged in (False, True):
            select(paged)
            reset(paged)
            graphs[paged] = dec.capture_batch_graph(nb, False)
            reset(paged)
            timed(graphs[paged].replay, a.warmup, 1)
        out = {}
        for paged in (False, True):
            reset(paged)
            graphs[paged].replay()
            out[paged] = (bbs[paged]["logits"][:nb].clone(), bbs[paged]["tok"][:nb].clone())
        same_logits, same_tok = bool(torch.equal(out[True][0], out[False][0])), bool(torch.equal(out[True][1], out[False][1]))
        ts = dict(contiguous=[], paged=[], contiguous_again=[])
        for _ in range(a.rounds):
            for name, paged in (("contiguous", False), ("paged", True), ("contiguous_again", False)):
                reset(paged)
                ts[name].append(timed(graphs[paged].replay, 1, a.reps)["median_ms"])
        res = {}
        for name, t in ts.items():
            t = sorted(t)
            res[name] = dict(ms_per_step=round(t[len(t) // 2], 4), min_ms=round(t[0], 4), max_ms=round(t[-1], 4))
        c, c2, p = res["contiguous"]["ms_per_step"], res["contiguous_again"]["ms_per_step"], res["paged"]["ms_per_step"]
        emit(rows, a.out, what="batched decode step (graph replay), paged KV cache against contiguous slots", model="7B", weights="16bit", nb=nb,
             ctx=a.ctx, max_new=a.max_new, max_seq_len=smax, rounds=a.rounds, reps=a.reps, **res,
             paged_over_contiguous=round(p / c, 4), contiguous_again_over_contiguous=round(c2 / c, 4),
             pages_per_request=need, page_MB=round(page_bytes / 1e6, 3), pool_GB_for_this_mix=round(nb * need * page_bytes / 1e9, 3),
             contiguous_GB_at_max_seq_len=round(nb * slot_bytes(smax) / 1e9, 3), contiguous_GB_at_4096=round(nb * slot_bytes(4096) / 1e9, 3),
             paged_graph_logits_equal_contiguous=same_logits, paged_graph_tokens_equal_contiguous=same_tok)


if __name__ == "__main__":
    with torch.no_grad():
        main()
