"""The batched decode step on fp8 pages against the contiguous fp8-KV slots, by scripts/paged_kv_bench.py's method.  The
7B decoder at full width (weights generated on the device from a seed), every slot holding the same --ctx-row prompt, nb requests: the
graph-replayed batched step on the contiguous fp8-KV slots (enable_fp8_kv), on fp8 pages (enable_paged_kv(fp8=True)) and on 16-bit pages
(enable_paged_kv), each request's pages dealt from a shuffled pool (no two of its pages are neighbours), captured once each and alternated
round by round in one process after warm-up (HIP events around the replays, device synchronised; median, min, max over the rounds).  The
yardstick is the contiguous fp8-KV step -- unchanged code -- measured TWICE per round, before and after the fp8-paged one: its two series
give the run-to-run spread the fp8-paged figure is read against (the bytes are equal by construction; the paged step adds one dependent
4-byte load per workgroup).  The 16-bit paged step is timed in the same rounds.  Per point also: the pool bytes this request mix (--ctx
prompt rows + --max-new tokens) reserves on fp8 pages, on 16-bit pages and in contiguous fp8 slots at this max_seq_len and at 4096.
Output check, asserted: the fp8-paged graph's logits and tokens equal the contiguous fp8-KV graph's bit for bit.
Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.fp8_batch_bench import emit, timed      # noqa: E402  (the timing loop is that script's)

MODES = ("contiguous_fp8kv", "paged_fp8", "paged_16bit")


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
    assert torch.cuda.is_available(), "paged_fp8kv_bench.py measures on the GPU"
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
    bbs = {}

    def select(mode):
        """The decoder's switches for `mode` (each drops the captured graphs and the slot buffers of the other layout ...)."""
        dec.enable_paged_kv(0, False)
        dec.enable_fp8_kv(mode == "contiguous_fp8kv")
        if mode != "contiguous_fp8kv":
            dec.enable_paged_kv(n_pages, fp8=mode == "paged_fp8")
        dec._bb = bbs.get(mode)                 # ... which this script keeps: every graph replays on its own buffers

    # the three sets of slots stay alive side by side; the same prompt in every slot (prefilled once, then copied / quantised / scattered)
    select("contiguous_fp8kv")
    bb = bbs["contiguous_fp8kv"] = dec._ensure_batch(nmax)
    dec.prefill_slot(0, x, bb["logits"][0])
    for kv8 in bb["kv8"]:
        for t in kv8:
            t[1:].copy_(t[0:1].expand_as(t[1:]))
    perm = None
    for mode in ("paged_fp8", "paged_16bit"):
        select(mode)
        bb = bbs[mode] = dec._ensure_batch(nmax)
        ids = bb["pool"].alloc(nmax * need)
        perm = torch.randperm(len(ids), generator=torch.Generator().manual_seed(0)).tolist() if perm is None else perm
        pages = [[ids[perm[b * need + j]] for j in range(need)] for b in range(nmax)]
        dec._set_table_rows(0, [table_row(pg, bb["pages_per_seq"]) for pg in pages])
        dec.prefill_slot(0, x, bb["logits"][0])
        for b in range(1, nmax):
            for li in range(dec.n_layers):
                if mode == "paged_fp8":
                    ops.kv_page_quant(bb["stage"][0][li], bb["stage"][1][li], bb["pools8"][li], bb["table"][b], 0, a.ctx)
                else:
                    ops.kv_page_scatter(bb["stage"][0][li], bb["stage"][1][li], bb["kpool"][li], bb["vpool"][li], bb["table"][b], 0, a.ctx)
    for b_ in bbs.values():
        b_["logits"][1:].copy_(b_["logits"][0:1].expand_as(b_["logits"][1:]))
    logits0 = bbs["contiguous_fp8kv"]["logits"].clone()
    assert all(torch.equal(b_["logits"], logits0) for b_ in bbs.values())     # the prefill does not depend on the slots' layout or format
    page_bytes = {}
    for mode in ("paged_fp8", "paged_16bit"):
        select(mode)
        page_bytes[mode] = dec.kv_page_bytes()
    slot8_bytes = lambda rows: dec.n_layers * 2 * dec.nkv * rows * (128 + 4)

    rows = []
    for nb in a.nb:
        def reset(mode):
            bbs[mode]["pos"][:nb].fill_(a.ctx)
            bbs[mode]["logits"].copy_(logits0)

        graphs, out = {}, {}
        for mode in MODES:
            select(mode)
            reset(mode)
            graphs[mode] = dec.capture_batch_graph(nb, False)
            reset(mode)
            timed(graphs[mode].replay, a.warmup, 1)
        for mode in MODES:
            reset(mode)
            graphs[mode].replay()
            out[mode] = (bbs[mode]["logits"][:nb].clone(), bbs[mode]["tok"][:nb].clone())
        same_logits = bool(torch.equal(out["paged_fp8"][0], out["contiguous_fp8kv"][0]))
        same_tok = bool(torch.equal(out["paged_fp8"][1], out["contiguous_fp8kv"][1]))
        assert same_logits and same_tok, f"nb {nb}: the fp8-paged step differs from the contiguous fp8-KV step"
        series = (("contiguous_fp8kv", "contiguous_fp8kv"), ("paged_fp8", "paged_fp8"), ("contiguous_fp8kv_again", "contiguous_fp8kv"),
                  ("paged_16bit", "paged_16bit"))
        ts = {name: [] for name, _ in series}
        for _ in range(a.rounds):
            for name, mode in series:
                reset(mode)
                ts[name].append(timed(graphs[mode].replay, 1, a.reps)["median_ms"])
        res = {}
        for name, t in ts.items():
            t = sorted(t)
            res[name] = dict(ms_per_step=round(t[len(t) // 2], 4), min_ms=round(t[0], 4), max_ms=round(t[-1], 4))
        c, c2 = res["contiguous_fp8kv"]["ms_per_step"], res["contiguous_fp8kv_again"]["ms_per_step"]
        p8, p16 = res["paged_fp8"]["ms_per_step"], res["paged_16bit"]["ms_per_step"]
        emit(rows, a.out, what="batched decode step (graph replay), fp8 pages against contiguous fp8-KV slots and 16-bit pages", model="7B",
             weights="16bit", nb=nb, ctx=a.ctx, max_new=a.max_new, max_seq_len=smax, rounds=a.rounds, reps=a.reps, **res,
             paged_fp8_over_contiguous_fp8kv=round(p8 / c, 4), contiguous_again_over_contiguous=round(c2 / c, 4),
             paged_fp8_over_paged_16bit=round(p8 / p16, 4), pages_per_request=need, fp8_page_MB=round(page_bytes["paged_fp8"] / 1e6, 3),
             page_16bit_MB=round(page_bytes["paged_16bit"] / 1e6, 3), fp8_pool_GB_for_this_mix=round(nb * need * page_bytes["paged_fp8"] / 1e9, 3),
             pool_16bit_GB_for_this_mix=round(nb * need * page_bytes["paged_16bit"] / 1e9, 3),
             contiguous_fp8_GB_at_max_seq_len=round(nb * slot8_bytes(smax) / 1e9, 3), contiguous_fp8_GB_at_4096=round(nb * slot8_bytes(4096) / 1e9, 3),
             paged_fp8_graph_logits_equal_contiguous_fp8kv=same_logits, paged_fp8_graph_tokens_equal_contiguous_fp8kv=same_tok)


if __name__ == "__main__":
    with torch.no_grad():
        main()
