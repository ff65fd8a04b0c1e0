"""Growing reservations page by page and preemption by swap against whole reservations.  The 7B decoder at full
width (weights generated on the device from a seed), 16-bit pages, every request the same --ctx-row prompt with max_new_tokens=--budget that
really stops after --stop tokens (a stopping criterion): what a server sees, which does not know the stop in advance.
  drain     : N requests through max_slots slots on ONE pool size under reserve="whole" and under "grow": wall time to drain (host clock,
              device synchronised; prefills included, they are the same work in both), peak and mean requests in flight per step, steps,
              preemptions and resumes.  Two pool sizes: one that holds two whole reservations, one tight enough that "grow" preempts.
  step      : the step time at equal occupancy (max_slots requests in flight, roomy pool) on steps where no request crosses a page edge,
              host clock around step() (which ends in a device-to-host copy of the tokens), whole / grow / whole again per round: the two
              whole series give the run-to-run spread the grow figure is read against.  "whole" is the code path of the parent commit, untouched.
  swap      : one request with the pages it holds after --stop tokens (28 at the defaults) swapped out and in again --reps times: ms each way (host clock, device synchronised before
              and after), the GB/s the page bytes imply, and the plain pinned copy_ of the same bytes each way as the yardstick; then the
              request decodes on, and its tokens are compared with an unswapped run.
Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.fp8_batch_bench import emit      # noqa: E402


def stop_after(n):
    return lambda ids, _: ids.shape[1] >= n


def med(ts):
    ts = sorted(ts)
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), n=len(ts))


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, default=1650)
    ap.add_argument("--budget", type=int, default=2048)
    ap.add_argument("--stop", type=int, default=128)
    ap.add_argument("--requests", type=int, default=8)
    ap.add_argument("--max-slots", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-window", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-seq-len", type=int, default=4096)
    ap.add_argument("--layers", type=int, default=None, help="fewer decoder layers (rehearsals only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "paged_grow_bench.py measures on the GPU"
    from videollama2_amd.config import videollama2_7b
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.paging import pages_for, pages_needed, rows_next
    from videollama2_amd.serving import ContinuousBatcher
    from videollama2_amd.weights import LazyRandomStateDict
    cfg = videollama2_7b()
    dec = HipMistralDecoder(cfg, LazyRandomStateDict(cfg, "cuda", seed=1234), "cuda", max_seq_len=a.max_seq_len, n_layers=a.layers)
    torch.cuda.empty_cache()
    x = (0.5 * torch.randn(a.ctx, cfg["llm"]["hidden_size"], device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))).bfloat16()
    whole = pages_needed(a.ctx, a.budget, dec.max_seq_len)
    first, last = pages_for(rows_next(a.ctx, 0, dec.max_seq_len)), pages_for(rows_next(a.ctx, a.stop - 1, dec.max_seq_len))
    page_bytes = dec.kv_page_bytes()
    rows = []
    common = dict(model="7B", weights="16bit", pages="16bit", ctx=a.ctx, budget=a.budget, stop=a.stop, max_seq_len=dec.max_seq_len,
                  n_layers=dec.n_layers, page_MB=round(page_bytes / 1e6, 3), whole_reservation_pages=whole, pages_at_admission=first,
                  pages_at_stop=last)

    def batcher(reserve, n, stop):
        b = ContinuousBatcher(dec, max_slots=a.max_slots, use_graph=True, reserve=reserve)
        rid = [b.submit(x, max_new_tokens=a.budget, stopping_criteria=stop_after(stop)) for _ in range(n)]
        return b, rid

    # ---- drain time, occupancy, preemptions
    tight = a.max_slots * (last - 1)                  # the slots' pages at admission fit, their pages at the stop do not
    assert last > first and tight >= whole
    for label, usable in (("two whole reservations", 2 * whole), ("tight", tight)):
        dec.enable_paged_kv(usable + 1)                 # (drops the captured graphs)
        tokens = {}
        for reserve in ("whole", "grow"):               # unreported runs: they capture the step graph of every occupancy
            b, rid = batcher(reserve, a.requests, a.stop)
            b.run()
            tokens[reserve] = [b.finished[r].tolist() for r in rid]
        # measured runs: alternate the policies, each with its graphs warm
        for reserve in ("whole", "grow"):
            b, rid = batcher(reserve, a.requests, a.stop)
            per_step = []
            t0 = clock()
            while b.in_flight():
                out = b.step()
                per_step.append(len(out))
            t1 = clock()
            same = [b.finished[r].tolist() for r in rid] == tokens["whole"]
            emit(rows, a.out, what="drain N requests on one pool size", pool=label, usable_pages=usable, pool_GB=round((usable + 1) * page_bytes / 1e9, 3),
                 reserve=reserve, requests=a.requests, max_slots=a.max_slots, drain_s=round(t1 - t0, 4), steps=b.steps,
                 peak_in_flight=max(per_step), mean_in_flight=round(sum(per_step) / len(per_step), 3), preemptions=b.preemptions, resumes=b.resumes,
                 tokens_equal_whole=same, **common)
    # ---- step overhead at equal occupancy, on steps without a page edge
    dec.enable_paged_kv(a.max_slots * whole + 1)
    lead = 0
    while pages_for(rows_next(a.ctx, lead, dec.max_seq_len)) == first:       # run past the first edge, then time a window before the next one
        lead += 1
    lead += 2
    window = a.step_window
    assert len({pages_for(rows_next(a.ctx, k, dec.max_seq_len)) for k in range(lead, lead + window + 1)}) == 1, "the window crosses a page edge"
    series = dict(whole=[], grow=[], whole_again=[])
    for _ in range(a.rounds):
        for name, reserve in (("whole", "whole"), ("grow", "grow"), ("whole_again", "whole")):
            b, rid = batcher(reserve, a.max_slots, lead + window + 2)
            for _ in range(lead):
                b.step()
            assert sum(r is not None for r in b.slots) == a.max_slots
            ts = []
            for _ in range(window):
                t0 = clock()
                b.step()
                ts.append((clock() - t0) * 1e3)
            assert b.preemptions == 0
            b.run()
            series[name].append(med(ts)["median_ms"])
    res = {k: med(v) for k, v in series.items()}
    w, g, w2 = (res[k]["median_ms"] for k in ("whole", "grow", "whole_again"))
    emit(rows, a.out, what="step time at equal occupancy, no page edge in the window (host clock around step())", in_flight=a.max_slots,
         window_steps=window, rounds=a.rounds, **res, grow_over_whole=round(g / w, 4), whole_again_over_whole=round(w2 / w, 4), **common)
    # ---- swap cost
    dec.enable_paged_kv(whole + last + 2)
    runs = {}
    for swaps in (0, a.reps):
        b, rid = batcher("grow", 1, a.stop + 8)
        while len(b.slots[0].tokens if b.slots[0] is not None else []) < a.stop:
            b.step()
        r = b.slots[0]
        n_pages_req = len(r.pages)
        t_out, t_in, ids_seen = [], [], set()
        for i in range(swaps + 1 if swaps else 0):                             # the first cycle allocates the pinned buffers and the arena: not reported
            t0 = clock()
            b._swap_out(r)
            t1 = clock()
            b._admit_grow()
            t2 = clock()
            ids_seen.add(tuple(r.pages))
            if i:
                t_out.append((t1 - t0) * 1e3)
                t_in.append((t2 - t1) * 1e3)
        runs[swaps] = b.run()[rid[0]].tolist()
        if swaps:
            nbytes = n_pages_req * page_bytes
            dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            d2h, h2d = [], []
            for i in range(a.reps + 1):
                t0 = clock()
                host.copy_(dev, non_blocking=True)
                t1 = clock()
                dev.copy_(host, non_blocking=True)
                t2 = clock()
                if i:
                    d2h.append((t1 - t0) * 1e3)
                    h2d.append((t2 - t1) * 1e3)
            o, i_, c_o, c_i = med(t_out), med(t_in), med(d2h), med(h2d)
            gbs = lambda m: round(nbytes / (m["median_ms"] * 1e-3) / 1e9, 2)
            emit(rows, a.out, what="swap one request out and in (host clock, device synchronised)", request_pages=n_pages_req,
                 request_MB=round(nbytes / 1e6, 2), launches_each_way=dec.n_layers * 2, arena_MB=round(sum(t.numel() * t.element_size() for t in b._arena.values()) / 1e6, 3),
                 swap_out=o, swap_in=i_, swap_out_GBps=gbs(o), swap_in_GBps=gbs(i_), plain_pinned_d2h=c_o, plain_pinned_h2d=c_i,
                 plain_d2h_GBps=gbs(c_o), plain_h2d_GBps=gbs(c_i), swap_out_over_plain=round(o["median_ms"] / c_o["median_ms"], 3),
                 swap_in_over_plain=round(i_["median_ms"] / c_i["median_ms"], 3), **common)
    emit(rows, a.out, what="tokens after the swaps equal the unswapped run", equal=runs[0] == runs[a.reps], tokens=len(runs[0]), **common)


if __name__ == "__main__":
    with torch.no_grad():
        main()
