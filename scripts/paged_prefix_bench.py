"""The batched decode step over a shared prefix held once in the page pool, by the method of scripts/paged_kv_bench.py.
The 7B decoder at full width (weights generated on the device from a seed), nb questions about one video: a prefix of --prefix rows (its whole
pages, Pf = 64 * floor(prefix / 64), are shared; the tail is each request's) and --question own rows per request.  Three graph-replayed steps,
captured once each and alternated round by round in one process after warm-up (HIP events around the replays, device synchronised; median,
min, max over the rounds):
  (a) the plain paged step: every request holds the whole prompt in pages of its own (vl2_attn_decode_paged);
  (b) the contiguous shared step at P = Pf: the prefix in the single-sequence cache, own rows in private caches (vl2_attn_decode_shared);
  (c) the paged shared step: the prefix pages once, own pages per request, all dealt from one shuffled pool (vl2_attn_decode_shared_paged).
(a) and (b) are unchanged code.  (b) is measured TWICE per round (before and after (c)): its two series give the run-to-run spread.
max_seq_len = Pf + 192, so (b)'s private caches and (c)'s own pages both cover 192 own rows.  Output check (asserted): (c)'s logits and
tokens equal (b)'s bit for bit at every point.  Per point also the pool pages in use for (a) and for (c).
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
    ap.add_argument("--prefix", type=int, default=1621)
    ap.add_argument("--question", type=int, default=8)
    ap.add_argument("--max-new", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.nb = [int(n) for n in a.nb.split(",")]
    assert torch.cuda.is_available(), "paged_prefix_bench.py measures on the GPU"
    from videollama2_amd import ops
    from videollama2_amd.config import videollama2_7b
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.paging import own_pages_needed, pages_needed, shared_rows, table_row
    from videollama2_amd.weights import LazyRandomStateDict
    cfg = videollama2_7b()
    P, Pf = a.prefix, shared_rows(a.prefix)
    S = P + a.question
    own_cap = 192
    assert S - Pf + a.max_new <= own_cap
    dec = HipMistralDecoder(cfg, LazyRandomStateDict(cfg, "cuda", seed=1234), "cuda", max_seq_len=Pf + own_cap)
    torch.cuda.empty_cache()
    nmax, smax = max(a.nb), dec.max_seq_len
    need_a, need_c, n_pre = pages_needed(S, a.max_new, smax), own_pages_needed(P, a.question, a.max_new, smax), Pf // 64
    assert need_c == own_cap // 64
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = (0.5 * torch.randn(S, cfg["llm"]["hidden_size"], device="cuda", generator=gen)).bfloat16()       # prefix ++ question, the same for every request

    # (b) the prefix in the single-sequence cache, tail ++ question through extend, its rows into every request's private cache
    sp = dec._ensure_shared(nmax, Pf, own_cap)
    dec.prefill(x[:Pf])
    dec.extend(x[Pf:], start_pos=Pf, logits_out=sp["logits"][0])
    for li in range(dec.n_layers):
        sp["k"][li][:, :, :S - Pf].copy_(dec.kcache[li][None, :, Pf:S])
        sp["v"][li][:, :, :S - Pf].copy_(dec.vcache[li][None, :, Pf:S])
    sp["logits"][1:].copy_(sp["logits"][0:1].expand_as(sp["logits"][1:]))
    logits_shared = sp["logits"].clone()

    # one pool for (a) and (c), every page dealt from one shuffle
    n_pages = 1 + nmax * need_a + n_pre + nmax * need_c
    dec.enable_paged_kv(n_pages)
    bb = dec._ensure_batch(nmax)
    ids = bb["pool"].alloc(n_pages - 1)
    perm = torch.randperm(len(ids), generator=torch.Generator().manual_seed(0)).tolist()
    deal = iter(ids[i] for i in perm)
    take = lambda n: [next(deal) for _ in range(n)]
    pages_a = [take(need_a) for _ in range(nmax)]
    pre_pages = take(n_pre)
    pages_c = [take(need_c) for _ in range(nmax)]
    pps = bb["pages_per_seq"]
    table_a = torch.tensor([table_row(pg, pps) for pg in pages_a], dtype=torch.int32, device="cuda")
    table_c = torch.tensor([table_row(pre_pages + pg, pps) for pg in pages_c], dtype=torch.int32, device="cuda")
    prefix_pages = torch.tensor(pre_pages, dtype=torch.int32, device="cuda")
    partial_c = torch.empty((nmax * ops.shared_partial_floats(Pf, own_cap, dec.nh),), dtype=torch.float32, device="cuda")
    # (c) the single-sequence cache's rows into the prefix pages and into every request's own pages
    for li in range(dec.n_layers):
        pools = (bb["kpool"][li], bb["vpool"][li])
        ops.kv_page_scatter(dec.kcache[li], dec.vcache[li], *pools, table_c[0], 0, Pf)
        for b in range(nmax):
            ops.kv_page_scatter(dec.kcache[li], dec.vcache[li], *pools, table_c[b], Pf, S)
    # (a) the whole prompt prefilled through the staging cache, its rows into every request's pages
    bb["table"].copy_(table_a)
    dec.prefill_slot(0, x, bb["logits"][0])
    for b in range(1, nmax):
        for li in range(dec.n_layers):
            ops.kv_page_scatter(bb["stage"][0][li], bb["stage"][1][li], bb["kpool"][li], bb["vpool"][li], table_a[b], 0, S)
    logits_plain = bb["logits"][0:1].expand_as(bb["logits"]).clone()

    def attend_c_for(nb):
        def attend(li, qkv, o):
            ops.attn_decode_shared_paged(qkv, bb["kpool"][li], bb["vpool"][li], table_c, prefix_pages, bb["cos_t"], bb["sin_t"], partial_c, o, dec.nh,
                                         dec.nkv, Pf, own_cap, bb["pos"][:nb], dec.hd ** -0.5)
        return attend

    page_bytes = dec.kv_page_bytes()
    rows = []
    for nb in a.nb:
        def reset(which):
            buf, lg = (sp, logits_shared) if which == "b" else (bb, logits_plain if which == "a" else logits_shared)
            buf["pos"][:nb].fill_(S)
            buf["logits"].copy_(lg)

        graphs = {}
        reset("a")
        graphs["a"] = dec.capture_batch_graph(nb, False)
        reset("b")
        attend_b = dec._shared_attend(sp, nb)
        step_b = lambda: dec._batched_step(nb, False, sp, attend_b)
        graphs["b"] = dec._capture(step_b, step_b, (sp["tok"], sp["pos"], sp["logits"], sp["sstep"]))
        reset("c")
        graphs["c"] = dec.capture_batch_graph(nb, False, attend_c_for(nb), ("prefix", Pf))
        out = {}
        for which in ("a", "b", "c"):
            reset(which)
            timed(graphs[which].replay, a.warmup, 1)
            reset(which)
            graphs[which].replay()
            buf = sp if which == "b" else bb
            out[which] = (buf["logits"][:nb].clone(), buf["tok"][:nb].clone())
        same_logits, same_tok = bool(torch.equal(out["c"][0], out["b"][0])), bool(torch.equal(out["c"][1], out["b"][1]))
        assert same_logits and same_tok, f"nb {nb}: the paged shared step differs from the contiguous shared step"
        ts = dict(plain_paged=[], shared=[], shared_paged=[], shared_again=[])
        for _ in range(a.rounds):
            for name, which in (("plain_paged", "a"), ("shared", "b"), ("shared_paged", "c"), ("shared_again", "b")):
                reset(which)
                ts[name].append(timed(graphs[which].replay, 1, a.reps)["median_ms"])
        res = {}
        for name, t in ts.items():
            t = sorted(t)
            res[name] = dict(ms_per_step=round(t[len(t) // 2], 4), min_ms=round(t[0], 4), max_ms=round(t[-1], 4))
        pa, sb, sc, sb2 = (res[k]["ms_per_step"] for k in ("plain_paged", "shared", "shared_paged", "shared_again"))
        emit(rows, a.out, what="batched decode step (graph replay) over a shared prefix: plain paged (a), contiguous shared (b), paged shared (c)",
             model="7B", weights="16bit", nb=nb, prefix=P, shared_rows=Pf, tail=P - Pf, question=a.question, max_new=a.max_new, max_seq_len=smax,
             own_cap=own_cap, rounds=a.rounds, reps=a.reps, **res, shared_paged_over_shared=round(sc / sb, 4),
             shared_again_over_shared=round(sb2 / sb, 4), shared_paged_over_plain_paged=round(sc / pa, 4),
             plain_paged_tokens_equal_shared=bool(torch.equal(out["a"][1], out["b"][1])),
             pages_in_use_plain_paged=nb * need_a, pages_in_use_shared_paged=n_pre + nb * need_c, page_MB=round(page_bytes / 1e6, 3),
             pool_GB_plain_paged=round(nb * need_a * page_bytes / 1e9, 3), pool_GB_shared_paged=round((n_pre + nb * need_c) * page_bytes / 1e9, 3),
             shared_paged_logits_equal_shared=same_logits, shared_paged_tokens_equal_shared=same_tok)


if __name__ == "__main__":
    with torch.no_grad():
        main()
