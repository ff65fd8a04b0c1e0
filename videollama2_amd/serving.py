"""Continuous batching: new requests are admitted BETWEEN decode steps, finished ones leave at once.

The reference's worker (videollama2/serve/model_worker.py:263-300 `generate_stream`, :350-352 the `limit_model_concurrency`
semaphore) lets several requests be in flight, each in its own `model.generate` thread with a TextIteratorStreamer; on one GPU
those generate loops serialise kernel by kernel.  Here the in-flight requests share ONE decode step per token: every request
owns a slot (its KV-cache slice, position and current token live on the device), a step streams the weights once for all
occupied slots (decoder._decode_kernels_batched), and between two steps
  * requests that hit EOS / a stop criterion / max_new_tokens / the cache end are retired (their streamer gets `end()`),
  * waiting requests are prefilled straight into a free slot's cache and join the next step.
With at most 4 slots the step runs the multi-row GEMV whose rows are bit-identical to the single-sequence step, so a request's
tokens do not depend on what else is in flight or when it was admitted (asserted in the tests).
A request may sample (`submit(do_sample=True, ...)`, the worker's `temperature > 0.001` requests): its settings and its row of uniform numbers go
into its slot at admission, and a step that holds any sampled request draws every slot's token in ONE ops.sample_tokens launch (greedy slots
take the argmax there), so it still replays from one captured graph per occupancy."""
import collections
import itertools

import torch

from . import _lib
from .decoder import eos_set
from .paging import (PAGE_ROWS, admit_fifo, admit_grow, own_pages_needed, pages_for, pages_needed, parked_row, plan_growth, prefix_parked_row,
                     rows_next, shared_rows, table_row)


class _Request:
    __slots__ = ("rid", "x", "max_new", "streamer", "criteria", "tokens", "slot", "done", "sampler", "u", "need", "pages", "S", "order", "swap")

    def __init__(self, rid, x, max_new, streamer, criteria, sampler=None, u=None):
        self.rid, self.x, self.max_new, self.streamer, self.criteria = rid, x, max_new, streamer, criteria
        self.sampler, self.u = sampler, u              # (temperature, top_k, top_p) and the request's uniform numbers, or None: greedy
        self.tokens, self.slot, self.done = [], None, False
        self.need, self.pages = 0, None                # paged KV: the reservation (pages) and, once admitted, the page ids
        self.S, self.order, self.swap = 0, None, None  # reserve="grow": prompt rows, admission order, and while swapped out (pinned pages, logits row)


class PrefixHandle:
    """A resident prefix of a ContinuousBatcher (`open_prefix`): P prompt rows of which the first `shared_rows` = 64 * floor(P / 64) live
    once in the page pool, in `pages`; the ragged tail rows are kept here and prepended to every request's suffix."""
    __slots__ = ("P", "shared_rows", "pages", "tail", "open", "epoch", "own_cap", "prefix_pages", "partial", "ids")

    def __init__(self, P, pages, tail):
        self.P, self.shared_rows, self.pages, self.tail = P, shared_rows(P), list(pages), tail
        self.open, self.epoch, self.ids = True, None, None


class ContinuousBatcher:
    """decoder: HipMistralDecoder.  max_slots: requests decoding together (<= 4 keeps every request bit-identical to its
    solo greedy decode; more switches the step to the skinny-M MFMA path, equal to bf16 rounding).
    use_graph (default: on a GPU): one captured hipGraph per occupancy (highest occupied slot + 1).
    fp8 / MXFP4 decode weights (decoder.enable_fp8_decode() / enable_mxfp4_decode()): the steps stream those copies, with the same guarantees
    against the solo decode on the same copies.  Toggling them with requests in flight is allowed: the toggle drops the captured step graphs, the next step runs (and captures) every
    slot on the weights then selected, and the decoder's cache_epoch is bumped as for any toggle.
    fp8 KV cache (decoder.enable_fp8_kv()): the slots hold fp8 rows only (0.52 x the memory), a request is prefilled into the decoder's 16-bit
    staging cache and quantised into its slot, and the steps attend on the fp8 rows -- a request's tokens equal its solo fp8-KV decode.  That
    switch changes the slots' format, so the decoder refuses it while requests are in flight.
    paged KV cache (decoder.enable_paged_kv(n_pages)): the slots' rows live in pages of 64 positions from one shared pool, so max_slots costs a
    table row each and a request holds pages_needed(S, max_new, max_seq_len) pages from admission to retirement.  Admission is strict FIFO on
    the WHOLE reservation (`paging.admit_fifo`): the head of the queue joins only when a slot is free and the pool holds all its pages,
    otherwise nobody is admitted in that step -- so no request can run out of pages in flight and the step's graph replays untouched (it reads
    the page table from the device).  A request's tokens are bit for bit the contiguous slots'.  A request that can never fit the pool is
    refused at `submit`.  The decoder refuses the switch with requests in flight.
    reserve="grow" (needs the paged KV cache, 16-bit or fp8 pages; the default "whole" is everything above, untouched): the
    pool follows the rows that exist.  A request is admitted on the pages of its prompt (`paging.admit_grow`), takes one more page each time it
    crosses a 64-row edge (one `_set_table_rows` copy; the captured step graphs read the table from the device and are never re-captured), and
    when the pool is dry the newest admitted request is SWAPPED OUT (`paging.plan_growth`): its pages go through one small device arena
    (`ops.kv_pages_move`) into pinned host memory, byte for byte, with its row of logits; its slot and pages are freed, and it waits in
    `swapped`, which is served before `waiting`, oldest first.  A resumed request may land in another slot and on other page ids.  Nothing is
    recomputed, so a request's tokens stay bit for bit those of its solo decode.  `submit` still refuses a request whose WORST-CASE reservation
    exceeds the pool: that is what lets the oldest request always finish alone.  `preemptions` / `resumes` count the events.  Not built: growth
    behind a resident prefix (`open_prefix` is refused), a cap on host swap memory, growth in `generate_batch`, recompute-style preemption.
    fp8 pages (decoder.enable_paged_kv(n_pages, fp8=True)): the same reservations, admission and retirement on pages of
    fp8 rows; a request is prefilled into the staging cache and quantised into its pages, and its tokens are bit for bit those of the
    contiguous fp8-KV slots.  A resident prefix is refused on them.
    resident prefix (`open_prefix(x_prefix)` under the paged KV cache): many questions about one video arriving over time.
    The whole pages of the prefix are held ONCE in the pool and appear under the same ids in every request's table row; a request reserves
    only its own pages, and the step reads the prefix once for all requests (`ops.attn_decode_shared_paged`).  While it is open every
    `submit` names it (`prefix=handle`); a request's tokens are bit for bit its solo
    `generate_batch([cat(x_prefix[Pf:], suffix)], shared_prefix=x_prefix[:Pf])` on an unpaged decoder, Pf = the shared rows.  One prefix at a
    time; `close_prefix()` returns its pages."""

    reserve = "whole"           # the reservation policy: "whole" (admission to retirement) | "grow" (page by page, preemption by swap)
    swapped = ()                # (reserve="grow": the requests swapped out to host memory)

    def __init__(self, decoder, max_slots=4, eos_token_id=None, use_graph=None, reserve="whole"):
        if decoder.tp > 1:
            raise NotImplementedError("continuous batching is built for the single-GPU decoder")
        if reserve not in ("whole", "grow"):
            raise ValueError(f"ContinuousBatcher: reserve must be \"whole\" or \"grow\", got {reserve!r}")
        if reserve == "grow" and not decoder.paged_kv:
            raise RuntimeError("ContinuousBatcher: reserve=\"grow\" grows reservations in the page pool: call decoder.enable_paged_kv(n_pages) "
                               "first")
        self.reserve = reserve
        self.swapped = collections.deque()      # reserve="grow": the requests swapped out to host memory, oldest first
        self.preemptions = self.resumes = 0
        self._orders = itertools.count()
        self._arena = {}                        # reserve="grow": one reusable device arena of pages_per_seq pages per pool kind
        self.dec = decoder
        self.max_slots = int(max_slots)
        self.eos = eos_set(eos_token_id)
        self.use_graph = (decoder._dev.type == "cuda") if use_graph is None else bool(use_graph)
        self.waiting = collections.deque()
        self.slots = [None] * self.max_slots
        self.finished = {}
        self._ids = itertools.count()
        self.steps = 0
        self.bb = decoder._ensure_batch(self.max_slots, owner=self)
        self._prefix = None                     # the resident prefix (PrefixHandle), or None

    # ---- the resident prefix
    @torch.no_grad()
    def open_prefix(self, x_prefix):
        """Make x_prefix [P, D] (the spliced rows every coming request begins with) resident: prefill its shared rows Pf = 64 * floor(P / 64)
        once, keep them in Pf / 64 pages of the pool for as long as the prefix is open, and point every slot's table row at them.  Returns
        the handle `submit(..., prefix=handle)` takes (`.P`, `.shared_rows`, `.pages`).  Refused before any kernel call: a decoder the
        shared-prefix mode refuses (tensor parallelism, head_dim != 128, fp8 prefill, Mixtral), no paged KV cache, fp8 pages, requests waiting or in
        flight, a prefix already open, fewer than 64 rows, a prefix that leaves no room for a suffix row, a pool too small."""
        from .ops import shared_partial_floats
        dec = self.dec
        self._open_prefix_refusals()
        P = int(x_prefix.shape[0])
        Pf = shared_rows(P)
        if Pf < PAGE_ROWS:
            raise ValueError(f"open_prefix: a prefix of {P} rows has no whole page of {PAGE_ROWS} rows to share")
        if P + 1 > dec.max_seq_len:
            raise ValueError(f"open_prefix: a prefix of {P} rows leaves no room for a suffix row in the KV cache ({dec.max_seq_len})")
        bb = dec._ensure_batch(self.max_slots, owner=self)
        self.bb = bb                            # (nothing is in flight: buffers reallocated since the last step lose nobody's rows)
        n_pre, smallest = Pf // PAGE_ROWS, own_pages_needed(P, 1, 1, dec.max_seq_len)
        if n_pre + smallest > bb["pool"].n_free:
            raise ValueError(f"open_prefix: the prefix needs {n_pre} pages and one request at least {smallest} more, the pool has "
                             f"{bb['pool'].n_free} free (of {bb['pool'].n_pages - 1}; enable_paged_kv(n_pages))")
        pps = bb["pages_per_seq"]
        x_prefix = x_prefix.to(device=dec._dev)
        h = PrefixHandle(P, bb["pool"].alloc(n_pre), x_prefix[Pf:].clone())
        try:
            dec.prefill(x_prefix[:Pf])                              # into the single-sequence cache: what every request's extend reads
            dec._set_table_rows(0, [prefix_parked_row(h.pages, pps)] * self.max_slots)
            dec._prefix_rows_to_pages(0, 0, Pf)
            h.epoch = dec.cache_epoch
            h.own_cap = PAGE_ROWS * (pps - n_pre)
            h.prefix_pages = torch.tensor(h.pages, dtype=torch.int32).to(dec._dev)
            h.partial = torch.empty((self.max_slots * shared_partial_floats(Pf, h.own_cap, dec.nh),), dtype=torch.float32, device=dec._dev)
        except BaseException:
            bb["pool"].free(h.pages)
            dec._set_table_rows(0, [parked_row(pps)] * self.max_slots)
            raise
        self._drop_prefix_graphs()
        self._prefix = h
        return h

    def _open_prefix_refusals(self):
        """The refusals of open_prefix that do not depend on the prefix (ModelBatcher.open_video makes them before the encoder runs)."""
        dec = self.dec
        if self.reserve == "grow":
            raise NotImplementedError("open_prefix: this batcher grows its reservations page by page (reserve=\"grow\") and growth behind a "
                                      "resident prefix is not built: use a reserve=\"whole\" batcher")
        dec._shared_prefix_refusals(paged_ok=True)       # everything the shared-prefix mode refuses, except paging itself
        if not dec.paged_kv:
            raise RuntimeError("open_prefix: the resident prefix lives in the page pool: call decoder.enable_paged_kv(n_pages) first")
        if dec.paged_kv_fp8:
            raise NotImplementedError("open_prefix: the pages hold fp8 rows and no fp8 form of the shared-prefix kernels is built (the prefix "
                                      "phase and extend read 16-bit rows): call decoder.enable_paged_kv(n_pages) for 16-bit pages first")
        if self.in_flight():
            raise RuntimeError(f"open_prefix: {self.in_flight()} requests are waiting or in flight: drain them (run()) first")
        if self._prefix is not None:
            raise RuntimeError("open_prefix: a prefix is open already (one resident prefix per batcher): close_prefix() first")

    def close_prefix(self):
        """Give the prefix pages back and park every slot on page 0 again.  Refused with requests waiting or in flight."""
        h = self._prefix
        if h is None:
            raise RuntimeError("close_prefix: no prefix is open")
        if self.in_flight():
            raise RuntimeError(f"close_prefix: {self.in_flight()} requests are waiting or in flight: drain them (run()) first")
        h.open, self._prefix = False, None
        self._drop_prefix_graphs()
        if self.dec._bb is self.bb:             # (reallocated buffers took the pool and the table with them)
            self.bb["pool"].free(h.pages)
            self.dec._set_table_rows(0, [parked_row(self.bb["pages_per_seq"])] * self.max_slots)

    def _drop_prefix_graphs(self):
        graphs = self.dec.__dict__.get("_batch_graphs", {})
        for key in [k for k in graphs if "prefix" in k]:
            del graphs[key]

    # ---- admission
    def submit(self, inputs_embeds, max_new_tokens=2048, streamer=None, stopping_criteria=None, do_sample=False, temperature=None, top_k=None,
               top_p=None, generator=None, prefix=None, **warpers):
        """Queue one request (inputs_embeds [S, D]: the spliced prompt of `prepare_inputs_labels_for_multimodal`).  It is prefilled
        and joins the batch at the next `step()` with a free slot.  Returns the request id.
        do_sample=True: HF `_sample` with the warpers temperature -> top_k -> top_p, HF's defaults (1.0, 50, 1.0) for the unspecified ones and
        HF's checks, as `VideoLLaMA2Hip.generate(do_sample=True)`; other warpers (`repetition_penalty`, ...) are refused unless neutral.  The
        request's uniform numbers are drawn here from `generator` (or torch's generator for the device), as many and in the same call as a solo
        `HipMistralDecoder.generate(sampler=...)` of this request draws them, so it samples the same tokens under the same seed.
        prefix=handle (`open_prefix`): inputs_embeds holds only the request's own n >= 1 rows; its prompt is the prefix's P rows and then
        these, and it reserves only the pages behind the prefix's whole pages.  While a prefix is open every request names it."""
        from .model import UNBUILT_WARPERS, resolve_sampler
        h = self._prefix
        if prefix is not None and self.reserve == "grow":
            raise NotImplementedError("submit: this batcher grows its reservations page by page (reserve=\"grow\") and growth behind a resident "
                                      "prefix is not built: submit without prefix=, or use a reserve=\"whole\" batcher")
        if prefix is not h:
            if prefix is None:
                raise ValueError("submit: a prefix is open on this batcher: pass prefix=handle (plain and prefix requests do not share a step), "
                                 "or close_prefix() first")
            raise ValueError("submit: the prefix handle is closed or was opened on another batcher" if isinstance(prefix, PrefixHandle)
                             else f"submit: prefix must be the handle open_prefix returned, got {type(prefix).__name__}")
        unknown = set(warpers) - {k for k, _ in UNBUILT_WARPERS}
        if unknown:
            raise TypeError(f"submit() got unexpected keyword arguments {sorted(unknown)}")
        given = dict(temperature=temperature, top_k=top_k, top_p=top_p, **warpers)
        sampler = resolve_sampler(dict({k: v for k, v in given.items() if v is not None}, do_sample=do_sample, generator=generator))
        S = inputs_embeds.shape[0]
        if h is not None:                # the prompt is prefix ++ suffix
            if S < 1:
                raise ValueError("submit: a request behind a prefix needs at least one row of its own")
            S += h.P
        if S > self.dec.max_seq_len:
            raise ValueError(f"sequence length {S} exceeds the KV cache ({self.dec.max_seq_len})")
        crit = stopping_criteria
        if crit is not None and not isinstance(crit, (list, tuple)):
            crit = [crit]
        max_new = min(int(max_new_tokens), self.dec.max_seq_len - S + 1)
        need = 0
        if h is not None:                # its own pages only; the pool it can ever draw on excludes the prefix pages
            need = own_pages_needed(h.P, S - h.P, max_new, self.dec.max_seq_len)
            if need > self.dec._n_pages - 1 - len(h.pages):
                raise ValueError(f"paged KV cache: the request needs {need} pages of its own ({h.P} prefix rows + {S - h.P} rows + {max_new} new "
                                 f"tokens), the pool serves {self.dec._n_pages - 1 - len(h.pages)} beside the prefix's {len(h.pages)} "
                                 f"(enable_paged_kv(n_pages); page 0 is the parking page)")
            inputs_embeds = torch.cat([h.tail, inputs_embeds.to(device=h.tail.device, dtype=h.tail.dtype)])   # the rows its extend computes
        elif self.dec.paged_kv:          # its whole reservation; one that the pool can never hold would block the queue for ever
            need = pages_needed(S, max_new, self.dec.max_seq_len)
            if need > self.dec._n_pages - 1:
                raise ValueError(f"paged KV cache: the request needs {need} pages ({S} prompt rows + {max_new} new tokens), the pool serves "
                                 f"{self.dec._n_pages - 1} (enable_paged_kv(n_pages); page 0 is the parking page)")
        u = None
        if sampler is not None:
            u = torch.rand((max_new,), device=self.dec._dev, generator=sampler[3])
            sampler = sampler[:3]
        r = _Request(next(self._ids), inputs_embeds, max_new, streamer, crit, sampler, u)
        r.need, r.S = need, S
        self.waiting.append(r)
        return r.rid

    # ---- reserve="grow": growth, preemption by swap, admission on the pages of the prompt
    def _pos(self, r):
        """The position of r's next token = the rows its cache holds: host arithmetic, no device read."""
        return r.S + len(r.tokens)

    def _pools_of(self, li):
        """Layer li's pool tensors, every kind: (kpool, vpool) on 16-bit pages, (k8pool, v8pool, kspool, vspool) on fp8 pages."""
        bb = self.bb
        return bb["pools8"][li] if "pools8" in bb else (bb["kpool"][li], bb["vpool"][li])

    def _arena_for(self, pool):
        """The reusable device arena of pages_per_seq pages for pools of this dtype and page shape."""
        key = (pool.dtype, tuple(pool.shape[1:]))
        a = self._arena.get(key)
        if a is None or a.device != pool.device or a.shape[0] != self.bb["pages_per_seq"]:
            a = self._arena[key] = torch.empty((self.bb["pages_per_seq"],) + key[1], dtype=pool.dtype, device=pool.device)
        return a

    def _grow(self):
        """Growth and preemption before a step.  Returns whether a request was preempted."""
        bb, dec = self.bb, self.dec
        live = {r.order: r for r in self.slots if r is not None}
        grants, victims = plan_growth([(o, len(r.pages), rows_next(r.S, len(r.tokens), dec.max_seq_len)) for o, r in live.items()],
                                      bb["pool"].n_free)
        for o in victims:
            self._swap_out(live[o])
        for o, n in grants:                     # the new page into the request's table row: one small H2D copy, the graphs replay untouched
            r = live[o]
            r.pages = r.pages + bb["pool"].alloc(n)
            dec._set_table_rows(r.slot, [table_row(r.pages, bb["pages_per_seq"])])
        return bool(victims)

    def _swap_out(self, r):
        """Preempt r: its pages, layer by layer and pool by pool, through the arena into pinned host tensors kept on the request; its logits
        row; its table row parked, its pages and slot freed.  Everything is enqueued on the current stream: stream order is the only
        synchronisation, and whoever gets the pages next writes them later on the same stream."""
        from . import ops
        bb, dec = self.bb, self.dec
        n = len(r.pages)
        ids = torch.tensor(r.pages, dtype=torch.int32).to(dec._dev)
        pinned = dec._dev.type == "cuda"
        saved = []
        for li in range(dec.n_layers):
            for pool in self._pools_of(li):
                arena = self._arena_for(pool)
                ops.kv_pages_move(pool, arena, ids, True)
                host = torch.empty((n,) + tuple(pool.shape[1:]), dtype=pool.dtype, pin_memory=pinned)
                host.copy_(arena[:n], non_blocking=True)
                saved.append(host)
        r.swap = (saved, bb["logits"][r.slot].clone())
        bb["pool"].free(r.pages)
        dec._set_table_rows(r.slot, [parked_row(bb["pages_per_seq"])])
        self.slots[r.slot] = None
        r.slot, r.pages = None, None
        self.swapped.append(r)
        self.swapped = collections.deque(sorted(self.swapped, key=lambda q: q.order))
        self.preemptions += 1

    def _swap_in(self, r, slot):
        """Resume r in `slot` on the pages r.pages (already in the slot's table row): the saved pages back into the first of them, the logits
        row restored; the pinned buffers are released."""
        from . import ops
        bb, dec = self.bb, self.dec
        saved, logits = r.swap
        n = saved[0].shape[0]
        ids = torch.tensor(r.pages[:n], dtype=torch.int32).to(dec._dev)
        it = iter(saved)
        for li in range(dec.n_layers):
            for pool in self._pools_of(li):
                arena = self._arena_for(pool)
                arena[:n].copy_(next(it), non_blocking=True)
                ops.kv_pages_move(pool, arena, ids, False)
        bb["logits"][slot].copy_(logits)
        bb["pos"][slot:slot + 1].fill_(self._pos(r))
        r.swap = None
        self.resumes += 1

    def _admit_grow(self):
        """Admission under reserve="grow": the swapped requests first (oldest first), then the waiting ones, strict FIFO over both."""
        bb, dec = self.bb, self.dec
        queue = list(self.swapped) + list(self.waiting)
        needs = [pages_for(rows_next(r.S, len(r.tokens), dec.max_seq_len)) for r in queue]
        free = [s for s, r in enumerate(self.slots) if r is None]
        take = admit_grow(needs, len(free), bb["pool"].n_free, self.max_slots - len(free))
        for r, need, slot in zip(queue[:take], needs, free):
            (self.swapped if r.swap is not None else self.waiting).popleft()
            r.pages = bb["pool"].alloc(need)
            dec._set_table_rows(slot, [table_row(r.pages, bb["pages_per_seq"])])
            if r.swap is not None:
                self._swap_in(r, slot)
            else:
                r.order = next(self._orders)
                dec.prefill_slot(slot, r.x, bb["logits"][slot])
                bb["pos"][slot:slot + 1].fill_(r.S)
                r.x = None
            T, k, p = r.sampler if r.sampler is not None else (0.0, 0, 1.0)
            bb["samp_T"][slot:slot + 1].fill_(T); bb["samp_k"][slot:slot + 1].fill_(k); bb["samp_p"][slot:slot + 1].fill_(p)
            bb["sstep"][slot:slot + 1].fill_(len(r.tokens))            # a sampled request has drawn one number per token
            if r.u is not None:                  # kept on the request: a resumed one fills another slot's row with it
                bb["u"][slot, :r.u.numel()].copy_(r.u)
            r.slot = slot
            self.slots[slot] = r

    def _admit(self):
        bb, dec = self.bb, self.dec
        paged = dec.paged_kv
        h = self._prefix
        if paged:                # strict FIFO on whole reservations: how many requests from the head of the queue join in this step
            free = sum(r is None for r in self.slots)
            take = admit_fifo([r.need for r in self.waiting], free, bb["pool"].n_free)
        for slot in range(self.max_slots):
            if not self.waiting or (paged and take == 0):
                return
            if self.slots[slot] is not None:
                continue
            r = self.waiting.popleft()
            if paged:            # its pages into the slot's table row (one small H2D copy; the rest of the row is -1), before its prefill's rows go there
                take -= 1
                r.pages = bb["pool"].alloc(r.need)
                dec._set_table_rows(slot, [table_row((h.pages if h is not None else []) + r.pages, bb["pages_per_seq"])])
            if h is not None:    # tail ++ suffix on top of the shared rows of the single-sequence cache, then its rows into the own pages
                Pf = h.shared_rows
                if dec.cache_epoch != h.epoch:           # someone else used the single-sequence cache: its rows [0, Pf) come back from the pages
                    dec._prefix_rows_from_pages(slot, 0, Pf)
                dec.pos = Pf
                dec.extend(r.x, start_pos=Pf, logits_out=bb["logits"][slot])
                dec._prefix_rows_to_pages(slot, Pf, Pf + r.x.shape[0])
                dec.pos = Pf
                h.epoch = dec.cache_epoch
                bb["pos"][slot:slot + 1].fill_(Pf + r.x.shape[0])
            else:
                dec.prefill_slot(slot, r.x, bb["logits"][slot])                   # rows [0, S) of the slot's cache (fp8 KV: quantised from the staging cache)
                bb["pos"][slot:slot + 1].fill_(r.x.shape[0])
            T, k, p = r.sampler if r.sampler is not None else (0.0, 0, 1.0)                # temperature 0: a greedy slot
            bb["samp_T"][slot:slot + 1].fill_(T); bb["samp_k"][slot:slot + 1].fill_(k); bb["samp_p"][slot:slot + 1].fill_(p)
            bb["sstep"][slot:slot + 1].zero_()
            if r.u is not None:
                bb["u"][slot, :r.u.numel()].copy_(r.u)
            r.slot, r.x, r.u = slot, None, None
            self.slots[slot] = r

    # ---- one decode step for everything in flight
    @torch.no_grad()
    def step(self):
        """Admit, run one step, retire.  Returns {request id: new token} for the requests that produced a token."""
        self.dec._ensure_batch(self.max_slots, owner=self)     # raises if ANOTHER batcher owns the slots with requests in flight
        self.dec._bb_busy = self                               # from here on generate_batch / a second batcher are refused while we hold requests
        if self.dec._bb is not self.bb:       # the slot buffers (and caches) were reallocated: a larger generate_batch() on this decoder, enable_fp8_kv
            if self._prefix is not None:      # its pages went with the pool
                self._prefix.open, self._prefix = False, None
                raise RuntimeError("the decoder's batch buffers were reallocated while a prefix was open: its pages are gone; open_prefix() "
                                   "again and resubmit")
            if any(r is not None for r in self.slots):
                raise RuntimeError("the decoder's batch buffers were reallocated while requests were in flight: use one batcher per decoder "
                                   "and do not call generate_batch() with more sequences than max_slots on it")
            self.bb = self.dec._bb            # no slot is occupied, so no request's rows were lost: go on in the new buffers
        if self.reserve == "grow":
            if not self.dec.paged_kv:
                raise RuntimeError("reserve=\"grow\": the decoder's paged KV cache was switched off under this batcher")
            if not self._grow():              # (no admission in a step that preempted)
                self._admit_grow()
        else:
            self._admit()
        occupied = [s for s, r in enumerate(self.slots) if r is not None]
        if not occupied:
            return {}
        bb, dec = self.bb, self.dec
        nb = occupied[-1] + 1
        holes = [s for s in range(nb) if self.slots[s] is None]
        h = self._prefix
        if holes:            # an empty slot below the highest occupied one still computes (and is ignored): park it at position 0, greedy
            idx = torch.tensor(holes, device=bb["pos"].device)
            bb["pos"][idx] = 0 if h is None else h.shared_rows     # a resident prefix: behind its shared rows, on row 0 of the parking page
            bb["samp_T"][idx] = 0.0
        sampled = any(self.slots[s].sampler is not None for s in occupied)
        attend, mode = (None, ()) if h is None else (dec._paged_prefix_attend(h, nb), ("prefix", h.shared_rows))
        if self.use_graph:
            dec.capture_batch_graph(nb, sampled, attend, mode).replay()     # the draws of every slot's logits + the forward of the new tokens
        else:
            dec._batched_step(nb, sampled, None, attend)
        self.steps += 1
        toks = bb["tok"][:nb].tolist()                    # one small D2H per step for the stop checks (as HF's loop does)
        out = {}
        for s in occupied:
            r = self.slots[s]
            t = int(toks[s])
            r.tokens.append(t)
            out[r.rid] = t
            if r.streamer is not None:
                r.streamer.put(torch.tensor([[t]], dtype=torch.long))
            stop = t in self.eos or len(r.tokens) >= r.max_new
            if not stop and r.criteria is not None:
                ids = torch.tensor([r.tokens], dtype=torch.long)
                stop = any(bool(c(ids, None)) for c in r.criteria)
            if stop:
                self._retire(s)
        return out

    def _retire(self, slot):
        r = self.slots[slot]
        r.done = True
        if r.streamer is not None:
            r.streamer.end()
        self.finished[r.rid] = torch.tensor(r.tokens, dtype=torch.long, device=self.dec._dev)
        self.slots[slot] = None
        if r.pages is not None:          # paged KV: the pages go back to the pool (dirty: whoever gets them overwrites what it reads) and the
            self.bb["pool"].free(r.pages)            # slot's row points at the parking page again
            r.pages = None
            pps, h = self.bb["pages_per_seq"], self._prefix
            self.dec._set_table_rows(slot, [parked_row(pps) if h is None else prefix_parked_row(h.pages, pps)])

    def in_flight(self):
        return sum(r is not None for r in self.slots) + len(self.waiting) + len(self.swapped)

    def run(self):
        """Step until nothing is waiting or in flight.  Returns {request id: LongTensor [n_new]} of everything finished so far."""
        while self.in_flight():
            self.step()
        return self.finished


class ModelBatcher:
    """The same loop one level up: requests are (input_ids, images) pairs exactly as `VideoLLaMA2Hip.generate(inputs, images=)`
    takes them; the video is encoded and spliced at submission, the decode steps are shared."""

    def __init__(self, model, max_slots=4, eos_token_id=None, use_graph=None, reserve="whole"):
        self.model = model
        self.inner = ContinuousBatcher(model.decoder, max_slots, eos_token_id, use_graph, reserve)

    @torch.no_grad()
    def open_video(self, input_ids_prefix, images):
        """One video, many questions arriving over time: input_ids_prefix (the token ids every question begins with, modal sentinels
        included) and its media are encoded ONCE, spliced as `generate_shared` splices its common prefix, and made resident
        (`ContinuousBatcher.open_prefix`).  Returns the handle `submit(input_ids, prefix=handle)` takes."""
        from .model import MODAL_INDEX_MAP
        self.inner._open_prefix_refusals()                   # before the encoder or any other kernel runs
        ids_l = (input_ids_prefix[0] if input_ids_prefix.dim() == 2 else input_ids_prefix).tolist()
        n_sent = sum(1 for t in ids_l if t in set(MODAL_INDEX_MAP.values()))
        media = list(images) if images is not None else []
        if n_sent != len(media):
            raise ValueError(f"open_video: the prefix holds {n_sent} modal sentinels for {len(media)} media")
        feats = []
        if n_sent:
            f = self.model.encode_images_or_videos(media)
            feats = [f[k] for k in range(n_sent)]
        h = self.inner.open_prefix(self.model._embed_suffix(ids_l, feats, 0))
        h.ids = ids_l
        return h

    def close_video(self):
        self.inner.close_prefix()

    def _embed_behind(self, h, input_ids, images):
        """The embedding rows of a question behind the resident prefix h: its ids must begin with the prefix's and bring no media of their own."""
        from .model import MODAL_INDEX_MAP
        if not isinstance(h, PrefixHandle) or h.ids is None:
            raise ValueError("submit: prefix must be the handle open_video returned")
        if h is not self.inner._prefix:
            raise ValueError("submit: the prefix handle is closed or was opened on another batcher")
        ids_l = (input_ids[0] if input_ids.dim() == 2 else input_ids).tolist()
        t = len(h.ids)
        if ids_l[:t] != h.ids or len(ids_l) <= t:
            raise ValueError(f"submit: the request's ids must begin with the open prefix's {t} ids and add at least one of their own")
        if images is not None or any(tok in set(MODAL_INDEX_MAP.values()) for tok in ids_l[t:]):
            raise ValueError("submit: a request behind an open prefix brings no media of its own (a modal sentinel follows the prefix's ids, or "
                             "images were passed)")
        emb = torch.empty((len(ids_l) - t, self.model.decoder.D), dtype=_lib.elem_dtype(), device=self.model._dev)
        self.model._embed_ids(torch.tensor(ids_l[t:], dtype=torch.int64).to(self.model._dev), emb)
        return emb

    @torch.no_grad()
    def submit(self, input_ids, images=None, attention_mask=None, prefix=None, **kw):
        """Queue one request; the keywords are ContinuousBatcher.submit's, and unspecified sampling settings come from the model's
        generation_config as in `VideoLLaMA2Hip.generate(do_sample=True)`.  prefix=handle (`open_video`): input_ids begin with the
        prefix's ids; only the rest is embedded, and the video is not encoded again."""
        from .model import UNBUILT_WARPERS, resolve_sampler
        sampler = resolve_sampler(kw, getattr(self.model, "generation_config", None))
        for k in ("do_sample", "temperature", "top_k", "top_p", "generator") + tuple(k for k, _ in UNBUILT_WARPERS):
            kw.pop(k, None)
        if sampler is not None:
            kw.update(do_sample=True, temperature=sampler[0], top_k=sampler[1], top_p=sampler[2], generator=sampler[3])
        if prefix is not None:
            return self.inner.submit(self._embed_behind(prefix, input_ids, images), prefix=prefix, **kw)
        ids = input_ids if input_ids.dim() == 2 else input_ids[None]
        emb, lens = self.model._inputs_embeds(ids, attention_mask, images)
        return self.inner.submit(emb[0, :lens[0]], **kw)

    def step(self):
        return self.inner.step()

    def run(self):
        return self.inner.run()

    def in_flight(self):
        return self.inner.in_flight()

    @property
    def finished(self):
        return self.inner.finished
