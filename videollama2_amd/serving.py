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

from .decoder import eos_set
from .paging import admit_fifo, pages_needed, parked_row, table_row


class _Request:
    __slots__ = ("rid", "x", "max_new", "streamer", "criteria", "tokens", "slot", "done", "sampler", "u", "need", "pages")

    def __init__(self, rid, x, max_new, streamer, criteria, sampler=None, u=None):
        self.rid, self.x, self.max_new, self.streamer, self.criteria = rid, x, max_new, streamer, criteria
        self.sampler, self.u = sampler, u              # (temperature, top_k, top_p) and the request's uniform numbers, or None: greedy
        self.tokens, self.slot, self.done = [], None, False
        self.need, self.pages = 0, None                # paged KV: the reservation (pages) and, once admitted, the page ids


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
    refused at `submit`.  Not built: growing a reservation page by page, preemption.  The decoder refuses the switch with requests in flight."""

    def __init__(self, decoder, max_slots=4, eos_token_id=None, use_graph=None):
        if decoder.tp > 1:
            raise NotImplementedError("continuous batching is built for the single-GPU decoder")
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

    # ---- admission
    def submit(self, inputs_embeds, max_new_tokens=2048, streamer=None, stopping_criteria=None, do_sample=False, temperature=None, top_k=None,
               top_p=None, generator=None, **warpers):
        """Queue one request (inputs_embeds [S, D]: the spliced prompt of `prepare_inputs_labels_for_multimodal`).  It is prefilled
        and joins the batch at the next `step()` with a free slot.  Returns the request id.
        do_sample=True: HF `_sample` with the warpers temperature -> top_k -> top_p, HF's defaults (1.0, 50, 1.0) for the unspecified ones and
        HF's checks, as `VideoLLaMA2Hip.generate(do_sample=True)`; other warpers (`repetition_penalty`, ...) are refused unless neutral.  The
        request's uniform numbers are drawn here from `generator` (or torch's generator for the device), as many and in the same call as a solo
        `HipMistralDecoder.generate(sampler=...)` of this request draws them, so it samples the same tokens under the same seed."""
        from .model import UNBUILT_WARPERS, resolve_sampler
        unknown = set(warpers) - {k for k, _ in UNBUILT_WARPERS}
        if unknown:
            raise TypeError(f"submit() got unexpected keyword arguments {sorted(unknown)}")
        given = dict(temperature=temperature, top_k=top_k, top_p=top_p, **warpers)
        sampler = resolve_sampler(dict({k: v for k, v in given.items() if v is not None}, do_sample=do_sample, generator=generator))
        S = inputs_embeds.shape[0]
        if S > self.dec.max_seq_len:
            raise ValueError(f"sequence length {S} exceeds the KV cache ({self.dec.max_seq_len})")
        crit = stopping_criteria
        if crit is not None and not isinstance(crit, (list, tuple)):
            crit = [crit]
        max_new = min(int(max_new_tokens), self.dec.max_seq_len - S + 1)
        need = 0
        if self.dec.paged_kv:            # its whole reservation; one that the pool can never hold would block the queue for ever
            need = pages_needed(S, max_new, self.dec.max_seq_len)
            if need > self.dec._n_pages - 1:
                raise ValueError(f"paged KV cache: the request needs {need} pages ({S} prompt rows + {max_new} new tokens), the pool serves "
                                 f"{self.dec._n_pages - 1} (enable_paged_kv(n_pages); page 0 is the parking page)")
        u = None
        if sampler is not None:
            u = torch.rand((max_new,), device=self.dec._dev, generator=sampler[3])
            sampler = sampler[:3]
        r = _Request(next(self._ids), inputs_embeds, max_new, streamer, crit, sampler, u)
        r.need = need
        self.waiting.append(r)
        return r.rid

    def _admit(self):
        bb, dec = self.bb, self.dec
        paged = dec.paged_kv
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
                dec._set_table_rows(slot, [table_row(r.pages, bb["pages_per_seq"])])
            dec.prefill_slot(slot, r.x, bb["logits"][slot])                       # rows [0, S) of the slot's cache (fp8 KV: quantised from the staging cache)
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
            if any(r is not None for r in self.slots):
                raise RuntimeError("the decoder's batch buffers were reallocated while requests were in flight: use one batcher per decoder "
                                   "and do not call generate_batch() with more sequences than max_slots on it")
            self.bb = self.dec._bb            # no slot is occupied, so no request's rows were lost: go on in the new buffers
        self._admit()
        occupied = [s for s, r in enumerate(self.slots) if r is not None]
        if not occupied:
            return {}
        bb, dec = self.bb, self.dec
        nb = occupied[-1] + 1
        holes = [s for s in range(nb) if self.slots[s] is None]
        if holes:            # an empty slot below the highest occupied one still computes (and is ignored): park it at position 0, greedy
            idx = torch.tensor(holes, device=bb["pos"].device)
            bb["pos"][idx] = 0
            bb["samp_T"][idx] = 0.0
        sampled = any(self.slots[s].sampler is not None for s in occupied)
        if self.use_graph:
            dec.capture_batch_graph(nb, sampled).replay()     # the draws of every slot's logits + the forward of the new tokens
        else:
            dec._batched_step(nb, sampled)
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
            self.dec._set_table_rows(slot, [parked_row(self.bb["pages_per_seq"])])

    def in_flight(self):
        return sum(r is not None for r in self.slots) + len(self.waiting)

    def run(self):
        """Step until nothing is waiting or in flight.  Returns {request id: LongTensor [n_new]} of everything finished so far."""
        while self.in_flight():
            self.step()
        return self.finished


class ModelBatcher:
    """The same loop one level up: requests are (input_ids, images) pairs exactly as `VideoLLaMA2Hip.generate(inputs, images=)`
    takes them; the video is encoded and spliced at submission, the decode steps are shared."""

    def __init__(self, model, max_slots=4, eos_token_id=None, use_graph=None):
        self.model = model
        self.inner = ContinuousBatcher(model.decoder, max_slots, eos_token_id, use_graph)

    @torch.no_grad()
    def submit(self, input_ids, images=None, attention_mask=None, **kw):
        """Queue one request; the keywords are ContinuousBatcher.submit's, and unspecified sampling settings come from the model's
        generation_config as in `VideoLLaMA2Hip.generate(do_sample=True)`."""
        from .model import UNBUILT_WARPERS, resolve_sampler
        sampler = resolve_sampler(kw, getattr(self.model, "generation_config", None))
        for k in ("do_sample", "temperature", "top_k", "top_p", "generator") + tuple(k for k, _ in UNBUILT_WARPERS):
            kw.pop(k, None)
        if sampler is not None:
            kw.update(do_sample=True, temperature=sampler[0], top_k=sampler[1], top_p=sampler[2], generator=sampler[3])
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
