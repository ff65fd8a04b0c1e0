"""HipMistralDecoder -- the decoder backend behind `Videollama2MistralForCausalLM.generate(inputs, images=...)`
(videollama2/model/videollama2_mistral.py:110-144) and, with the q/k/v bias HF Qwen2Attention adds, behind
`Videollama2Qwen2ForCausalLM.generate` (videollama2/model/videollama2_qwen2.py:108-142; alias `HipQwen2Decoder`): consumes `inputs_embeds [S, hidden]`, runs the Mistral prefill and
the greedy decode loop on its own KV cache and returns the NEW token ids, as HF `generate` does on the
`inputs_embeds` path.  Per-layer math follows HF:models/mistral/modeling_mistral.py (RMSNorm fp32 statistics,
rotate-half RoPE theta=1e6, causal GQA attention, SwiGLU), executed by libvl2hip.so kernels only."""
import gc

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib, ops
from .paging import PagePool, pages_needed, parked_row, table_row
from .weights import pack_decoder


def eos_set(eos_token_id):
    """The stop ids of a decode loop: `eos_token_id` is None, one id, or a list / tuple / set of ids."""
    if eos_token_id is None:
        return set()
    return set(eos_token_id) if isinstance(eos_token_id, (list, tuple, set)) else {int(eos_token_id)}


# ---------------------------------------------------------------------- projection forms
# A form is the kernel family that projects a layer's activations, picked once per call from the path and the weight format ("16bit" |
# "fp8" | "mxfp4").  The two layer loops (HipMistralDecoder._rows / _tokens) ask it for normed(x, w) = RMSNorm(x) @ w.T (the norm weight
# is folded into w: q/k/v, gate/up), res(a, w, x) = x + a @ w.T (o, down) and, in the token loop, head(x, out) = the fp32 logits.
# `layers` holds the per-layer weights it reads (the 16-bit dicts, or their fp8 / MXFP4 copies as (codes, scales) pairs); lm_head is
# quantised in fp8 only, the MXFP4 forms run the 16-bit one.  16-bit forms under tensor parallelism: the residual rides on rank 0's
# partial sum and the result is all-reduced; the quantised forms are single-rank and issue no all-reduce.
class _Form:
    def __init__(self, dec, fmt="16bit"):
        self.dec, self.fmt = dec, fmt
        w = dec.w if fmt == "16bit" else dec.w8 if fmt == "fp8" else dec.w4
        self.layers, self.lm_head = w["layers"], (dec.w8 if fmt == "fp8" else dec.w)["lm_head"]

    def begin(self, x):
        """The rows loop's prologue: (0, rstd) of x's rows in rn, which the carried norm reads and Mixtral's MoE combine keeps current."""
        self.rs = ops.row_stats(x)
        self.rn = ops.row_norm_finalize(self.rs, self.dec.D, ops.NORM_RMS, self.dec.eps)

    def res(self, a, w, x, out=None):
        if self.fmt != "16bit":
            return self._mm(a, w, res=x, out=out)
        dec = self.dec
        return dec._reduce(self._mm(a, w, res=x if dec.tp_rank == 0 else None, out=out))


class _Tiled(_Form):
    """The tiled MFMA GEMMs with the RMSNorm carried: each residual projection's epilogue emits its rows' statistics, reduced once into rn
    for the next normed GEMM.  Tensor parallel: the GEMM output is a partial sum, so the statistics are taken after the all-reduce."""

    def normed(self, x, w, bias=None, swiglu=False):
        return ops.gemm(x, w, bias=bias, swiglu=swiglu, norm=(ops.NORM_RMS, self.rn, self.dec.eps, None), mfma16=swiglu)

    def res(self, a, w, x):
        dec = self.dec
        if dec.tp > 1:
            x = dec._reduce(ops.gemm(a, w, res=x if dec.tp_rank == 0 else None))
            ops.row_stats(x, out=self.rs)
        else:
            x = ops.gemm(a, w, res=x, stats_out=self.rs)
        ops.row_norm_finalize(self.rs, dec.D, ops.NORM_RMS, dec.eps, out=self.rn)
        return x


class _W8A8(_Form):
    """fp8 weights and fp8 activations, quantised per row on the fly (with the row's RMS for a normed projection)."""

    def __init__(self, dec):
        super().__init__(dec, "fp8")

    def begin(self, x):
        pass

    def normed(self, x, w, bias=None, swiglu=False):
        return ops.gemm_fp8(*ops.quant_act_fp8(x, rms_eps=self.dec.eps), *w, bias=bias, swiglu=swiglu)

    def _mm(self, a, w, **kw):
        return ops.gemm_fp8(*ops.quant_act_fp8(a), *w, **kw)


class _Skinny(_Form):
    """RMSNorm as its own launch, then the skinny-M MFMA kernel: the weights stream once for up to 64 rows (16-bit: the tiled GEMM
    beyond; fp8 / MXFP4: calls of at most 64 rows)."""
    QUANTISED = dict(fp8=ops.gemm_skinny_fp8, mxfp4=ops.gemm_skinny_mxfp4)

    def __init__(self, dec, fmt, rows):
        super().__init__(dec, fmt)
        mm16 = ops.gemm_skinny if rows <= 64 else ops.gemm
        self._mm = mm16 if fmt == "16bit" else (lambda a, w, kern=self.QUANTISED[fmt], **kw: kern(a, *w, **kw))
        self._head = mm16 if fmt == "mxfp4" else self._mm

    def normed(self, x, w, **kw):
        return self._mm(ops.rmsnorm(x, self.dec.w["ones"], self.dec.eps), w, **kw)

    def head(self, x, out):
        return self._head(ops.rmsnorm(x, self.dec.w["norm_w"], self.dec.eps), self.lm_head, out_f32=True, out=out)


class _Gemv(_Form):
    """GEMV with the RMSNorm fused into the kernel (fp8 / MXFP4: plain RMS, the weight folded in), one row or a few (batched: one pass
    over the weights for all rows, each bit for bit the single-row call)."""
    KERNELS = {"16bit": (ops.gemv, ops.gemv_batched), "fp8": (ops.gemv_fp8, ops.gemv_batched_fp8),
               "mxfp4": (ops.gemv_mxfp4, ops.gemv_batched_mxfp4)}

    def __init__(self, dec, fmt, batched):
        super().__init__(dec, fmt)
        self._mv = self.KERNELS[fmt][batched]
        self._head_fmt = "16bit" if fmt == "mxfp4" else fmt
        self._head_mv = self.KERNELS[self._head_fmt][batched]

    def _mm(self, a, w, **kw):
        return self._mv(w, a, **kw) if self.fmt == "16bit" else self._mv(*w, a, **kw)

    def normed(self, x, w, **kw):
        fold = dict(norm_w=self.dec.w["ones"]) if self.fmt == "16bit" else dict(rms_plain=True)
        return self._mm(x, w, eps=self.dec.eps, **fold, **kw)

    def head(self, x, out):
        w = (self.lm_head,) if self._head_fmt == "16bit" else self.lm_head
        return self._head_mv(*w, x, norm_w=self.dec.w["norm_w"], eps=self.dec.eps, out_f32=True, out=out)


class HipMistralDecoder(nn.Module):
    """tp_group: optional torch.distributed group for tensor parallelism over the heads / MLP width (the
    reference has none -- its 72B path is accelerate's device_map="auto").  Every rank holds 1/tp of the q/k/v/gate/up rows
    and of the o/down columns and of the KV cache; the two row-parallel projections of a layer produce partial sums that are
    all-reduced (RCCL over xGMI; 2 x [S, D] bf16 per layer in the prefill, 2 x [D] per layer per token in the decode loop).
    The residual is folded into rank 0's partial so the sum needs no extra pass."""

    def __init__(self, cfg, state_dict, device="cuda", max_seq_len=4096, n_layers=None, tp_group=None, tp_shard=None, tp_local=None):
        super().__init__()
        self.cfg = cfg
        l = cfg["llm"]
        self._dev = torch.device(device)
        self.tp_group = tp_group
        self.tp = dist.get_world_size(tp_group) if tp_group is not None else 1
        self.tp_rank = dist.get_rank(tp_group) if tp_group is not None else 0
        if tp_shard is not None:                 # (rank, size) WITHOUT a group: one rank's shard run alone, no collectives --
            self.tp_rank, self.tp = tp_shard     # timing model only (scripts/tp_model.py); the numbers it produces are partial sums
        # ... unless `tp_local` (dist.LocalTensorParallel) stands in for the group: every rank's shard in ONE process, the all-reduce
        # a rendezvous of host threads -- how >= 2 REAL shards are summed and checked on a 1-GPU box (tests/test_gpu_tp.py)
        self.tp_local = tp_local
        self.w = pack_decoder(state_dict, cfg, self._dev, n_layers, self.tp_rank, self.tp)
        self.n_layers = len(self.w["layers"])
        self.nh, self.nkv, self.hd = l["num_attention_heads"] // self.tp, l["num_key_value_heads"] // self.tp, l["head_dim"]
        self.D, self.V, self.eps = l["hidden_size"], l["vocab_size"], l["rms_norm_eps"]
        self.max_seq_len = max_seq_len
        # RoPE tables, fp32, HF MistralRotaryEmbedding: inv_freq = theta^(-2i/d); cos/sin of pos*inv_freq
        self.cos_t, self.sin_t = self._rope_tables(max_seq_len)
        self._elem = _lib.elem()
        bf = dict(dtype=_lib.elem_dtype(), device=self._dev)
        self.kcache = [torch.zeros((self.nkv, max_seq_len, self.hd), **bf) for _ in range(self.n_layers)]
        self.vcache = [torch.zeros((self.nkv, max_seq_len, self.hd), **bf) for _ in range(self.n_layers)]
        nsplit_max = (max_seq_len + 63) // 64
        self.partial = torch.empty((self.nh * nsplit_max * 130,), dtype=torch.float32, device=self._dev)
        # decode-step state lives on the device so that one captured hipGraph replays for every token:
        #   tok = current token id, state = {position of the token being fed, step index}, hist = generated ids
        self.tok = torch.zeros((1,), dtype=torch.int32, device=self._dev)
        self.state = torch.zeros((2,), dtype=torch.int32, device=self._dev)
        self.hist = torch.zeros((max_seq_len,), dtype=torch.int32, device=self._dev)
        I = l["intermediate_size"] // self.tp
        self._b = dict(x0=torch.empty((1, self.D), **bf), qkv=torch.empty(((self.nh + 2 * self.nkv) * self.hd,), **bf),
                       o=torch.empty((self.nh * self.hd,), **bf), x1=torch.empty((self.D,), **bf),
                       a=torch.empty((I,), **bf))
        self.logits = torch.empty((self.V,), dtype=torch.float32, device=self._dev)
        self.graph = None
        self.pos = 0
        # bumped by every call that rewrites the own KV cache (prefill, prefill_batch into it, extend) or changes the arithmetic of the
        # rows a later call would append (fp8 toggles): a caller that recorded it can tell whether the rows it left are still there
        self.cache_epoch = 0
        self._stage = None                  # (vl2_llm_desc, keepalive, decode workspace): prefill / decode step as ONE C call each
        # validation hook for 1-GPU boxes: issue the tensor-parallel all-reduces even when the group has ONE rank (the sum over one
        # rank is the identity), so that the captured-RCCL decode graph can be exercised on hardware without a second GPU
        self.tp_always_reduce = False
        self.decode_fp8 = self.prefill_fp8 = self.decode_mxfp4 = False
        self._fp8_kv, self.kv8 = False, None        # enable_fp8_kv: per layer (k8, v8, ks, vs), the single-sequence fp8 KV cache
        self._paged_kv, self._n_pages = False, 0    # enable_paged_kv: the batched paths keep their slots' rows in pages of a shared pool
        self._paged_fp8 = False                     # enable_paged_kv(fp8=True): those pages hold fp8 rows (codes + row scales)

    def _rope_tables(self, rows):
        """cos / sin of pos * inv_freq for positions 0 .. rows-1, fp32 [rows, head_dim / 2] on the device."""
        inv = 1.0 / (self.cfg["llm"]["rope_theta"] ** (torch.arange(0, self.hd, 2, dtype=torch.int64).float() / self.hd))
        fr = torch.arange(rows, dtype=torch.float32)[:, None] * inv[None, :]
        return fr.cos().contiguous().to(self._dev), fr.sin().contiguous().to(self._dev)

    def _step_buffers(self, B, u_cols):
        """Activations, logits, tokens, positions and per-slot draw settings of a batched decode step for B slots (u: u_cols uniform
        numbers per slot; temperature 0 = greedy; slot b draws at u[b, sstep[b]])."""
        bf = dict(dtype=_lib.elem_dtype(), device=self._dev)
        I = self.cfg["llm"]["intermediate_size"] // self.tp
        return dict(
            x0=torch.empty((B, self.D), **bf), x1=torch.empty((B, self.D), **bf), qkv=torch.empty((B, (self.nh + 2 * self.nkv) * self.hd), **bf),
            o=torch.empty((B, self.nh * self.hd), **bf), a=torch.empty((B, I), **bf),
            logits=torch.empty((B, self.V), dtype=torch.float32, device=self._dev),
            tok=torch.zeros((B,), dtype=torch.int32, device=self._dev), pos=torch.zeros((B,), dtype=torch.int32, device=self._dev),
            samp_T=torch.zeros((B,), dtype=torch.float32, device=self._dev), samp_k=torch.zeros((B,), dtype=torch.int32, device=self._dev),
            samp_p=torch.ones((B,), dtype=torch.float32, device=self._dev), u=torch.zeros((B, u_cols), dtype=torch.float32, device=self._dev),
            sstep=torch.zeros((B,), dtype=torch.int32, device=self._dev))

    @property
    def decode_format(self):
        """The weight format of the decode step's projections: "16bit" | "fp8" | "mxfp4"."""
        return "mxfp4" if self.decode_mxfp4 else "fp8" if self.decode_fp8 else "16bit"

    @torch.no_grad()
    def enable_fp8_decode(self, on=True):
        """OPTIONAL arithmetic (the fp8 half of BASELINE.json configs[4]): the decode step's projections stream fp8
        (OCP e4m3fn) copies of the packed weights with one power-of-two scale per output row (csrc/k_fp8.h; activations stay 16-bit).
        Prefill keeps the 16-bit weights (it is MFMA-bound, decode is bound by the weight stream).  The copies are made once, here
        (+7.2 GB for the 7B model).  Not the reference's arithmetic and never the default: oracle/fp8_oracle.py defines the quantiser."""
        if self.tp > 1:
            raise NotImplementedError("fp8 decode weights: single-rank decoders only")
        if on and self.decode_mxfp4:
            raise ValueError("MXFP4 decode weights are on: call enable_mxfp4_decode(False) before enable_fp8_decode()")
        if on and getattr(self, "w8", None) is None:
            self._make_w8()
        self.decode_fp8 = bool(on)
        self._invalidate_graphs()                                 # a captured step (greedy or sampled) holds the other projections
        self.cache_epoch += 1
        return self

    @torch.no_grad()
    def enable_mxfp4_decode(self, on=True):
        """OPTIONAL arithmetic: the decode step's projections stream MXFP4 copies of the packed weights (OCP Microscaling Formats v1.0: E2M1
        elements, one E8M0 power-of-two scale per block of 32 k, 4.25 bits per weight; csrc/k_mxfp4.h; activations stay 16-bit).  Copies of
        wqkv / wo / wgu / wd of every layer are made once, here, from the packed weights (self.w4, +1.8 GB for the 7B model).  lm_head STAYS
        16-bit: its error lands on the logits directly and it is 0.26 GB of a 4 GB stream.  Prefill, extend, attention, RoPE, the KV cache
        and the embedding stay 16-bit too (the fp8 prefill may be on beside it).  The single-token step then runs operator by operator (it is
        replayed from a hipGraph anyway; the stage call knows no MXFP4).  Not the reference's arithmetic and never the default: the format
        costs about 11 % rel-L2 per projection; tests/mxfp4_oracle.py defines the quantiser."""
        if self.tp > 1:
            raise NotImplementedError("MXFP4 decode weights: single-rank decoders only")
        if on and self.decode_fp8:
            raise ValueError("fp8 decode weights are on: call enable_fp8_decode(False) before enable_mxfp4_decode()")
        if on and getattr(self, "w4", None) is None:
            self.w4 = dict(layers=[{k: ops.quant_mxfp4(lw[k]) for k in ("wqkv", "wo", "wgu", "wd")} for lw in self.w["layers"]])
        self.decode_mxfp4 = bool(on)
        self._invalidate_graphs()                                 # a captured step holds the other projections
        self.cache_epoch += 1
        return self

    FP8_KV_EXTEND_MSG = ("the fp8 KV cache is on: extend / generate(prefix_cache=True) are not built on it (the answer's rows exist only in "
                         "fp8 and the append attention reads 16-bit rows): call enable_fp8_kv(False) first, or prefill the whole prompt")

    @property
    def fp8_kv(self):
        """Whether the decode steps keep and read the KV cache in fp8 (enable_fp8_kv)."""
        return self._fp8_kv

    def _fp8_kv_refusals(self):
        if self.tp > 1 or self.tp_group is not None or self.tp_local is not None or self.tp_always_reduce:
            raise NotImplementedError("fp8 KV cache: single-rank decoders only (no tensor-parallel shard's cache is built in fp8): build the "
                                      "decoder without a tensor-parallel group, or keep the 16-bit cache")
        if self.hd != 128:
            raise NotImplementedError(f"fp8 KV cache: head_dim 128 only (this decoder has {self.hd}): keep the 16-bit cache")

    @torch.no_grad()
    def enable_fp8_kv(self, on=True):
        """OPTIONAL arithmetic: the decode steps keep the KV cache in fp8 (OCP e4m3fn codes with one power-of-two scale per (kv head,
        position) row of 128 elements, K and V apart; csrc/k_kv8.h) -- half the attention's bytes per step and 0.52 x
        the slots' memory.  Orthogonal to `decode_format`: 16-bit, fp8 and MXFP4 decode weights all run on it.  The 16-bit cache stays as
        the prefill's staging cache: `prefill` is unchanged (same bits, its attention reads the 16-bit rows), its rows are then quantised
        once, and `decode_step` / `capture_graph` / `generate` attend on the fp8 cache alone, the new token's rows quantised on their way in
        (the step runs operator by operator: the stage call has no form for it).  The batched paths (`generate_batch`, ContinuousBatcher)
        hold their slots in fp8 only and prefill through one 16-bit staging cache.  Switching drops every captured graph and the slot
        buffers and resets the single-sequence state (pos = 0, a new cache_epoch); it is refused while a batcher holds requests in flight.
        While it is on the decoder holds both single-sequence caches (+0.52 x the 16-bit one); switching it off frees the fp8 one.
        `extend` / prefix reuse, tensor parallelism, Mixtral and head_dim != 128 raise NotImplementedError.  Not the reference's
        arithmetic and never the default: with it off every path keeps its bits; tests/fp8kv_oracle.py defines the format."""
        if on:
            self._fp8_kv_refusals()
        # (whatever its pages hold: fp8 pages are entered through enable_paged_kv(fp8=True) alone.  Under fp8 pages the words "16-bit rows" are
        # not true; the message is kept word for word because tests/test_paged_kv_host.py and tests/test_paged_prefix_host.py pin it)
        if on and getattr(self, "_paged_kv", False):
            raise NotImplementedError("fp8 KV cache: the paged KV cache is on (its pages hold 16-bit rows): call enable_paged_kv(0, False) first")
        busy = getattr(self, "_bb_busy", None)
        if busy is not None and busy.in_flight():
            raise RuntimeError("enable_fp8_kv: a ContinuousBatcher holds requests in flight on this decoder's slots, whose caches would change "
                               "format under them: drain it (run()) first")
        if on and self.kv8 is None:
            self.kv8 = [ops.kv8_alloc((), self.nkv, self.max_seq_len, self._dev) for _ in range(self.n_layers)]
        if not on:
            self.kv8 = None                          # freed with the switch (allocated again by the next enable)
        self._fp8_kv = bool(on)
        self._invalidate_graphs()
        self._bb = None                              # the slot caches are in the other format: the next batched call allocates them again
        self.pos = 0
        self.cache_epoch += 1
        return self

    def _quant_rows(self, kcache, vcache, kv8, n):
        """Rows [0, n) of every layer's 16-bit caches (a prefill's) -> the fp8 caches kv8 (per layer (k8, v8, ks, vs))."""
        for li in range(self.n_layers):
            ops.kv_quant(kcache[li], vcache[li], kv8[li], 0, n)

    # ------------------------------------------------------------------ paged KV cache of the batched paths
    @property
    def paged_kv(self):
        """Whether the batched paths keep their slots' KV rows in pages of a shared pool (enable_paged_kv)."""
        return self._paged_kv

    @property
    def paged_kv_fp8(self):
        """Whether the pages of the paged KV cache hold fp8 rows (enable_paged_kv(n_pages, fp8=True))."""
        return self._paged_kv and self._paged_fp8

    def kv_page_bytes(self):
        """Bytes of ONE page over all layers, K and V: n_layers * 2 * nkv * 64 * 128 * 2 (8.39 MB at 7B; 64 pages = a 4096-row slot); while
        fp8 pages are on, n_layers * 2 * nkv * 64 * (128 + 4): a code per element and a scale per row (4.33 MB at 7B)."""
        if self.paged_kv_fp8:
            return self.n_layers * 2 * self.nkv * ops.KV_PAGE_ROWS * (128 + 4)
        return self.n_layers * 2 * self.nkv * ops.KV_PAGE_ROWS * 128 * 2

    def _paged_kv_refusals(self):
        if self.tp > 1 or self.tp_group is not None or self.tp_local is not None or self.tp_always_reduce:
            raise NotImplementedError("paged KV cache: single-rank decoders only (no tensor-parallel shard's slots are built on pages): build "
                                      "the decoder without a tensor-parallel group, or keep the contiguous slots")
        if self.hd != 128:
            raise NotImplementedError(f"paged KV cache: head_dim 128 only (this decoder has {self.hd}): keep the contiguous slots")
        if self._fp8_kv:
            raise NotImplementedError("paged KV cache: the fp8 KV cache is on (the pages hold 16-bit rows): call enable_fp8_kv(False) first")

    @torch.no_grad()
    def enable_paged_kv(self, n_pages, on=True, fp8=False):
        """OPTIONAL layout, never the default: the batched paths (`generate_batch`, ContinuousBatcher) keep their slots' 16-bit KV rows in
        PAGES of 64 positions drawn from one pool of `n_pages` pages per layer (csrc/k_attn_paged.h) instead of a
        private cache of max_seq_len rows per slot: a request holds ceil(min(S + max_new, max_seq_len) / 64) pages, `kv_page_bytes()` each,
        whatever max_seq_len is.  Page 0 is the parking page of the slots that hold no request, so n_pages - 1 pages serve requests.  It
        changes where rows live and not one sum: every batched result is bit for bit the contiguous slots' (with it off every path keeps
        its bits and its launches).  A request is prefilled into one 16-bit staging cache (the unchanged `prefill`) and its rows are copied
        into its pages.  Switching drops every captured batch graph and the slot buffers; it is refused while a batcher holds requests in
        flight.  The single-sequence paths (`generate`, `extend`, the prefix cache) keep their contiguous cache and are untouched.
        Tensor parallelism, head_dim != 128, Mixtral, the fp8 KV cache (each switch refuses the other) and
        `generate_batch(shared_prefix=...)` raise NotImplementedError.  Growing a reservation page by page and preemption by swap:
        `ContinuousBatcher(reserve="grow")`; `generate_batch` keeps reserving up front.
        fp8=True (csrc/k_attn_paged_kv8.h): the pages hold the rows of the fp8 KV cache -- e4m3fn codes and one
        power-of-two scale per (kv head, row), `enable_fp8_kv`'s format -- so a page is `kv_page_bytes()` = 0.52 x the 16-bit page and every
        batched result is bit for bit that of contiguous fp8-KV slots (a decoder with `enable_fp8_kv()`): the staging rows are quantised into
        the pages, the step appends and reads codes and scales.  It is the only way into the combination: `fp8_kv` stays off (the
        single-sequence cache is never paged and keeps its 16-bit bits), the two switches still refuse each other, and a resident prefix
        (`ContinuousBatcher.open_prefix`) is refused on fp8 pages.  Switching the page format drops the slot buffers and the graphs like
        any other call."""
        if on:
            self._paged_kv_refusals()
            if int(n_pages) < 2:
                raise ValueError(f"enable_paged_kv: n_pages {n_pages}: page 0 is the parking page, a request needs at least one more")
        busy = getattr(self, "_bb_busy", None)
        if busy is not None and busy.in_flight():
            raise RuntimeError("enable_paged_kv: a ContinuousBatcher holds requests in flight on this decoder's slots, whose rows would change "
                               "layout under them: drain it (run()) first")
        self._paged_kv, self._n_pages = bool(on), int(n_pages) if on else 0
        self._paged_fp8 = bool(on and fp8)
        self._invalidate_graphs()
        self._bb = None                              # the slots are in the other layout: the next batched call allocates them again
        return self

    def _set_table_rows(self, slot0, rows):
        """Rows slot0 .. of the device page table <- `rows` (lists of pages_per_seq ids each): one small H2D copy."""
        self._bb["table"][slot0:slot0 + len(rows)].copy_(torch.tensor(rows, dtype=torch.int32))

    def _make_w8(self):
        """The fp8 copies of the packed projections (shared by the decode and the prefill switch).  The stage descriptor is rebuilt with
        the fp8 pointers -- and with it the decode workspace, so every captured graph (which points into the old workspace) goes too."""
        self.w8 = dict(layers=[{k: ops.quant_fp8(lw[k]) for k in ("wqkv", "wo", "wgu", "wd")} for lw in self.w["layers"]],
                       lm_head=ops.quant_fp8(self.w["lm_head"]))
        self._stage = None
        self._invalidate_graphs()

    def _invalidate_graphs(self):
        """Drop every captured decode graph: the greedy one and the sampled one (keyed by the sampler only) both bake in the weight
        pointers / arithmetic (`decode_format`) and the stage workspace of the moment they were captured; so do the batched steps' graphs
        (capture_batch_graph), which the next step captures again on the weights then selected."""
        self.graph = None
        self._graph_sample = (None, None)
        self.__dict__.get("_batch_graphs", {}).clear()

    @torch.no_grad()
    def enable_fp8_prefill(self, on=True):
        """OPTIONAL arithmetic (BASELINE.json configs[4] "fp8 MFMA on CDNA4"): the four projections of every layer of the
        PREFILL run on the fp8 matrix pipe (v_mfma_f32_32x32x64_f8f6f4, twice the 16-bit MFMA rate and half the operand bytes): weights = the
        row-scaled e4m3fn copies of enable_fp8_decode, activations quantised per token row on the fly (W8A8; csrc/k_fp8.h quant_act_fp8_kernel,
        k_gemm.h gemm3 / gemm4 FP8).  Attention, RoPE, the KV cache and lm_head stay 16-bit.  Not the reference's arithmetic, never the
        default: oracle/fp8_oracle.py (gemm_w8a8) defines it."""
        if self.tp > 1:
            raise NotImplementedError("fp8 prefill: single-rank decoders only")
        if on and getattr(self, "w8", None) is None:
            self._make_w8()
        self.prefill_fp8 = bool(on)
        self.cache_epoch += 1
        return self

    def _stage_desc(self):
        if self._stage is None:
            d, keep = ops.llm_desc(self.w, self.cfg["llm"], self.nh, self.nkv, self.max_seq_len, self.eps, self.kcache, self.vcache,
                                   self.cos_t, self.sin_t, w8=getattr(self, "w8", None))
            ws, _ = ops._llm_ws(d, 1, self._dev)
            self._stage = (d, keep, ws)
        return self._stage

    def _use_stage(self, cache=None):
        return ops.stage_enabled() and self.tp == 1 and cache is None and not self.tp_always_reduce

    def _reduce(self, t):
        """Sum the row-parallel partial results over the tensor-parallel group (no-op without one).  gloo (CPU tests, debug)
        takes device tensors through host memory."""
        if self.tp > 1 and self.tp_local is not None:
            return self.tp_local.reduce(self.tp_rank, t)
        if (self.tp > 1 or self.tp_always_reduce) and self.tp_group is not None:
            if t.is_cuda and dist.get_backend(self.tp_group) == "gloo":
                h = t.cpu()
                dist.all_reduce(h, group=self.tp_group)
                t.copy_(h)
            else:
                dist.all_reduce(t, group=self.tp_group)
        return t

    # ------------------------------------------------------------------ the rows loop: prefill, prefill_batch, extend (MFMA GEMMs)
    def _rows(self, f, x, segs, outs, append=False):
        """One pass of the layers over the rows x [n, D] with projection form f.  segs = [(s0, s1, P, k per layer, v per layer)]: rows
        s0 .. s1-1 are the positions P .. P + s1 - s0 - 1 of the sequence that owns those caches.  The projections run on all rows at once;
        RoPE, the cache write and the causal attention run per segment on its own cache (append: vl2_attn_append; otherwise vl2_attn_fwd
        with causal_off).  Every form ends on the 16-bit lm_head: the fp32 logits of each segment's last row go to its entry of `outs`.
        Returns the last hidden state [n, D]."""
        nh, nkv, hd, smax = self.nh, self.nkv, self.hd, self.max_seq_len
        q = torch.empty((x.shape[0], nh * hd), dtype=_lib.elem_dtype(), device=self._dev)
        o = torch.empty_like(q)
        f.begin(x)
        for li, lw in enumerate(self.w["layers"]):
            qkv = f.normed(x, f.layers[li]["wqkv"], bias=lw["bqkv"])          # bqkv: Qwen2 only
            for s0, s1, P, kc, vc in segs:
                n = s1 - s0
                ops.rope_kv(qkv[s0:s1], q[s0:s1], kc[li], vc[li], self.cos_t, self.sin_t, nh, nkv, P)
                if append:
                    ops.attn_append(q[s0:s1], kc[li], vc[li], o[s0:s1], P, nh, nkv, hd ** -0.5)
                else:
                    ops.attn_fwd(q[s0:s1], kc[li], vc[li], o[s0:s1], (0, hd, nh * hd), (0, smax * hd, hd), (0, smax * hd, hd),
                                 (0, hd, nh * hd), 1, nh, n, P + n, nh // nkv, hd ** -0.5, True, P, hd)
            x = self._rows_block(f, li, o, x)
        for (_, s1, _, _, _), out in zip(segs, outs):
            ops.gemv(self.w["lm_head"], x[s1 - 1], norm_w=self.w["norm_w"], eps=self.eps, out_f32=True, out=out)
        return x

    def _rows_block(self, f, li, o, x):
        """The rest of a layer after attention, many rows: x + o_proj(o), then the MLP (SwiGLU) with its residual.
        (HipMixtralDecoder replaces it by its sparse MoE block.)"""
        wl = f.layers[li]
        x = f.res(o, wl["wo"], x)
        return f.res(f.normed(x, wl["wgu"], swiglu=True), wl["wd"], x)

    @torch.no_grad()
    def prefill(self, x, return_all_logits=False, cache=None, logits_out=None):
        """x: inputs_embeds [S, D] (any float dtype, device).  Fills the KV cache for positions 0..S-1 and returns
        fp32 logits of the last position [V] (or all positions [S, V]).  cache = (k per layer, v per layer) overrides the
        decoder's own single-sequence cache (batched decode gives every sequence its slice)."""
        _lib.check_elem(self._elem, type(self).__name__)
        kcache, vcache = cache if cache is not None else (self.kcache, self.vcache)
        S = x.shape[0]
        if S > self.max_seq_len:
            raise ValueError(f"sequence length {S} exceeds the KV cache ({self.max_seq_len})")
        x = x.to(device=self._dev, dtype=_lib.elem_dtype()).contiguous()
        if cache is None:
            self.cache_epoch += 1
        out = self.logits if logits_out is None else logits_out
        if self._use_stage(cache) and not return_all_logits:      # the whole prefill as one call into libvl2hip.so (vl2_llm_prefill)
            ops.llm_prefill(self._stage_desc()[0], x, out, fp8=self.prefill_fp8)
            self.pos = S
            self.last_hidden = None
            if self._fp8_kv:
                self._quant_rows(self.kcache, self.vcache, self.kv8, S)
            return out
        # operator by operator: the RMSNorm rides in the q/k/v and gate/up GEMMs (weights.fold_norm), or the fp8 matrix pipe (vl2_stage.inc)
        f = _W8A8(self) if self.prefill_fp8 else _Tiled(self)
        x = self._rows(f, x, [(0, S, 0, kcache, vcache)], () if return_all_logits else (out,))
        self.pos = S
        self.last_hidden = x
        if self._fp8_kv and cache is None:         # the decode steps read the fp8 cache: the prefill's rows, quantised once
            self._quant_rows(kcache, vcache, self.kv8, S)
        if return_all_logits:
            return ops.gemm(ops.rmsnorm(x, self.w["norm_w"], self.eps), self.w["lm_head"], out_f32=True)
        return out

    EXTEND_SKINNY_ROWS = 64      # up to this many rows the projections stream the weights once on the skinny-M kernel (ops.gemm_skinny)
    EXTEND_APPEND_ROWS = 64      # up to this many rows the attention is vl2_attn_append (split-KV); beyond, vl2_attn_fwd with causal_off

    @torch.no_grad()
    def extend(self, x_new, start_pos=None, logits_out=None):
        """Prefill of the rows start_pos .. start_pos + n - 1 (default start_pos = self.pos) against the single-sequence KV cache, whose
        rows 0 .. start_pos - 1 must already hold the sequence (a previous prefill / extend / decode steps); rows from start_pos on are
        overwritten.  x_new: inputs_embeds [n, D].  Leaves the last row's fp32 logits in self.logits (returned) and self.pos =
        start_pos + n.  Few rows: the skinny-M projections (RMSNorm as its own launch, like the batched decode step) and the append
        attention; otherwise the prefill's tiled GEMMs and vl2_attn_fwd."""
        _lib.check_elem(self._elem, type(self).__name__)
        if self._fp8_kv:
            raise NotImplementedError(self.FP8_KV_EXTEND_MSG)
        if self.tp > 1 or self.tp_always_reduce:
            raise NotImplementedError("extend: single-rank decoders only")
        if self.prefill_fp8:
            raise NotImplementedError("extend runs the 16-bit projections: call enable_fp8_prefill(False) first")
        P = self.pos if start_pos is None else int(start_pos)
        n = x_new.shape[0]
        if n <= 0:
            raise ValueError("extend: no rows")
        if P < 0 or P > self.pos:
            raise ValueError(f"extend: start position {P} is not inside the resident cache (0 .. {self.pos})")
        if P + n > self.max_seq_len:
            raise ValueError(f"sequence length {P + n} exceeds the KV cache ({self.max_seq_len})")
        self.cache_epoch += 1
        x = x_new.to(device=self._dev, dtype=_lib.elem_dtype()).contiguous()
        f = _Skinny(self, "16bit", n) if n <= self.EXTEND_SKINNY_ROWS else _Tiled(self)
        out = self.logits if logits_out is None else logits_out
        x = self._rows(f, x, [(0, n, P, self.kcache, self.vcache)], (out,), append=n <= self.EXTEND_APPEND_ROWS)
        self.pos = P + n
        self.last_hidden = x
        return out

    # ------------------------------------------------------------------ the token loop: decode steps (M = 1 or the batch, HBM-bound)
    def _tokens(self, f, attend, x, x1, qkv, o, a, logits):
        """One decode step's layers over x ([D], or [nb, D] for the batch) with projection form f, on the step's buffers x1 / qkv / o / a.
        attend(li, qkv, o): RoPE + cache append + attention on layer li's cache.  Leaves the fp32 logits in `logits`."""
        for li, lw in enumerate(self.w["layers"]):
            f.normed(x, f.layers[li]["wqkv"], bias=lw["bqkv"], out=qkv)
            attend(li, qkv, o)
            self._token_block(f, li, o, x, x1, a)
        f.head(x, logits)

    def _token_block(self, f, li, o, x, x1, a):
        """The rest of a decode layer after attention: x1 = x + o_proj(o), then x = x1 + MLP(x1) in place (x's old value is dead).
        (HipMixtralDecoder replaces the MLP by its sparse MoE GEMVs.)"""
        wl = f.layers[li]
        f.res(o, wl["wo"], x, out=x1)
        f.res(f.normed(x1, wl["wgu"], swiglu=True, out=a), wl["wd"], x1, out=x)

    def _decode_kernels(self, dyn):
        """Enqueue one decode step for the token in self.tok: embed -> 32 x {qkv GEMV (+RMSNorm), RoPE+append+attention,
        o GEMV (+res), gate/up GEMV (+RMSNorm, SwiGLU), down GEMV (+res)} -> lm_head GEMV (+final RMSNorm) into self.logits, on the
        16-bit weights, their fp8 copies (enable_fp8_decode) or their MXFP4 copies (enable_mxfp4_decode; lm_head 16-bit).  dyn=True reads the position from self.state[0] on the device
        (hipGraph-replayable); no allocation either way.  With enable_fp8_kv the attention appends to and reads the fp8 cache (self.kv8); the
        16-bit cache is not touched."""
        b = self._b
        pos_dev = self.state[0:1] if dyn else None
        if self._fp8_kv:
            self._fp8_kv_refusals()                  # (tp_always_reduce can be set after the switch)
        ops.embed_rows(self.tok, self.w["embed"], b["x0"])

        def attend(li, qkv, o):
            if self._fp8_kv:
                return ops.attn_decode_kv8(qkv, self.kv8[li], self.cos_t, self.sin_t, self.partial, o, self.nh, self.nkv, self.pos,
                                           self.hd ** -0.5, pos_dev=pos_dev, ctx_cap=self.max_seq_len)
            ops.attn_decode(qkv, self.kcache[li], self.vcache[li], self.cos_t, self.sin_t, self.partial, o, self.nh, self.nkv,
                            self.pos, self.hd ** -0.5, pos_dev=pos_dev, ctx_cap=self.max_seq_len)
        self._tokens(_Gemv(self, self.decode_format, batched=False), attend, b["x0"][0], b["x1"], b["qkv"], b["o"], b["a"], self.logits)

    @torch.no_grad()
    def decode_step(self, tok_dev=None):
        """Eager step: feed the token in self.tok (or tok_dev) at position self.pos -> fp32 logits [V] (self.logits)."""
        _lib.check_elem(self._elem, type(self).__name__)
        if self.pos >= self.max_seq_len:
            raise ValueError("KV cache exhausted")
        if tok_dev is not None and tok_dev.data_ptr() != self.tok.data_ptr():
            self.tok.copy_(tok_dev)
        self._decode_kernels(dyn=False)
        self.pos += 1
        return self.logits

    @torch.no_grad()
    def capture_graph(self, sampler=None):
        """sampler = (temperature, top_k, top_p): the sampled-token launch (ops.sample_token, reading its uniform number u[step] from
        self.u_buf on the device) takes the argmax's place in the captured step; one graph per sampler setting.
        Capture {argmax -> decode step} once as a hipGraph (torch.cuda.CUDAGraph records the launches libvl2hip.so
        enqueues on the capture stream).  Replays read token / position / step from device memory.
        Tensor-parallel decoders: the two all-reduces per layer are RCCL kernels on the capture stream and become graph nodes
        like every other launch (ProcessGroupNCCL supports stream capture); the host-staged gloo debug path cannot be captured."""
        if (self.tp > 1 or self.tp_always_reduce) and (self.tp_group is None or dist.get_backend(self.tp_group) != "nccl"):
            raise NotImplementedError("hipGraph decode under tensor parallelism needs the nccl (RCCL) backend: gloo stages through the host")
        if sampler is None and self.graph is not None:
            return self.graph
        if sampler is not None and getattr(self, "_graph_sample", (None, None))[0] == tuple(sampler):
            return self._graph_sample[1]
        def one_step():                                       # argmax + the token's forward: ONE call into libvl2hip.so
            if sampler is not None:                           # (the stage call opens with its own argmax: the sampled step is the operator sequence)
                ops.sample_token(self.logits, self.tok, self.u_buf, sampler[0], sampler[1], sampler[2], hist=self.hist, state=self.state)
                self._decode_kernels(dyn=True)
            elif self._use_stage() and not self.decode_mxfp4 and not self._fp8_kv:        # (the stage call knows the 16-bit and the fp8 weights, 16-bit KV)
                d, _, ws = self._stage_desc()
                ops.llm_decode_step(d, self.logits, self.tok, self.state, self.hist, self.partial, ws, fp8=self.decode_fp8)
            else:
                ops.argmax(self.logits, self.tok, self.hist, 0, self.state)
                self._decode_kernels(dyn=True)

        def warm_up():
            self.state.copy_(torch.tensor([max(self.pos - 1, 0), 0], dtype=torch.int32))
            one_step()
        g = self._capture(warm_up, one_step, (self.state, self.tok, self.logits, self.hist[:2]))
        if sampler is not None:
            self._graph_sample = (tuple(sampler), g)
        else:
            self.graph = g
        return g

    @staticmethod
    def _capture(warm_up, step, keep):
        """`step` as a hipGraph: warm-up outside capture on a side stream (first-launch attribute calls, the allocator), capture in
        thread-local mode (a RCCL watchdog thread may be polling events), then the tensors in `keep`, which the warm-up advanced, are
        restored.  Python's cyclic garbage collector is held off while the stream captures: a pass that starts inside the capture may
        finalise a dead decoder (a decoder and its ContinuousBatcher refer to each other, so a dropped pair waits for the collector) and
        with it that decoder's captured graphs and pools, which the runtime does not survive in the middle of a capture (seen: the process
        aborted in a collection that began inside capture_batch_graph).  torch.cuda.graph no longer collects before it captures."""
        saved = [t.clone() for t in keep]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            warm_up()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        gc_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                step()
        finally:
            if gc_on:
                gc.enable()
        for t, s in zip(keep, saved):
            t.copy_(s)
        torch.cuda.synchronize()
        return g

    @torch.no_grad()
    def generate(self, inputs_embeds, max_new_tokens=2048, eos_token_id=None, stopping_criteria=None,
                 return_logits=False, use_graph=False, streamer=None, sampler=None, start_pos=None):
        """Greedy decode (HF GenerationMixin._sample, do_sample=False): returns LongTensor [1, n_new] of NEW tokens.
        Stops at `eos_token_id` (int or list), when `stopping_criteria(output_ids, None)` is truthy
        (KeywordsStoppingCriteria semantics, videollama2/mm_utils.py:341-345), or at max_new_tokens / cache end.
        use_graph=True replays one captured hipGraph per token (argmax + the whole decode step).
        streamer: optional object with put(LongTensor[1, n]) / end() (the HF `BaseStreamer` protocol the reference's worker
        uses with TextIteratorStreamer, serve/model_worker.py:263-300): every new token is handed over as soon as it is known.
        sampler = (temperature, top_k, top_p[, generator]): HF `_sample` with do_sample=True -- the logits warpers in HF's order and one draw per
        step (ops.sample_token, csrc/k_sample.h) instead of the argmax; the uniform numbers come from torch's generator for this device (or the
        given one), so `torch.manual_seed` makes a run repeatable like it does for the reference.
        start_pos: None = prefill `inputs_embeds` from position 0 (the plain path); an int = the cache already holds the sequence's rows
        0 .. start_pos - 1 and `inputs_embeds` are its rows from start_pos on (`extend`), then the same decode loop."""
        eos = eos_set(eos_token_id)
        if start_pos is None:
            logits = self.prefill(inputs_embeds)
        else:
            logits = self.extend(inputs_embeds, start_pos=start_pos)
        if logits.data_ptr() != self.logits.data_ptr():
            self.logits.copy_(logits)
        max_new_tokens = min(max_new_tokens, self.max_seq_len - self.pos + 1)
        crit = None
        if stopping_criteria is not None:
            crit = stopping_criteria if isinstance(stopping_criteria, (list, tuple)) else [stopping_criteria]
        toks, all_logits = [], []
        # a prompt that fills the cache leaves no position to decode into: the capture warm-up would run a step at row
        # max_seq_len (the kernels now ignore such a step, but there is nothing to replay either) -> plain last-step path
        tp_ok = self.tp == 1 or (self.tp_group is not None and dist.get_backend(self.tp_group) == "nccl")
        use_graph = use_graph and tp_ok and self._dev.type == "cuda" and self.pos < self.max_seq_len
        if sampler is not None:
            T, tk, tp = float(sampler[0]), int(sampler[1]), float(sampler[2])
            gen = sampler[3] if len(sampler) > 3 else None
            if getattr(self, "u_buf", None) is None:
                self.u_buf = torch.zeros((self.max_seq_len + 1,), dtype=torch.float32, device=self._dev)
            self.u_buf[:max_new_tokens].copy_(torch.rand((max_new_tokens,), device=self._dev, generator=gen))
            sampler = (T, tk, tp)
        if use_graph:
            g = self.capture_graph(sampler)
            self.state.copy_(torch.tensor([self.pos - 1, 0], dtype=torch.int32))
        for step in range(max_new_tokens):
            if return_logits:
                all_logits.append(self.logits.clone())
            last = step + 1 == max_new_tokens or self.pos >= self.max_seq_len
            if use_graph and not last:
                g.replay()                           # argmax(step) + forward of the new token -> logits(step+1)
                self.pos += 1
            elif sampler is not None:
                ops.sample_token(self.logits, self.tok, self.u_buf, sampler[0], sampler[1], sampler[2], hist=self.hist, step=step)
            else:
                ops.argmax(self.logits, self.tok, self.hist, step)
            t = int(self.tok.item())                 # one 4-byte D2H per token (the reference syncs per token too)
            toks.append(t)
            if streamer is not None:
                streamer.put(torch.tensor([[t]], dtype=torch.long))
            if t in eos or last:
                break
            if crit is not None:
                ids = torch.tensor([toks], dtype=torch.long, device=self._dev)
                if any(bool(c(ids, None)) for c in crit):
                    break
            if not use_graph:
                self.decode_step()
        if streamer is not None:
            streamer.end()
        out = torch.tensor([toks], dtype=torch.long, device=self._dev)
        return (out, torch.stack(all_logits)) if return_logits else out

    # ------------------------------------------------------------------ batched prefill / decode
    @torch.no_grad()
    def prefill_batch(self, xs, caches, logits_out):
        """Several prompts prefilled together: the projections and norms run once on the concatenated rows [sum S_b, D] (bigger
        M: fuller GEMM grids), RoPE / cache fill / causal attention per sequence on its own cache.  Every kernel here is
        row-independent, so the result is bit-identical to prefilling the prompts one by one.
        xs: list of [S_b, D]; caches: list of (k per layer, v per layer); logits_out: [B, V] fp32 (last position of each)."""
        if self.prefill_fp8:
            raise NotImplementedError("fp8 prefill (enable_fp8_prefill) covers the single-sequence prefill; the batched prefill runs the 16-bit "
                                      "projections: call enable_fp8_prefill(False) first")
        lens = [x.shape[0] for x in xs]
        if max(lens) > self.max_seq_len:
            raise ValueError(f"sequence length {max(lens)} exceeds the KV cache ({self.max_seq_len})")
        if any(len(kc) and kc[0] is self.kcache[0] for kc, _ in caches):
            self.cache_epoch += 1
        X = torch.cat([x.to(device=self._dev, dtype=_lib.elem_dtype()) for x in xs], 0).contiguous()
        segs, s0 = [], 0
        for n, (kc, vc) in zip(lens, caches):
            segs.append((s0, s0 + n, 0, kc, vc))
            s0 += n
        self._rows(_Tiled(self), X, segs, logits_out)
        return lens

    def _ensure_batch(self, B, owner=None):
        """Slot buffers (KV caches, positions, tokens, logits) of the batched decode paths.  They are SHARED by `generate_batch`,
        `model.generate(batch > 1)` and `serving.ContinuousBatcher`; a batcher with requests in flight marks them busy
        (`_bb_busy` = the batcher) and every other user is refused until it drains, instead of silently overwriting the caches and
        positions of the requests in flight."""
        busy = getattr(self, "_bb_busy", None)
        if busy is not None and busy is not owner and busy.in_flight():
            raise RuntimeError("the decoder's batch slots are in use by a ContinuousBatcher with requests in flight: drain it "
                               "(run()) or use a second decoder -- generate_batch / batched generate / another batcher would "
                               "overwrite their KV caches")
        if getattr(self, "_bb", None) is not None and self._bb["B"] >= B:
            return self._bb
        self._batch_graphs = {}                      # captured graphs point into the buffers replaced below
        if self._dev.type == "cuda":
            ops.attach_workspace(self._dev)          # fp32 partial sums of the skinny-M GEMMs of a large-batch decode step
        bf = dict(dtype=_lib.elem_dtype(), device=self._dev)
        smax = self.max_seq_len
        if self._fp8_kv:         # the slots in fp8 ONLY (per layer (k8, v8, ks, vs) with a leading slot dimension) + one sequence's 16-bit staging
            self._fp8_kv_refusals()                  # cache, which a request's prefill fills before its rows are quantised into its slot
            caches = dict(kv8=[ops.kv8_alloc((B,), self.nkv, smax, self._dev) for _ in range(self.n_layers)],
                          stage=([torch.zeros((self.nkv, smax, self.hd), **bf) for _ in range(self.n_layers)],
                                 [torch.zeros((self.nkv, smax, self.hd), **bf) for _ in range(self.n_layers)]))
        elif self._paged_kv:     # the pools, the page table (every slot parked on page 0), the allocator + one sequence's 16-bit staging cache;
            self._paged_kv_refusals()                # no tensor of max_seq_len rows per slot
            pps = (smax + ops.KV_PAGE_ROWS - 1) // ops.KV_PAGE_ROWS
            if self._paged_fp8:  # fp8 pages: per layer (k8pool, v8pool, kspool, vspool), codes 0 and scales 1 (the parking page stays finite)
                pools = dict(pools8=[ops.kv8_pool_alloc(self._n_pages, self.nkv, self._dev) for _ in range(self.n_layers)])
            else:
                pools = [ops.kv_pool_alloc(self._n_pages, self.nkv, self._dev) for _ in range(self.n_layers)]
                pools = dict(kpool=[p[0] for p in pools], vpool=[p[1] for p in pools])
            # the table covers 64 * pps >= max_seq_len positions and the kernel wants cos / sin rows for all of them
            cos_t, sin_t = (self.cos_t, self.sin_t) if pps * ops.KV_PAGE_ROWS == smax else self._rope_tables(pps * ops.KV_PAGE_ROWS)
            caches = dict(**pools, pool=PagePool(self._n_pages), pages_per_seq=pps,
                          table=torch.tensor([parked_row(pps)] * B, dtype=torch.int32).to(self._dev), cos_t=cos_t, sin_t=sin_t,
                          stage=([torch.zeros((self.nkv, smax, self.hd), **bf) for _ in range(self.n_layers)],
                                 [torch.zeros((self.nkv, smax, self.hd), **bf) for _ in range(self.n_layers)]))
        else:
            caches = dict(k=[torch.zeros((B, self.nkv, smax, self.hd), **bf) for _ in range(self.n_layers)],
                          v=[torch.zeros((B, self.nkv, smax, self.hd), **bf) for _ in range(self.n_layers)])
        self._bb = dict(
            B=B, **caches,
            partial=torch.empty((B * self.nh * ((smax + 63) // 64) * 130,), dtype=torch.float32, device=self._dev),
            **self._step_buffers(B, smax + 1))
        return self._bb

    def prefill_slot(self, slot, x, logits_out):
        """Prefill one request (inputs_embeds x [S, D]) into batch slot `slot`: rows [0, S) of its caches, the last row's fp32 logits in
        logits_out.  fp8 KV: through the 16-bit staging cache, whose rows [0, S) are then quantised into the slot.  Paged KV: through the
        staging cache likewise, its rows then copied (fp8 pages: quantised) into the pages the slot's table row names (assigned by the caller
        beforehand).  The decoder's own single-sequence position is left alone."""
        bb, own_pos = self._bb, self.pos
        if self._fp8_kv:
            self.prefill(x, cache=bb["stage"], logits_out=logits_out)
            self._quant_rows(*bb["stage"], [tuple(t[slot] for t in kv8) for kv8 in bb["kv8"]], x.shape[0])
        elif self._paged_kv:     # through the 16-bit staging cache (the prefill keeps its bits), then its rows [0, S) into the slot's pages
            self.prefill(x, cache=bb["stage"], logits_out=logits_out)
            for li in range(self.n_layers):
                if self._paged_fp8:                  # (fp8 pages: quantised on their way into the pages)
                    ops.kv_page_quant(bb["stage"][0][li], bb["stage"][1][li], bb["pools8"][li], bb["table"][slot], 0, x.shape[0])
                    continue
                ops.kv_page_scatter(bb["stage"][0][li], bb["stage"][1][li], bb["kpool"][li], bb["vpool"][li], bb["table"][slot], 0, x.shape[0])
        else:
            self.prefill(x, cache=([k[slot] for k in bb["k"]], [v[slot] for v in bb["v"]]), logits_out=logits_out)
        self.pos = own_pos

    PREFILL_GROUP_TOKENS = 8192   # rows prefilled in one pass (activation scratch: ~0.6 GB at 7B widths)
    GEMM_BATCH = 5      # from this many sequences on, the decode step runs its projections on MFMA (M = sequences)

    def _decode_kernels_batched(self, nb, bb=None, attend=None):
        """One decode step for the nb sequences of the batch: the weights stream ONCE for nb tokens, the attention runs per
        sequence on its own cache slice and position (one launch for all of them).
        nb < GEMM_BATCH: multi-row GEMV (a row is bit-identical to the single-sequence step).  nb >= GEMM_BATCH: the
        projections run on the skinny-M MFMA kernel (weights streamed once, GEMV-style, for up to 64 rows; the tiled GEMMs
        beyond that; RMSNorm as its own kernel) -- prefill-style arithmetic, i.e. equal to the single-sequence step to bf16
        rounding, not to the bit.
        With enable_fp8_decode the same step streams the fp8 copies (W8A16): the multi-row fp8 GEMV below GEMM_BATCH (a row is bit-identical
        to the single-sequence fp8 step), the fp8 skinny-M kernel from GEMM_BATCH on, in calls of at most 64 rows (bit-identical to the 16-bit
        skinny-M step on the dequantised weights).  With enable_mxfp4_decode: the same two paths on the MXFP4 copies, with the same guarantees
        against the solo MXFP4 step and the dequantised weights; lm_head on the 16-bit kernels.
        With enable_fp8_kv the attention of every form above runs on the slots' fp8 caches (one vl2_attn_decode_kv8_batched launch per layer):
        a row's attention is bit for bit the single-sequence fp8-KV step's.
        With enable_paged_kv the attention of every form above reads and appends the slots' rows in their pages (one vl2_attn_decode_paged
        launch per layer, the page table read from the device): bit for bit the contiguous slots' step.  On fp8 pages
        (enable_paged_kv(fp8=True)) that launch is vl2_attn_decode_kv8_paged: bit for bit the contiguous fp8-KV slots' step.
        bb / attend: the step's buffers and its attention callable attend(li, qkv, o) when they are not the slots' (the shared-prefix mode,
        `_shared_attend`)."""
        bb = self._bb if bb is None else bb
        if self._fp8_kv:
            self._fp8_kv_refusals()                  # (tp_always_reduce can be set after the slots exist)
        if self._paged_kv and attend is None:
            self._paged_kv_refusals()
        x = bb["x0"][:nb]
        ops.embed_rows(bb["tok"][:nb], self.w["embed"], x)
        if nb >= self.GEMM_BATCH:
            # M = nb rows: every projection is a few-tile grid, bound by how many workgroups stream the weights.  Split-K (partials
            # through the workspace) measured no gain here (B=16 8.09 vs 8.01 ms per step): the fp32 partial exchange costs what it saves
            ops.set_splitk(False)
            f = _Skinny(self, self.decode_format, nb)
        else:
            f = _Gemv(self, self.decode_format, batched=True)

        def attend_slots(li, qkv, o):
            if self._fp8_kv:
                return ops.attn_decode_kv8_batched(qkv, tuple(t[:nb] for t in bb["kv8"][li]), self.cos_t, self.sin_t, bb["partial"], o,
                                                   self.nh, self.nkv, bb["pos"][:nb], self.max_seq_len, self.hd ** -0.5)
            if self._paged_kv and self._paged_fp8:
                return ops.attn_decode_kv8_paged(qkv, bb["pools8"][li], bb["table"], bb["cos_t"], bb["sin_t"], bb["partial"], o, self.nh, self.nkv,
                                                 bb["pos"][:nb], self.max_seq_len, self.hd ** -0.5)
            if self._paged_kv:
                return ops.attn_decode_paged(qkv, bb["kpool"][li], bb["vpool"][li], bb["table"], bb["cos_t"], bb["sin_t"], bb["partial"], o,
                                             self.nh, self.nkv, bb["pos"][:nb], self.max_seq_len, self.hd ** -0.5)
            ops.attn_decode_batched(qkv, bb["k"][li][:nb], bb["v"][li][:nb], self.cos_t, self.sin_t, bb["partial"], o, self.nh, self.nkv,
                                    bb["pos"][:nb], self.max_seq_len, self.hd ** -0.5)
        self._tokens(f, attend_slots if attend is None else attend, x, bb["x1"][:nb], bb["qkv"][:nb], bb["o"][:nb], bb["a"][:nb], bb["logits"][:nb])
        bb["pos"][:nb] += 1

    def _sample_rows(self, nb, bb=None):
        """The draws of slots 0 .. nb-1 in ONE launch from their per-slot settings (samp_T / samp_k / samp_p, u, sstep): greedy slots take the
        argmax, sampled ones draw and advance their sstep."""
        bb = self._bb if bb is None else bb
        ops.sample_tokens(bb["logits"][:nb], bb["samp_T"], bb["samp_k"], bb["samp_p"], bb["u"], bb["sstep"], bb["tok"])

    @torch.no_grad()
    def _batched_step(self, nb, sampled=False, bb=None, attend=None):
        bb = self._bb if bb is None else bb
        if sampled:
            self._sample_rows(nb, bb)
        else:
            for b in range(nb):
                ops.argmax(bb["logits"][b], bb["tok"][b:b + 1])
        self._decode_kernels_batched(nb, bb, attend)

    def capture_batch_graph(self, nb, sampled=False, attend=None, mode=()):
        """{the draws + the whole batched decode step} as ONE hipGraph per (batch size, sampled) (tokens, positions and the
        draw settings live on the device, so the same graph replays for every step).  sampled=False: one argmax launch per
        request; sampled=True: one ops.sample_tokens launch for all nb rows, whatever mix of greedy and sampled slots they hold.
        enable_fp8_decode / enable_mxfp4_decode (on / off) drop them all (_invalidate_graphs): the next step captures the weights then selected.
        attend / mode: the step's attention callable when it is not the slots' own, and what the key names it by (the resident prefix of a
        ContinuousBatcher: `_paged_prefix_attend`, ("prefix", shared rows))."""
        graphs = self.__dict__.setdefault("_batch_graphs", {})
        key = (nb, bool(sampled)) + tuple(mode)
        if key in graphs:
            return graphs[key]
        if self.tp > 1:
            raise NotImplementedError("hipGraph decode is built for the single-GPU decoder (collectives are launched eagerly)")
        bb = self._bb
        step = lambda: self._batched_step(nb, sampled, None, attend)
        graphs[key] = g = self._capture(step, step, (bb["tok"], bb["pos"], bb["logits"], bb["sstep"]))
        return g

    @torch.no_grad()
    def generate_batch(self, inputs_embeds_list, max_new_tokens=2048, eos_token_id=None, return_logits=False, use_graph=None, sampler=None,
                       shared_prefix=None):
        """Greedy decode of several requests at once (not in the reference, whose eval loops run batch 1 and whose worker
        serialises requests; its padded-batch `prepare_inputs_labels_for_multimodal`, arch.py:227-261, is the nearest thing):
        every request is prefilled on its own (its M is already large), then ALL of them decode together, one token per
        request per step.  Prompts may have different lengths (per-sequence positions, no padding).  Returns a list of
        LongTensor [n_new_b] (each ends at its EOS / max_new_tokens); with return_logits also the per-step fp32 logits
        [steps, B, V].  A row of a batched step is bit-identical to the single-sequence step while nb < GEMM_BATCH.
        use_graph (default: on a GPU without tensor parallelism) replays one captured hipGraph per step.
        sampler = (temperature, top_k, top_p[, generator]): HF `_sample` with do_sample=True for every request -- ONE ops.sample_tokens launch per
        step over all requests in place of their argmaxes (request b draws from its own row u[b, step] of uniform numbers, generated request by
        request from the generator, so request 0's stream is the one a single-sequence `generate` with the same seed would use; its token is the
        one ops.sample_token gives on its row); replayed from its own captured graph like the greedy step.
        With enable_fp8_kv the slots hold fp8 rows only, so the requests are prefilled ONE AFTER ANOTHER through the single 16-bit staging
        cache and quantised into their slots (bit-identical to the grouped prefill); what it costs is the fuller GEMM
        grids of the grouped prefill: short prompts run their projections at a smaller M each.
        shared_prefix = x_prefix [P, D] (opt-in): every request's prompt is x_prefix followed by its entry of `inputs_embeds_list` (its
        suffix, at least one row).  The prefix is prefilled ONCE, its KV rows are kept once and read once per step for all requests
        (`_generate_batch_shared`).
        With enable_paged_kv the slots' rows live in pages of the shared pool: every request reserves pages_needed(S_b, max_new_tokens,
        max_seq_len) pages up front (a pool that cannot hold them all raises ValueError before any kernel runs) and gives them back when
        the call returns, on an error as well; the requests are prefilled ONE AFTER ANOTHER through the single 16-bit staging cache and
        copied into their pages (bit-identical to the grouped prefill; the cost is the grouped prefill's fuller GEMM grids, as under
        enable_fp8_kv).  Tokens and logits are bit for bit the contiguous slots'.  shared_prefix is refused."""
        if shared_prefix is not None:
            return self._generate_batch_shared(shared_prefix, inputs_embeds_list, max_new_tokens, eos_token_id, return_logits, use_graph, sampler)
        nb = len(inputs_embeds_list)
        if use_graph is None:
            use_graph = self._dev.type == "cuda" and self.tp == 1
        u_rows = None
        if sampler is not None:
            T_, tk_, tp_ = float(sampler[0]), int(sampler[1]), float(sampler[2])
            if not T_ > 0.0 or tk_ < 0 or not tp_ > 0.0:
                raise ValueError(f"sampler: need temperature > 0, top_k >= 0, top_p > 0 (got {T_}, {tk_}, {tp_})")
            gen = sampler[3] if len(sampler) > 3 else None
            n_u = min(max_new_tokens, self.max_seq_len) + 1
            u_rows = torch.stack([torch.rand((n_u,), device=self._dev, generator=gen) for _ in range(nb)]).contiguous()
        eos = eos_set(eos_token_id)
        bb = self._ensure_batch(nb)
        run = lambda: self._generate_batch_slots(bb, inputs_embeds_list, max_new_tokens, eos, return_logits, use_graph, sampler, u_rows)
        if self._paged_kv:       # reserve every request's pages first; they go back to the pool when the call returns, however it returns
            lens = [int(x.shape[0]) for x in inputs_embeds_list]
            if max(lens) > self.max_seq_len:
                raise ValueError(f"sequence length {max(lens)} exceeds the KV cache ({self.max_seq_len})")
            need = [pages_needed(n, max_new_tokens, self.max_seq_len) for n in lens]
            pool = bb["pool"]
            if sum(need) > pool.n_free:
                raise ValueError(f"paged KV cache: the {nb} requests need {sum(need)} pages ({need}), the pool has {pool.n_free} free "
                                 f"(of {pool.n_pages - 1}; enable_paged_kv(n_pages))")
            pages = [pool.alloc(n) for n in need]
            try:
                self._set_table_rows(0, [table_row(pg, bb["pages_per_seq"]) for pg in pages])
                return run()
            finally:
                for pg in pages:
                    pool.free(pg)
                self._set_table_rows(0, [parked_row(bb["pages_per_seq"])] * nb)
        return run()

    def _generate_batch_slots(self, bb, inputs_embeds_list, max_new_tokens, eos, return_logits, use_graph, sampler, u_rows):
        """generate_batch on the slot buffers bb (paged KV: the requests' pages are in the table already): prefill, then the token loop."""
        nb = len(inputs_embeds_list)
        sampled = sampler is not None
        if sampled:
            T_, tk_, tp_ = float(sampler[0]), int(sampler[1]), float(sampler[2])
            n_u = u_rows.shape[1]
            bb["samp_T"][:nb].fill_(T_); bb["samp_k"][:nb].fill_(tk_); bb["samp_p"][:nb].fill_(tp_)
            bb["u"][:nb, :n_u].copy_(u_rows); bb["sstep"][:nb].zero_()
        # prompts are prefilled together in groups of <= PREFILL_GROUP_TOKENS rows (bit-identical to one by one)
        lens, group, gtok = [], [], 0
        staged = self._fp8_kv or self._paged_kv      # the slots are not 16-bit contiguous caches: one by one through the staging cache
        caches = None if staged else [([k[b] for k in bb["k"]], [v[b] for v in bb["v"]]) for b in range(nb)]

        def flush():
            if group:
                b0 = group[0]
                self.prefill_batch([inputs_embeds_list[b] for b in group], [caches[b] for b in group], bb["logits"][b0:b0 + len(group)])
                group.clear()

        for b, xb in enumerate(inputs_embeds_list):
            if staged:
                if xb.shape[0] > self.max_seq_len:
                    raise ValueError(f"sequence length {xb.shape[0]} exceeds the KV cache ({self.max_seq_len})")
                self.prefill_slot(b, xb, bb["logits"][b])
                lens.append(xb.shape[0])
                continue
            if gtok + xb.shape[0] > self.PREFILL_GROUP_TOKENS:
                flush()
                gtok = 0
            group.append(b)
            gtok += xb.shape[0]
            lens.append(xb.shape[0])
        flush()
        bb["pos"][:nb].copy_(torch.tensor(lens, dtype=torch.int32))
        max_new_tokens = min(max_new_tokens, self.max_seq_len - max(lens) + 1)
        use_graph = use_graph and max(lens) < self.max_seq_len          # a full cache leaves nothing to replay (see generate)
        graph = self.capture_batch_graph(nb, sampled) if use_graph else None
        if graph is not None:                                                # capture clobbered nothing: state was restored
            bb["pos"][:nb].copy_(torch.tensor(lens, dtype=torch.int32))
        return self._batched_loop(bb, nb, max_new_tokens, eos, return_logits, graph, sampled, lambda: self._decode_kernels_batched(nb))

    def _batched_loop(self, bb, nb, max_new_tokens, eos, return_logits, graph, sampled, forward):
        """The token loop of the batched paths on the step buffers bb: draws, stop checks on the host, then `forward()` (or the captured
        graph, which holds the draws and the forward of a step)."""
        outs, done, all_logits = [[] for _ in range(nb)], [False] * nb, []
        for step in range(max_new_tokens):
            if return_logits:
                all_logits.append(bb["logits"][:nb].clone())
            last = step + 1 == max_new_tokens
            if graph is not None and not last:
                graph.replay()                                               # draws(step) + forward of the new tokens
            elif sampled:
                self._sample_rows(nb, bb)
            else:
                for b in range(nb):
                    ops.argmax(bb["logits"][b], bb["tok"][b:b + 1])
            toks = bb["tok"][:nb].tolist()                                   # one small D2H per step for the stop checks
            for b, t in enumerate(toks):
                if not done[b]:
                    outs[b].append(t)
                    done[b] = t in eos
            if all(done) or last:
                break
            if graph is None:
                forward()
        res = [torch.tensor(o, dtype=torch.long, device=self._dev) for o in outs]
        return (res, torch.stack(all_logits)) if return_logits else res

    # ------------------------------------------------------------------ batched decode over a shared prompt prefix
    def _shared_prefix_refusals(self, paged_ok=False):
        """paged_ok: the caller keeps the prefix and the own rows in pages (the resident prefix of a ContinuousBatcher)."""
        if not paged_ok and getattr(self, "_paged_kv", False):
            raise NotImplementedError("shared-prefix decode: the paged KV cache is on (the private caches of this mode are contiguous): call "
                                      "enable_paged_kv(0, False) first")
        if self._fp8_kv:
            raise NotImplementedError("shared-prefix decode: the fp8 KV cache is on (the prefix phase and extend read 16-bit rows): call "
                                      "enable_fp8_kv(False) first")
        if self.tp > 1 or self.tp_group is not None or self.tp_local is not None or self.tp_always_reduce:
            raise NotImplementedError("shared-prefix decode: single-rank decoders only (extend and the prefix phase are not built for a "
                                      "tensor-parallel shard)")
        if self.hd != 128:
            raise NotImplementedError(f"shared-prefix decode: head_dim 128 only (this decoder has {self.hd})")
        if self.prefill_fp8:
            raise NotImplementedError("shared-prefix decode: the suffixes run through extend, which runs the 16-bit projections: call "
                                      "enable_fp8_prefill(False) first")

    def _ensure_shared(self, B, P, own_cap):
        """Step buffers of the shared-prefix mode: the private caches [B, nkv, own_cap, 128] per layer (a request's rows from position P
        on -- not max_seq_len rows), the partial workspace for (P, own_cap) and the per-request step state of `_ensure_batch`."""
        sp = getattr(self, "_sp", None)
        if sp is not None and (sp["B"], sp["P"], sp["own_cap"]) == (B, P, own_cap):
            return sp
        self._sp = None                               # (the old caches go before the new ones are allocated)
        if self._dev.type == "cuda":
            ops.attach_workspace(self._dev)
        bf = dict(dtype=_lib.elem_dtype(), device=self._dev)
        cos_t, sin_t = self.cos_t, self.sin_t
        if P + own_cap > self.max_seq_len:            # own_cap is rounded up to the slice: the launch covers rows no request reaches
            cos_t, sin_t = self._rope_tables(P + own_cap)
        self._sp = dict(
            B=B, P=P, own_cap=own_cap, cos_t=cos_t, sin_t=sin_t,
            k=[torch.zeros((B, self.nkv, own_cap, self.hd), **bf) for _ in range(self.n_layers)],
            v=[torch.zeros((B, self.nkv, own_cap, self.hd), **bf) for _ in range(self.n_layers)],
            partial=torch.empty((B * ops.shared_partial_floats(P, own_cap, self.nh),), dtype=torch.float32, device=self._dev),
            **self._step_buffers(B, own_cap + 1))
        return self._sp

    def _shared_attend(self, sp, nb):
        """The attention callable of a shared-prefix step: prefix phase + own rows + combine (one ops.attn_decode_shared call per layer) on
        the decoder's single-sequence cache (rows [0, P): the shared prefix) and the private caches of sp."""
        def attend(li, qkv, o):
            ops.attn_decode_shared(qkv, self.kcache[li], self.vcache[li], sp["k"][li][:nb], sp["v"][li][:nb], sp["cos_t"], sp["sin_t"],
                                   sp["partial"], o, self.nh, self.nkv, sp["P"], sp["pos"][:nb], self.hd ** -0.5)
        return attend

    @torch.no_grad()
    def _generate_batch_shared(self, x_prefix, suffixes, max_new_tokens, eos_token_id, return_logits, use_graph, sampler):
        """generate_batch(shared_prefix=x_prefix): request b's prompt is x_prefix [P, D] ++ suffixes[b] [n_b, D].
        The prefix is prefilled once (the unchanged `prefill`) into the decoder's single-sequence cache, which IS the shared prefix.  Each
        suffix then runs through `extend(start_pos=P)` on that cache (existing kernels, existing bits); its rows [P, P + n_b) of every
        layer are copied to rows [0, n_b) of the request's private cache, its last row's logits to the request's logits row, and the next
        request overwrites the rows from P on.  The private caches hold own_cap = (longest suffix + max_new_tokens, rounded up to 64) rows
        per request.  The decode loop is generate_batch's; its step is `_decode_kernels_batched` with `_shared_attend`, captured as one
        hipGraph per call (P is a launch constant).  Projections: 16-bit, fp8 or MXFP4 decode weights, untouched.  A request's attention
        agrees with the plain batched step's to 16-bit rounding, not to the bit: the prefix sums run on the matrix pipe."""
        self._shared_prefix_refusals()
        _lib.check_elem(self._elem, type(self).__name__)
        nb, P = len(suffixes), int(x_prefix.shape[0])
        lens = [int(x.shape[0]) for x in suffixes]
        if nb == 0 or P <= 0 or min(lens) <= 0:
            raise ValueError("shared-prefix decode: need a prefix of at least one row and, for every request, a suffix of at least one row")
        if P + max(lens) > self.max_seq_len:
            raise ValueError(f"sequence length {P + max(lens)} exceeds the KV cache ({self.max_seq_len})")
        if use_graph is None:
            use_graph = self._dev.type == "cuda"
        sampled = sampler is not None
        max_new_tokens = min(max_new_tokens, self.max_seq_len - (P + max(lens)) + 1)
        if sampled:
            T_, tk_, tp_ = float(sampler[0]), int(sampler[1]), float(sampler[2])
            if not T_ > 0.0 or tk_ < 0 or not tp_ > 0.0:
                raise ValueError(f"sampler: need temperature > 0, top_k >= 0, top_p > 0 (got {T_}, {tk_}, {tp_})")
            gen = sampler[3] if len(sampler) > 3 else None
            n_u = max_new_tokens + 1
            u_rows = torch.stack([torch.rand((n_u,), device=self._dev, generator=gen) for _ in range(nb)]).contiguous()
        eos = eos_set(eos_token_id)
        sp = self._ensure_shared(nb, P, ops.shared_own_cap(max(lens), max_new_tokens))
        if sampled:
            sp["samp_T"].fill_(T_); sp["samp_k"].fill_(tk_); sp["samp_p"].fill_(tp_)
            sp["u"][:, :n_u].copy_(u_rows); sp["sstep"].zero_()
        self.prefill(x_prefix)
        for b, xb in enumerate(suffixes):
            self.extend(xb, start_pos=P, logits_out=sp["logits"][b])
            for li in range(self.n_layers):
                sp["k"][li][b, :, :lens[b]].copy_(self.kcache[li][:, P:P + lens[b]])
                sp["v"][li][b, :, :lens[b]].copy_(self.vcache[li][:, P:P + lens[b]])
        self.pos = P                                  # the resident rows a later extend may build on: the prefix
        pos0 = torch.tensor([P + n for n in lens], dtype=torch.int32)
        sp["pos"].copy_(pos0)
        attend = self._shared_attend(sp, nb)
        graph = None
        if use_graph and P + max(lens) < self.max_seq_len and max_new_tokens > 1:
            step = lambda: self._batched_step(nb, sampled, sp, attend)
            graph = self._capture(step, step, (sp["tok"], sp["pos"], sp["logits"], sp["sstep"]))
        return self._batched_loop(sp, nb, max_new_tokens, eos, return_logits, graph, sampled, lambda: self._decode_kernels_batched(nb, sp, attend))

    # ------------------------------------------------------------------ a shared prefix held once in the page pool
    def _paged_prefix_attend(self, px, nb):
        """The attention callable of a step over a resident prefix: prefix phase + own rows + combine through the page table (one
        ops.attn_decode_shared_paged call per layer).  px: the batcher's handle (serving.PrefixHandle: shared_rows, own_cap, prefix_pages on
        the device, partial)."""
        bb = self._bb

        def attend(li, qkv, o):
            ops.attn_decode_shared_paged(qkv, bb["kpool"][li], bb["vpool"][li], bb["table"], px.prefix_pages, bb["cos_t"], bb["sin_t"],
                                         px.partial, o, self.nh, self.nkv, px.shared_rows, px.own_cap, bb["pos"][:nb], self.hd ** -0.5)
        return attend

    def _prefix_rows_to_pages(self, slot, p0, p1):
        """Rows [p0, p1) of the single-sequence cache -> the pages slot's table row names, every layer."""
        bb = self._bb
        for li in range(self.n_layers):
            ops.kv_page_scatter(self.kcache[li], self.vcache[li], bb["kpool"][li], bb["vpool"][li], bb["table"][slot], p0, p1)

    def _prefix_rows_from_pages(self, slot, p0, p1):
        """The inverse: rows [p0, p1) of the single-sequence cache <- the pages slot's table row names, every layer."""
        bb = self._bb
        for li in range(self.n_layers):
            ops.kv_page_gather(bb["kpool"][li], bb["vpool"][li], self.kcache[li], self.vcache[li], bb["table"][slot], p0, p1)


HipQwen2Decoder = HipMistralDecoder      # same decoder; the q/k/v bias is picked up from the state dict (weights.pack_decoder)


class HipMixtralDecoder(HipMistralDecoder):
    """The decoder of VideoLLaMA2-8x7B (videollama2/model/videollama2_mixtral.py, HF:models/mixtral/modeling_mixtral.py): the Mistral
    attention, RoPE, norms and lm_head of the parent, and in every layer a sparse MoE block (MixtralSparseMoeBlock) in place of the MLP --
    router, token grouping, grouped expert GEMMs and combine on csrc/k_moe.h.  Runs operator by operator (the stage calls are
    dense-only); every routing table stays on the device, so the prefill and the decode step both capture into graphs.
    Single GPU, 16-bit weights: tensor parallelism and fp8 weights raise NotImplementedError, and so does batched / continuous decoding
    until `enable_moe_batch()` switches it on.  `enable_moe_fp8()` is this decoder's own fp8 switch: the decode
    step's expert products on e4m3fn copies of the expert stacks, everything else 16-bit.  `enable_moe_mxfp4()` is
    the same switch for OCP MXFP4 copies (4.25 bits per weight); the two exclude each other."""

    def __init__(self, cfg, state_dict, device="cuda", max_seq_len=4096, n_layers=None, tp_group=None, tp_shard=None, tp_local=None):
        if tp_group is not None or tp_shard is not None or tp_local is not None:
            raise NotImplementedError("MoE (mixtral) decoder: tensor / expert parallelism not built")
        super().__init__(cfg, state_dict, device, max_seq_len, n_layers)
        l = cfg["llm"]
        self.E, self.k, self.I = l["num_local_experts"], l["num_experts_per_tok"], l["intermediate_size"]
        self.moe_ids = torch.zeros((self.k,), dtype=torch.int32, device=self._dev)
        self.moe_wts = torch.zeros((self.k,), dtype=torch.float32, device=self._dev)
        self._b["a"] = torch.empty((self.k, self.I), dtype=_lib.elem_dtype(), device=self._dev)

    def _use_stage(self, cache=None):
        return False

    def enable_fp8_decode(self, on=True):
        raise NotImplementedError("MoE (mixtral) decoder: fp8 weights not built")

    def enable_fp8_prefill(self, on=True):
        raise NotImplementedError("MoE (mixtral) decoder: fp8 weights not built")

    def enable_mxfp4_decode(self, on=True):
        raise NotImplementedError("MoE (mixtral) decoder: MXFP4 weights not built")

    def enable_fp8_kv(self, on=True):
        raise NotImplementedError("MoE (mixtral) decoder: the fp8 KV cache is not built for it (its step runs the MoE GEMVs on the 16-bit "
                                  "cache): keep the 16-bit cache")

    def enable_paged_kv(self, n_pages, on=True, fp8=False):
        raise NotImplementedError("MoE (mixtral) decoder: the paged KV cache is not built for it (its batched decoding is not): keep the "
                                  "contiguous cache")

    # The regimes of the batched step's MoE block, set from scripts/moe_batch_bench.py (profiles/r20_moe_batch_bench.jsonl):
    MOE_GEMM_BATCH = 5      # below this many sequences: the solo step's GEMVs per token (a row is bit for bit the solo step, as below GEMM_BATCH
    #                         on the dense decoders); from it on the grouped kernels
    MOE_SKINNY_ROWS = 0     # up to this many sequences the grouped kernels are the grouped skinny-M GEMM (ops.moe_gemm_skinny), beyond it the
    #                         prefill's tiled grouped GEMM (ops.moe_gemm).  0: the tiled form at every size -- it measured faster than the
    #                         skinny form at every size from 5 to 64 (2 % at 5, 10 % at 16, 24 % at 64), so the skinny form serves no size by
    #                         default; 64 selects it for 5 .. 64 sequences (tests, the benchmark's comparison)

    @property
    def moe_batch(self):
        """Whether batched / continuous decoding is on (enable_moe_batch)."""
        return getattr(self, "_moe_batch", False)

    @torch.no_grad()
    def enable_moe_batch(self, on=True):
        """OPT-IN, off by default (with it off every refusal below stands word for word): batched prefill, `generate_batch`, hipGraph batch
        steps and `serving.ContinuousBatcher` on this decoder, with per-request sampling as for the dense decoders.
        The batched step's MoE block: below MOE_GEMM_BATCH sequences the solo step's GEMVs per token in one launch per form (a row is bit for
        bit the solo step); from it on a grouped GEMM, in which every active expert's weights stream once per step for all the rows routed
        to it (equal to the solo step to 16-bit rounding): the prefill's tiled grouped GEMM, or up to MOE_SKINNY_ROWS sequences the grouped
        skinny-M GEMM (0 by default: it measured slower).  Still refused: a shared prefix,
        the paged and the fp8 KV cache, fp8 / MXFP4 weights, tensor parallelism.  Switching drops the captured batch graphs and the slot
        buffers; it is refused while a batcher holds requests in flight."""
        busy = getattr(self, "_bb_busy", None)
        if busy is not None and busy.in_flight():
            raise RuntimeError("enable_moe_batch: a ContinuousBatcher holds requests in flight on this decoder's slots: drain it (run()) first")
        self._moe_batch = bool(on)
        self._invalidate_graphs()
        self._bb = None
        return self

    MOE_FP8_ROWS = 64       # the most sequences of a batched step while enable_moe_fp8 is on WITHOUT tiled=True: the grouped skinny-M GEMM's
    #                         limit (the 16-bit tiled form would change a request's arithmetic with the batch size; the tiled W8A16 grouped
    #                         GEMM, csrc/k_moe_gemm8.h, serves any number of sequences behind enable_moe_fp8(tiled=True))
    # With enable_moe_fp8(tiled=True): from this many sequences on the fp8 step runs the tiled W8A16 grouped GEMM (ops.moe_gemm_fp8), below it
    # the fp8 grouped skinny-M GEMM.  The rule: the smallest measured size from which the tiled fp8 step is faster than the fp8 skinny step at
    # that size and at every larger measured size by more than twice the spread of the 16-bit step timed twice; 65 if there is none (tiled then
    # serves only what was refused before).  Measured (scripts/moe_fp8_tiled_bench.py, profiles/r23_moe_fp8_tiled_bench.jsonl, DESIGN.md 22d;
    # ms per 8-layer step, skinny / tiled, spread <= 0.003 ms): 5: 3.37 / 3.26, 6: 3.58 / 3.37, 8: 3.85 / 3.51, 12: 4.27 / 3.70, 16: 4.58 / 3.80,
    # 24: 5.28 / 4.01, 32: 5.59 / 4.17, 48: 6.76 / 4.51, 64: 7.29 / 4.80 -- the tiled form wins at every measured size, so the fp8 skinny form
    # serves no size under tiled=True (the value is clamped to MOE_GEMM_BATCH: the rows kernels keep the sizes below it)
    MOE_FP8_TILED_FROM = 5

    @property
    def moe_fp8(self):
        """Whether the decode step's expert products stream fp8 copies of the expert weights (enable_moe_fp8)."""
        return getattr(self, "_moe_fp8", False)

    @property
    def moe_fp8_tiled(self):
        """Whether the batched fp8 step may run the tiled W8A16 grouped GEMM (enable_moe_fp8(tiled=True))."""
        return getattr(self, "_moe_fp8_tiled", False)

    @torch.no_grad()
    def enable_moe_fp8(self, on=True, tiled=False):
        """OPTIONAL arithmetic, never the default: every expert product of the decode step -- the solo step, and with
        enable_moe_batch() the batched and continuous steps -- reads OCP e4m3fn copies of wgu [E, 2I, D] and wd [E, D, I] with one power-of-two
        scale per expert and output row (ops.moe_quant_fp8, the quantiser of oracle/fp8_oracle.py); activations stay 16-bit, products and sums
        fp32 (csrc/k_moe_fp8.h).  The prefill, the router, attention, RoPE, the KV cache, wqkv / wo and lm_head keep their 16-bit weights, so
        `decode_format` stays "16bit" and enable_fp8_decode / enable_fp8_prefill / enable_mxfp4_decode keep refusing.  The copies are made
        once, here (+45 GB beside the 93 GB of 16-bit weights for the 8x7B model at full depth; the prefill still reads the latter).
        A batched step runs the fp8 rows kernels below MOE_GEMM_BATCH sequences and the fp8 grouped skinny-M GEMM from there to MOE_FP8_ROWS
        = 64; more slots than that are refused (the 16-bit tiled form is never used while the switch is on).
        tiled=True adds a third regime: from MOE_FP8_TILED_FROM sequences on, for any number of them, the prefill's
        sparse block on the fp8 stacks -- ops.moe_route, the tiled W8A16 grouped GEMM ops.moe_gemm_fp8 (csrc/k_moe_gemm8.h) twice,
        ops.moe_combine -- so more than 64 slots are admitted.  Both grouped forms are W8A16 on the same bytes: a request's arithmetic still
        changes with the batch size by summation order only.
        Switching `on` or `tiled` drops the captured graphs and bumps cache_epoch; it is refused while a batcher holds requests in flight."""
        busy = getattr(self, "_bb_busy", None)
        if busy is not None and busy.in_flight():
            raise RuntimeError("enable_moe_fp8: a ContinuousBatcher holds requests in flight on this decoder's slots: drain it (run()) first")
        if on and self.moe_mxfp4:
            raise ValueError("MXFP4 expert weights are on: call enable_moe_mxfp4(False) before enable_moe_fp8()")
        if on and getattr(self, "w8moe", None) is None:
            self.w8moe = [dict(wgu=ops.moe_quant_fp8(lw["wgu"]), wd=ops.moe_quant_fp8(lw["wd"])) for lw in self.w["layers"]]
        self._moe_fp8 = bool(on)
        self._moe_fp8_tiled = bool(on and tiled)
        self._invalidate_graphs()
        self.cache_epoch = getattr(self, "cache_epoch", 0) + 1
        return self

    MOE_MXFP4_ROWS = 64     # the most sequences of a batched step while enable_moe_mxfp4 is on WITHOUT tiled=True: the grouped skinny-M GEMM's
    #                         limit (the 16-bit tiled form would change a request's arithmetic with the batch size; the tiled W4A16 grouped
    #                         GEMM, csrc/k_moe_gemm4.h, serves any number of sequences behind enable_moe_mxfp4(tiled=True))
    # With enable_moe_mxfp4(tiled=True): from this many sequences on the MXFP4 step runs the tiled W4A16 grouped GEMM (ops.moe_gemm_mxfp4), below
    # it the MXFP4 grouped skinny-M GEMM.  The rule is MOE_FP8_TILED_FROM's: the smallest measured size from which the tiled MXFP4 step is faster
    # than the MXFP4 skinny step at that size and at every larger measured size by more than twice the spread of the 16-bit step timed twice;
    # 65 if there is none (tiled then serves only what was refused before).  Measured (scripts/moe_mxfp4_tiled_bench.py,
    # profiles/r25_moe_mxfp4_tiled_bench.jsonl; ms per 8-layer step, skinny / tiled, spread <= 0.003 ms): 5: 4.62 / 3.17,
    # 6: 4.83 / 3.25, 8: 5.27 / 3.40, 12: 5.70 / 3.58, 16: 6.05 / 3.69, 24: 6.71 / 3.91, 32: 7.08 / 4.07, 48: 8.35 / 4.42, 64: 8.92 / 4.72 -- the
    # tiled form wins at every measured size, so the MXFP4 skinny form serves no size under tiled=True (the value is clamped to MOE_GEMM_BATCH:
    # the rows kernels keep the sizes below it)
    MOE_MXFP4_TILED_FROM = 5

    @property
    def moe_mxfp4(self):
        """Whether the decode step's expert products stream MXFP4 copies of the expert weights (enable_moe_mxfp4)."""
        return getattr(self, "_moe_mxfp4", False)

    @property
    def moe_mxfp4_tiled(self):
        """Whether the batched MXFP4 step may run the tiled W4A16 grouped GEMM (enable_moe_mxfp4(tiled=True))."""
        return getattr(self, "_moe_mxfp4_tiled", False)

    def _moe_mxfp4_limit(self, got):
        return NotImplementedError(f"MoE (mixtral) decoder: MXFP4 expert weights are on (enable_moe_mxfp4): a batched step takes at most "
                                   f"{self.MOE_MXFP4_ROWS} sequences, the grouped skinny-M GEMM's limit (no tiled W4A16 grouped GEMM is built); "
                                   f"got {got}")

    @torch.no_grad()
    def enable_moe_mxfp4(self, on=True, tiled=False):
        """OPTIONAL arithmetic, never the default: every expert product of the decode step -- the solo step, and with
        enable_moe_batch() the batched and continuous steps -- reads OCP MXFP4 copies of wgu [E, 2I, D] and wd [E, D, I]: E2M1 codes with one
        E8M0 scale per block of 32 k, 4.25 bits per weight (ops.moe_quant_mxfp4, the quantiser of tests/mxfp4_oracle.py); activations stay
        16-bit, products and sums fp32, the block scale rides in the conversion (W4A16, csrc/k_moe_mxfp4.h).  The prefill, the router,
        attention, RoPE, the KV cache, wqkv / wo and lm_head keep their 16-bit weights, so `decode_format` stays "16bit" and
        enable_fp8_decode / enable_fp8_prefill / enable_mxfp4_decode keep refusing.  The copies are made once, here (computed: E * 3 * I * D *
        32 layers * 4.25 / 8 bytes = +24 GB beside the 93 GB of 16-bit weights for the 8x7B model at full depth; the prefill still reads the
        latter).  A batched step runs the MXFP4 rows kernels below MOE_GEMM_BATCH sequences and the MXFP4 grouped skinny-M GEMM from there to
        MOE_MXFP4_ROWS = 64; more slots than that are refused without tiled=True, and the 16-bit tiled form is never used while the switch is
        on (a request's arithmetic may change with the batch size by summation order only).
        tiled=True adds a third regime: from MOE_MXFP4_TILED_FROM sequences on, for any number of them, the prefill's
        sparse block on the MXFP4 stacks -- ops.moe_route, the tiled W4A16 grouped GEMM ops.moe_gemm_mxfp4 (csrc/k_moe_gemm4.h) twice,
        ops.moe_combine -- so more than 64 slots are admitted.  Both grouped forms are W4A16 on the same bytes: a request's arithmetic still
        changes with the batch size by summation order only.
        enable_moe_fp8 and this switch refuse each other while the other is on.  Switching `on` or `tiled` drops the captured graphs and
        bumps cache_epoch; it is refused while a batcher holds requests in flight."""
        busy = getattr(self, "_bb_busy", None)
        if busy is not None and busy.in_flight():
            raise RuntimeError("enable_moe_mxfp4: a ContinuousBatcher holds requests in flight on this decoder's slots: drain it (run()) first")
        if on and self.moe_fp8:
            raise ValueError("fp8 expert weights are on: call enable_moe_fp8(False) before enable_moe_mxfp4()")
        if on and getattr(self, "w4moe", None) is None:
            self.w4moe = [dict(wgu=ops.moe_quant_mxfp4(lw["wgu"]), wd=ops.moe_quant_mxfp4(lw["wd"])) for lw in self.w["layers"]]
        self._moe_mxfp4 = bool(on)
        self._moe_mxfp4_tiled = bool(on and tiled)
        self._invalidate_graphs()
        self.cache_epoch = getattr(self, "cache_epoch", 0) + 1
        return self

    def prefill_batch(self, xs, caches, logits_out):
        if not getattr(self, "_moe_batch", False):
            raise NotImplementedError("MoE (mixtral) decoder: batched prefill not built")
        # the scan kernel stages rows * k expert ids (csrc/k_moe.h MOE_SCAN_MAX): groups of at most that many rows, each bit for bit the
        # prompts one by one (every kernel of the rows loop is row-independent)
        cap, lens, b0 = self.MOE_SCAN_IDS // self.k, [], 0
        while b0 < len(xs):
            b1, rows = b0 + 1, xs[b0].shape[0]
            while b1 < len(xs) and rows + xs[b1].shape[0] <= cap:
                rows += xs[b1].shape[0]
                b1 += 1
            lens += super().prefill_batch(xs[b0:b1], caches[b0:b1], logits_out[b0:b1])
            b0 = b1
        return lens

    MOE_SCAN_IDS = 16384     # csrc/k_moe.h MOE_SCAN_MAX

    def generate_batch(self, *args, **kwargs):
        if kwargs.get("shared_prefix") is not None:
            self._shared_prefix_refusals()
        if not getattr(self, "_moe_batch", False):
            raise NotImplementedError("MoE (mixtral) decoder: batched decoding not built")
        return super().generate_batch(*args, **kwargs)

    def _shared_prefix_refusals(self, paged_ok=False):
        raise NotImplementedError("MoE (mixtral) decoder: shared-prefix decode is not built (its batched decoding is not)")

    def moe_part_bytes(self, nb):
        """Bytes of fp32 partial sums of the grouped skinny-M GEMMs of a step of nb <= 64 sequences: the larger of gate/up (N = 2I, K = D)
        and down (N = D, K = I), each ks * nb*k * N * 4 with the skinny-M K split ks of its (N, K)."""
        return max(ops.moe_skinny_part_bytes(nb, self.k, 2 * self.I, self.D), ops.moe_skinny_part_bytes(nb, self.k, self.D, self.I))

    def _moe_step_buffers(self, B):
        """The MoE block's buffers of a batched step for B slots: ids / weights [B, k], the compact tables, the normalised rows, the SwiGLU
        rows [B*k, I], the down rows [B*k, D] and the fp32 partials of the grouped skinny-M GEMMs (for min(B, 64) rows)."""
        bf = dict(dtype=_lib.elem_dtype(), device=self._dev)
        i32 = dict(dtype=torch.int32, device=self._dev)
        k = self.k
        return dict(ids=torch.zeros((B, k), **i32), wts=torch.zeros((B, k), dtype=torch.float32, device=self._dev),
                    counts=torch.zeros((self.E,), **i32), offs=torch.zeros((self.E + 1,), **i32), gather=torch.zeros((B * k,), **i32),
                    inv=torch.zeros((B, k), **i32), h=torch.empty((B, self.D), **bf), a=torch.empty((B * k, self.I), **bf),
                    y=torch.empty((B * k, self.D), **bf),
                    part=torch.empty((self.moe_part_bytes(min(B, 64)) // 4,), dtype=torch.float32, device=self._dev))

    def _ensure_batch(self, B, owner=None):
        if not getattr(self, "_moe_batch", False):
            raise NotImplementedError("MoE (mixtral) decoder: batched / continuous decoding not built")
        if self.moe_fp8 and not self.moe_fp8_tiled and B > self.MOE_FP8_ROWS:
            raise NotImplementedError(f"MoE (mixtral) decoder: fp8 expert weights are on (enable_moe_fp8): a batched step takes at most "
                                      f"{self.MOE_FP8_ROWS} sequences, the grouped skinny-M GEMM's limit (no tiled W8A16 grouped GEMM is built); "
                                      f"got {B}")
        if self.moe_mxfp4 and not self.moe_mxfp4_tiled and B > self.MOE_MXFP4_ROWS:
            raise self._moe_mxfp4_limit(B)
        bb = super()._ensure_batch(B, owner)
        if "moe" not in bb:
            bb["moe"] = self._moe_step_buffers(bb["B"])
        return bb

    def moe_block(self, lw, x1, rn):
        """x1 [S, D] (attention output + residual) -> x1 + MoE(RMSNorm(x1)); rn [S, 2] gets (0, rstd) of the result for the next
        layer's norm-carrying q/k/v GEMM.  Route (ids, weights, counts, offsets, gather / inverse tables, permuted rows), grouped
        gate/up + SwiGLU, grouped down, combine: five launches' worth of kernels, no host synchronisation."""
        S = x1.shape[0]
        r = ops.moe_route(x1, lw["wr"], self.k, self.eps)
        self.last_route = r                                   # (the tables of the last layer routed: tests follow the kernel's choice)
        a = ops.moe_gemm(r["xg"], lw["wgu"], r, S, self.k, swiglu=True, row_norm=r["rn"], eps=self.eps)
        y = ops.moe_gemm(a, lw["wd"], r, S, self.k)
        return ops.moe_combine(x1, y, r, self.eps, out=x1, row_norm=rn)

    @torch.no_grad()
    def prefill(self, x, return_all_logits=False, cache=None, logits_out=None):
        if cache is not None and not getattr(self, "_moe_batch", False):
            raise NotImplementedError("MoE (mixtral) decoder: external caches (batched decoding) not built")
        return super().prefill(x, return_all_logits=return_all_logits, cache=cache, logits_out=logits_out)

    def _rows_block(self, f, li, o, x):
        """x1 = x + o_proj(o) on the tiled GEMM whatever the form (its norm is taken by the router), then the sparse MoE block (any row
        count); the combine leaves (0, rstd) in the form's rn."""
        lw = self.w["layers"][li]
        return self.moe_block(lw, ops.gemm(o, lw["wo"], res=x), f.rn)

    def _token_block(self, f, li, o, x, x1, a):
        """x1 = x + o_proj(o); router GEMV (+RMSNorm, softmax, top-k -> ids / weights on the device); gate/up+SwiGLU GEMV of the k chosen
        experts (one launch); down GEMV of both (one launch, weighted, + residual) into x.  No host read: the step replays as a graph."""
        lw = self.w["layers"][li]
        if x.dim() == 2:
            return self._token_block_batched(f, lw, o, x, x1, li)
        ops.gemv(lw["wo"], o, res=x, out=x1)
        ops.moe_route_gemv(x1, lw["wr"], self.moe_ids, self.moe_wts, self.eps)
        if self.moe_fp8:                         # the same two launches on the fp8 copies of the expert stacks (enable_moe_fp8)
            w8 = self.w8moe[li]
            ops.moe_gemv_fp8(*w8["wgu"], x1, self.moe_ids, swiglu=True, eps=self.eps, out=a)
            ops.moe_gemv_fp8(*w8["wd"], a, self.moe_ids, wts=self.moe_wts, res=x1, out=x)
            return
        if self.moe_mxfp4:                       # the same two launches on the MXFP4 copies (enable_moe_mxfp4)
            w4 = self.w4moe[li]
            ops.moe_gemv_mxfp4(*w4["wgu"], x1, self.moe_ids, swiglu=True, eps=self.eps, out=a)
            ops.moe_gemv_mxfp4(*w4["wd"], a, self.moe_ids, wts=self.moe_wts, res=x1, out=x)
            return
        ops.moe_gemv(lw["wgu"], x1, self.moe_ids, swiglu=True, eps=self.eps, out=a)
        ops.moe_gemv(lw["wd"], a, self.moe_ids, wts=self.moe_wts, res=x1, out=x)

    def _token_block_batched_fp8(self, w8, lw, x, x1, nb, m, ids, wts):
        """The MoE block of a batched step on the fp8 expert copies: the rows kernels below MOE_GEMM_BATCH (a row is bit for bit the solo fp8
        step), the grouped skinny-M GEMM from there to MOE_FP8_ROWS (the solo fp8 step up to summation order); with enable_moe_fp8(tiled=True)
        the tiled W8A16 grouped GEMM from MOE_FP8_TILED_FROM on, for any nb (the same, up to summation order).  Returns the (ids, wts) the
        block routed with."""
        k, R = self.k, nb * self.k
        if self.moe_fp8_tiled and nb >= max(self.MOE_FP8_TILED_FROM, self.MOE_GEMM_BATCH):
            r = ops.moe_route(x1, lw["wr"], k, self.eps)    # the prefill's sparse block on the fp8 stacks (its tables are sized per call)
            a = ops.moe_gemm_fp8(r["xg"], *w8["wgu"], r, nb, k, swiglu=True, row_norm=r["rn"], eps=self.eps)
            ops.moe_combine(x1, ops.moe_gemm_fp8(a, *w8["wd"], r, nb, k), r, self.eps, out=x)
            return r["ids"], r["wts"]
        if nb > self.MOE_FP8_ROWS:
            raise NotImplementedError(f"MoE (mixtral) decoder: fp8 expert weights are on (enable_moe_fp8): a batched step takes at most "
                                      f"{self.MOE_FP8_ROWS} sequences, got {nb}")
        if nb < self.MOE_GEMM_BATCH:
            ops.moe_route_rows(x1, lw["wr"], k, self.eps, ids, wts)
            ops.moe_gemv_batched_fp8(*w8["wgu"], x1, ids, swiglu=True, eps=self.eps, out=m["a"][:R])
            ops.moe_gemv_batched_fp8(*w8["wd"], m["a"][:R], ids, wts=wts, res=x1, out=x)
            return ids, wts
        t = dict(counts=m["counts"], offs=m["offs"], gather=m["gather"][:R], inv=m["inv"][:nb], wts=wts)
        ops.moe_route_rows(x1, lw["wr"], k, self.eps, ids, wts, tables=t)
        h = ops.rmsnorm(x1, self.w["ones"], self.eps, out=m["h"][:nb])              # (the norm weight is folded into wgu)
        ops.moe_gemm_skinny_fp8(h, *w8["wgu"], t, nb, k, m["part"], rowmap=t["gather"], swiglu=True, out=m["a"][:R])
        ops.moe_gemm_skinny_fp8(m["a"][:R], *w8["wd"], t, nb, k, m["part"], out=m["y"][:R])
        ops.moe_combine(x1, m["y"][:R], t, self.eps, out=x)
        return ids, wts

    def _token_block_batched_mxfp4(self, w4, lw, x, x1, nb, m, ids, wts):
        """The MoE block of a batched step on the MXFP4 expert copies: the rows kernels below MOE_GEMM_BATCH (a row is bit for bit the solo
        MXFP4 step), the grouped skinny-M GEMM from there to MOE_MXFP4_ROWS (the solo MXFP4 step up to summation order; more rows are
        refused); with enable_moe_mxfp4(tiled=True) the tiled W4A16 grouped GEMM from MOE_MXFP4_TILED_FROM on, for any nb (the same, up to
        summation order).  Returns the (ids, wts) the block routed with."""
        if self.moe_mxfp4_tiled and nb >= max(self.MOE_MXFP4_TILED_FROM, self.MOE_GEMM_BATCH):
            k = self.k
            r = ops.moe_route(x1, lw["wr"], k, self.eps)    # the prefill's sparse block on the MXFP4 stacks (its tables are sized per call)
            a = ops.moe_gemm_mxfp4(r["xg"], *w4["wgu"], r, nb, k, swiglu=True, row_norm=r["rn"], eps=self.eps)
            ops.moe_combine(x1, ops.moe_gemm_mxfp4(a, *w4["wd"], r, nb, k), r, self.eps, out=x)
            return r["ids"], r["wts"]
        if nb > self.MOE_MXFP4_ROWS:
            raise self._moe_mxfp4_limit(nb)
        k, R = self.k, nb * self.k
        if nb < self.MOE_GEMM_BATCH:
            ops.moe_route_rows(x1, lw["wr"], k, self.eps, ids, wts)
            ops.moe_gemv_batched_mxfp4(*w4["wgu"], x1, ids, swiglu=True, eps=self.eps, out=m["a"][:R])
            ops.moe_gemv_batched_mxfp4(*w4["wd"], m["a"][:R], ids, wts=wts, res=x1, out=x)
            return ids, wts
        t = dict(counts=m["counts"], offs=m["offs"], gather=m["gather"][:R], inv=m["inv"][:nb], wts=wts)
        ops.moe_route_rows(x1, lw["wr"], k, self.eps, ids, wts, tables=t)
        h = ops.rmsnorm(x1, self.w["ones"], self.eps, out=m["h"][:nb])              # (the norm weight is folded into wgu)
        ops.moe_gemm_skinny_mxfp4(h, *w4["wgu"], t, nb, k, m["part"], rowmap=t["gather"], swiglu=True, out=m["a"][:R])
        ops.moe_gemm_skinny_mxfp4(m["a"][:R], *w4["wd"], t, nb, k, m["part"], out=m["y"][:R])
        ops.moe_combine(x1, m["y"][:R], t, self.eps, out=x)
        return ids, wts

    def _token_block_batched(self, f, lw, o, x, x1, li=None):
        """The same for the nb rows of a batched step (enable_moe_batch), on the slot buffers' MoE tensors: x1 = x + o_proj(o) through the
        form, then one of three regimes by nb (class attributes MOE_GEMM_BATCH / MOE_SKINNY_ROWS).  No host read and, in the first two, no
        allocation: the step captures into one hipGraph per batch size."""
        nb, k, m = x.shape[0], self.k, self._bb["moe"]
        R = nb * k
        f.res(o, lw["wo"], x, out=x1)
        ids, wts = m["ids"][:nb], m["wts"][:nb]
        if self.moe_fp8:                         # (enable_moe_fp8: the 16-bit regimes below are untouched with the switch off)
            ids, wts = self._token_block_batched_fp8(self.w8moe[li], lw, x, x1, nb, m, ids, wts)
        elif self.moe_mxfp4:                     # (enable_moe_mxfp4: likewise)
            ids, wts = self._token_block_batched_mxfp4(self.w4moe[li], lw, x, x1, nb, m, ids, wts)
        elif nb < self.MOE_GEMM_BATCH:             # the solo step's GEMVs, a token index in the grid: every (token, slot) pair streams its expert
            ops.moe_route_rows(x1, lw["wr"], k, self.eps, ids, wts)
            ops.moe_gemv_batched(lw["wgu"], x1, ids, swiglu=True, eps=self.eps, out=m["a"][:R])
            ops.moe_gemv_batched(lw["wd"], m["a"][:R], ids, wts=wts, res=x1, out=x)
        elif nb <= self.MOE_SKINNY_ROWS:         # grouped skinny-M: an expert's weights stream once for all the rows routed to it
            t = dict(counts=m["counts"], offs=m["offs"], gather=m["gather"][:R], inv=m["inv"][:nb], wts=wts)
            ops.moe_route_rows(x1, lw["wr"], k, self.eps, ids, wts, tables=t)
            h = ops.rmsnorm(x1, self.w["ones"], self.eps, out=m["h"][:nb])          # (the norm weight is folded into wgu)
            ops.moe_gemm_skinny(h, lw["wgu"], t, nb, k, m["part"], rowmap=t["gather"], swiglu=True, out=m["a"][:R])
            ops.moe_gemm_skinny(m["a"][:R], lw["wd"], t, nb, k, m["part"], out=m["y"][:R])
            ops.moe_combine(x1, m["y"][:R], t, self.eps, out=x)
        else:                                    # the prefill's sparse block on the nb rows (its tables are sized per call)
            r = ops.moe_route(x1, lw["wr"], k, self.eps)
            a = ops.moe_gemm(r["xg"], lw["wgu"], r, nb, k, swiglu=True, row_norm=r["rn"], eps=self.eps)
            ops.moe_combine(x1, ops.moe_gemm(a, lw["wd"], r, nb, k), r, self.eps, out=x)
            ids, wts = r["ids"], r["wts"]
        self.last_route = dict(ids=ids, wts=wts)             # (of the last layer routed: tests follow the kernel's choice)


def make_decoder(cfg, *args, **kwargs):
    """The decoder class of the config's family: Mistral / Qwen2 (dense) or Mixtral (sparse MoE)."""
    cls = HipMixtralDecoder if cfg["llm"].get("family") == "mixtral" else HipMistralDecoder
    return cls(cfg, *args, **kwargs)
