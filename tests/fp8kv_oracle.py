"""TEST INFRASTRUCTURE ONLY -- the definition of the fp8 KV cache of the decode step (product: videollama2_amd/csrc/k_kv8.h, include/vl2hip.h
vl2_kv_quant / vl2_attn_decode_kv8).  The reference has no such path, so this file DEFINES it, out of the fp8 oracle that
is pinned to the OFP8 specification (oracle/fp8_oracle.py):

  format : per layer k8 / v8 = uint8 [nkv, smax, 128] e4m3fn codes, ks / vs = fp32 [nkv, smax] = 2^e, one per (kv head, position) row of 128
           elements, e = row_scale_exponent(amax(row)) -- `fp8_oracle.quant_rows` applied to the [nkv * rows, 128] view of the cache.
  decode : attention of one roped query over the dequantised rows code * 2^e (fp32).

Only tests may import this file (nothing under videollama2_amd/ does: tests/test_fp8kv_host.py)."""
import contextlib

import torch

from oracle import fp8_oracle as F8
from oracle import vl2_oracle as O

HD = 128


def quant_cache_rows(cache):
    """cache [nkv, rows, 128] (any float dtype, taken as it is) -> (codes uint8 [nkv, rows, 128], scales fp32 [nkv, rows])."""
    nkv, rows, hd = cache.shape
    assert hd == HD
    q, s = F8.quant_rows(cache.reshape(nkv * rows, hd))
    return q.view(nkv, rows, hd), s.view(nkv, rows)


def dequant_cache(q, s):
    """codes [nkv, rows, 128], scales [nkv, rows] -> fp32 [nkv, rows, 128] = code * 2^e."""
    q, s = q.cpu(), s.cpu()
    return F8.dequant(q.reshape(-1, HD), s.reshape(-1)).view(q.shape)


def qdq(cache):
    """quantise -> dequantise: what a cache row is worth once it has been through the format."""
    return dequant_cache(*quant_cache_rows(cache))


def rope_row(x, cos, sin):
    """x [heads, 128] fp32, cos / sin [64] fp32 (one position): rotate-half RoPE, HF apply_rotary_pos_emb."""
    x1, x2 = x[:, :64], x[:, 64:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], 1)


def attn_decode_ref(q, kd, vd, scale):
    """fp32 attention of one roped query q [nh, 128] over a dequantised cache kd / vd [nkv, ctx, 128] (GQA: head h reads kv head
    h // (nh / nkv)) -> [nh * 128]."""
    q, kd, vd = q.float().cpu(), kd.float().cpu(), vd.float().cpu()
    nh, nkv = q.shape[0], kd.shape[0]
    rep = nh // nkv
    out = []
    for h in range(nh):
        p = torch.softmax((kd[h // rep] @ q[h]) * scale, 0)
        out.append(p @ vd[h // rep])
    return torch.cat(out)


class _TorchWithQuantisedCacheCat:
    """`torch` as oracle/vl2_oracle.py sees it while `quantised_kv()` is active: everything is torch's own, except that the concatenation
    of a layer's cached rows with the new token's row (mistral_layer: torch.cat([kv[0], k], 1) on [nkv, S, 128] tensors) returns the rows as
    the fp8 cache holds them -- the new row is quantised before the attention reads it, the resident rows are already on the grid
    (quantise -> dequantise of a dequantised row is the identity in value)."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def cat(tensors, dim=0):
        out = torch.cat(tensors, dim)
        if dim == 1 and out.dim() == 3 and out.shape[-1] == HD:
            return qdq(out).to(out.dtype)
        return out


@contextlib.contextmanager
def quantised_kv():
    """Run oracle/vl2_oracle.py's decode (mistral_forward with caches) with its cached K/V rows passed through quantise -> dequantise.  A
    prefill (no caches) is untouched, as in the product: its attention reads the rows it has just computed; they are quantised when the
    first decode step concatenates them."""
    saved = O.torch
    O.torch = _TorchWithQuantisedCacheCat()
    try:
        yield
    finally:
        O.torch = saved


def teacher_forced_logits(sd, cfg, x, tokens, kv8):
    """The fp32 oracle's logits [len(tokens) + 1, V]: prefill of x [S, D], then one decode step per token of `tokens` (fed whatever the
    logits say).  kv8: the decode steps run on the quantised cache."""
    logits, caches = O.mistral_forward(sd, cfg, x, 0, None)
    rows, pos = [logits[0].float()], x.shape[0]
    ctx = quantised_kv() if kv8 else contextlib.nullcontext()
    with ctx:
        for t in tokens:
            e = torch.nn.functional.embedding(torch.tensor([int(t)]), sd["model.embed_tokens.weight"]).to(x.dtype)
            logits, caches = O.mistral_forward(sd, cfg, e, pos, caches)
            rows.append(logits[0].float())
            pos += 1
    return torch.stack(rows)
