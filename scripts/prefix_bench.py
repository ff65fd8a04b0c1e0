"""Turn 2 of a chat about one video: what the prefix cache saves.  Three measurements, HIP events, warm-up + repeats (median, min, max):
  1. 7B (VideoLLaMA2-7B, 16 frames, seeded random weights): time to the first token's logits of turn 2 with P ~= 1650 resident rows and
     n new rows -- the full path (tower + connector + splice + prefill of P + n rows) against the prefix path (embed n ids + extend);
  2. the same two decoder paths for the Mixtral-8x7B layer stack (weights generated on the device; no encoder: its cost is the dense one's);
  3. the attention alone: vl2_attn_append against vl2_attn_fwd(causal_off = P) on the Mistral shape (32 q heads, 8 kv heads).
Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), reps=reps)


def emit(rows, out, **kw):
    print(json.dumps(kw), flush=True)
    rows.append(kw)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


def bench_attention(rows, a):
    from videollama2_amd import ops
    nh, nkv, P, smax = 32, 8, a.prefix, 4096
    kc = (torch.randn(nkv, smax, 128, device="cuda")).bfloat16()
    vc = (torch.randn(nkv, smax, 128, device="cuda")).bfloat16()
    for n in a.rows:
        q = torch.randn(n, nh * 128, device="cuda").bfloat16()
        o = torch.empty_like(q)
        t_app = timed(lambda: ops.attn_append(q, kc, vc, o, P, nh, nkv, 128 ** -0.5), a.warmup, a.reps * 5)
        t_fwd = timed(lambda: ops.attn_fwd(q, kc, vc, o, (0, 128, nh * 128), (0, smax * 128, 128), (0, smax * 128, 128), (0, 128, nh * 128),
                                           1, nh, n, P + n, nh // nkv, 128 ** -0.5, True, P, 128), a.warmup, a.reps * 5)
        emit(rows, a.out, what="attention one layer", P=P, n=n, attn_append=t_app, attn_fwd_causal_off=t_fwd)


def bench_dense(rows, a):
    from videollama2_amd import _lib, ops
    from videollama2_amd.config import videollama2_7b
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.weights import random_state_dict
    import numpy as np
    T = 16
    cfg = videollama2_7b(T)
    sd = random_state_dict(cfg, "cuda", seed=1234)
    model = VideoLLaMA2Hip(cfg, sd, "cuda", max_seq_len=4096)
    del sd
    torch.cuda.empty_cache()
    side = cfg["vision"]["image_size"]
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (T, side, side, 3), dtype=np.uint8)).to("cuda")
    images = [(frames, "video")]
    V = cfg["llm"]["vocab_size"]
    n_vis = model.encode_images_or_videos(images)[0].shape[0]
    cg = torch.Generator().manual_seed(1)
    n_text = a.prefix - n_vis + 1                    # prompt of P rows: text | video | text
    base = [1] + torch.randint(3, V, (31,), generator=cg).tolist() + [-201] + torch.randint(3, V, (n_text - 32 - 1,), generator=cg).tolist()
    dec = model.decoder
    for n in a.rows:
        new = torch.randint(3, V, (n,), generator=cg).tolist()
        ids2 = torch.tensor([base + new], device="cuda")

        def full():
            _, _, _, emb, _ = model.prepare_inputs_labels_for_multimodal(ids2, None, None, None, images)
            dec.prefill(emb[0])

        _, _, _, emb1, _ = model.prepare_inputs_labels_for_multimodal(ids2[:, :len(base)], None, None, None, images)
        P = emb1.shape[1]
        dec.prefill(emb1[0])
        ids_new = torch.tensor(new, device="cuda", dtype=torch.int32)
        x_new = torch.empty((n, dec.D), dtype=_lib.elem_dtype(), device="cuda")

        def prefix():
            ops.embed_rows(ids_new, dec.w["embed"], x_new)
            dec.extend(x_new, start_pos=P)

        t_pre = timed(prefix, a.warmup, a.reps)
        t_full = timed(full, a.warmup, a.reps)
        emit(rows, a.out, what="7B turn-2 time to first logits", frames=T, P=P, n=n, full_reencode_prefill=t_full, prefix_extend=t_pre)
    del model
    torch.cuda.empty_cache()


def bench_moe(rows, a):
    from videollama2_amd.config import videollama2_8x7b
    from videollama2_amd.decoder import HipMixtralDecoder
    from videollama2_amd.weights import LazyRandomStateDict
    cfg = videollama2_8x7b(8)
    sd = LazyRandomStateDict(cfg, "cuda", seed=1234, n_llm_layers=a.moe_layers)
    dec = HipMixtralDecoder(cfg, sd, "cuda", max_seq_len=4096, n_layers=a.moe_layers)
    torch.cuda.synchronize()
    D, P = cfg["llm"]["hidden_size"], a.prefix
    for n in a.rows:
        x = (0.5 * torch.randn(P + n, D, device="cuda")).bfloat16()
        t_full = timed(lambda: dec.prefill(x), a.warmup, a.reps)
        dec.prefill(x[:P])
        t_pre = timed(lambda: dec.extend(x[P:], start_pos=P), a.warmup, a.reps)
        emit(rows, a.out, what="8x7B decoder turn-2 prefill", layers=a.moe_layers, P=P, n=n, full_prefill=t_full, prefix_extend=t_pre)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefix", type=int, default=1650)
    ap.add_argument("--rows", default="8,32,64,256")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--moe-layers", type=int, default=32)
    ap.add_argument("--only", default="attn,dense,moe")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.rows = [int(r) for r in a.rows.split(",")]
    rows = []
    only = a.only.split(",")
    if "attn" in only:
        bench_attention(rows, a)
    if "dense" in only:
        bench_dense(rows, a)
    if "moe" in only:
        bench_moe(rows, a)


if __name__ == "__main__":
    with torch.no_grad():
        main()
