"""Hashes of the outputs of every decode-projection entry point (GEMV, multi-row GEMV, skinny-M GEMM; 16-bit, fp8 and MXFP4 weights) on
seeded inputs: the decode shapes of scripts/mxfp4_bench.py, M in {1, 2, 3, 4, 5, 8, 16, 17, 33, 64}, every epilogue an entry supports (plain,
bias, residual, SwiGLU, fp32 output), with and without the fused RMSNorm (weighted and plain).  Two builds of the library that compute the same
bits print the same file.

    python scripts/decode_bits.py --out hashes.json"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.mxfp4_bench import SHAPES  # noqa: E402

MS = (1, 2, 3, 4, 5, 8, 16, 17, 33, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    from videollama2_amd import ops
    from videollama2_amd.weights import pack_gate_up
    g = torch.Generator(device="cuda").manual_seed(1234)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, device="cuda", generator=g) * scale)
    out = {}

    def put(key, t):
        torch.cuda.synchronize()
        out[key] = hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:24]

    for name, N, K, _ in SHAPES:
        w = rnd(N, K, scale=K ** -0.5).bfloat16()
        wgu = pack_gate_up(w[:N // 2].contiguous(), w[N // 2:].contiguous())
        W = {False: (w, ops.quant_fp8(w), ops.quant_mxfp4(w)), True: (wgu, ops.quant_fp8(wgu), ops.quant_mxfp4(wgu))}
        nw, bias = 1 + 0.1 * rnd(K), rnd(N)
        for M in MS:
            x = rnd(M, K).bfloat16()
            for sw in (False, True):
                n_out = N // 2 if sw else N
                res = rnd(M, n_out).bfloat16()
                w16, (q8, s8), (q4, s4) = W[sw]
                epis = [("plain", {}), ("res", dict(res=res))] if sw else \
                       [("plain", {}), ("bias", dict(bias=bias)), ("res", dict(res=res)), ("f32", dict(out_f32=True)), ("bias_res_f32", dict(bias=bias, res=res, out_f32=True))]
                for en, ek in epis:
                    tag = f"{name}/M{M}/{'swiglu' if sw else 'rows'}/{en}"
                    put(f"skinny16/{tag}", ops.gemm_skinny(x, w16, swiglu=sw, **ek))
                    put(f"skinny8/{tag}", ops.gemm_skinny_fp8(x, q8, s8, swiglu=sw, **ek))
                    put(f"skinny4/{tag}", ops.gemm_skinny_mxfp4(x, q4, s4, swiglu=sw, **ek))
                    for nn, nk in (("nonorm", {}), ("norm_w", dict(norm_w=nw, eps=1e-5)), ("rms_plain", dict(rms_plain=True, eps=1e-5))):
                        if nn != "rms_plain":
                            put(f"gemvb16/{tag}/{nn}", ops.gemv_batched(w16, x, swiglu=sw, **ek, **nk))
                        put(f"gemvb8/{tag}/{nn}", ops.gemv_batched_fp8(q8, s8, x, swiglu=sw, **ek, **nk))
                        put(f"gemvb4/{tag}/{nn}", ops.gemv_batched_mxfp4(q4, s4, x, swiglu=sw, **ek, **nk))
                        if M == 1:
                            e1 = {k: (v[0] if k == "res" else v) for k, v in ek.items()}
                            if nn != "rms_plain":
                                put(f"gemv16/{tag}/{nn}", ops.gemv(w16, x[0], swiglu=sw, **e1, **nk))
                            put(f"gemv8/{tag}/{nn}", ops.gemv_fp8(q8, s8, x[0], swiglu=sw, **e1, **nk))
                            put(f"gemv4/{tag}/{nn}", ops.gemv_mxfp4(q4, s4, x[0], swiglu=sw, **e1, **nk))
        del W, w, wgu
        torch.cuda.empty_cache()
    h = hashlib.sha256(json.dumps(out, sort_keys=True).encode()).hexdigest()
    with open(a.out, "w") as f:
        json.dump(dict(cases=len(out), digest=h, hashes=out), f, indent=0, sort_keys=True)
    print(json.dumps(dict(cases=len(out), digest=h)))


if __name__ == "__main__":
    main()
