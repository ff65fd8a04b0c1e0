"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the MXFP4 weight format of the optional decode path (product: videollama2_amd/csrc/k_mxfp4.h,
include/vl2hip.h vl2_pack_quant_mxfp4 / vl2_gemv_mxfp4 / vl2_gemm_skinny_mxfp4).

The reference has no 4-bit path of this kind, so this file DEFINES the arithmetic; the kernels are held bit for bit (quantiser) / to fp32
summation order (GEMV) against it.  What it is pinned to instead: OCP Microscaling Formats (MX) v1.0 -- the E2M1 element (section 5.3.3: bias 1,
no infinities, no NaN, values +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, code bits s e e m), the E8M0 scale (section 5.4.1: 2^(byte - 127), 0xFF = NaN, never
written here) and the conversion of section 6.3: per block of 32, shared exponent = floor(log2(max|v|)) - emax_elem with emax_elem = 2, elements
rounded to nearest even and clamped to the largest normal.  The scale bytes are also checked against PyTorch's own `torch.float8_e8m0fnu`
(tests/test_mxfp4.py).

Layout: q [N, K / 2] uint8, byte j of a row holds k = 2j in bits 3:0 and k = 2j + 1 in bits 7:4 (PyTorch's `float4_e2m1fn_x2` order);
s [N, K / 32] uint8.  Dequantised weight: W~[n, k] = 2^(s[n, k // 32] - 127) * E2M1(q[n, k]) -- THE SCALE RIDES IN THE CONVERSION: the kernels hand
E2M1 * 2^e to the dot product as one 16-bit element (exact in bf16; exact in half inside half's range), so `gemv` below multiplies x by the
dequantised weights; it does not scale per-block partial sums (the two are the same real number, and the same fp64 number here).

Nothing under videollama2_amd/ imports this file."""
import math

import torch

E2M1_VALUES = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
BLOCK = 32
EMAX_ELEM = 2                                   # exponent of the largest E2M1 normal (6 = 1.5 * 2^2)


def e2m1_decode(code):
    """One 4-bit code -> float (s e e m)."""
    v = E2M1_VALUES[code & 7]
    return -v if code & 8 else v


def e2m1_encode(x):
    """float -> 4-bit code: round to nearest, ties to the even code (even mantissa bit), saturating at +-6.  The sign bit is the sign of x
    (a negative value that rounds to zero keeps it)."""
    s = 8 if math.copysign(1.0, x) < 0 else 0
    a = abs(x)
    best, bd = 0, None
    for c in range(8):                          # the 8 magnitudes are monotone: nearest value, ties to the even code
        d = abs(E2M1_VALUES[c] - a)
        if bd is None or d < bd or (d == bd and c % 2 == 0):
            best, bd = c, d
    return s | best


def block_exponent(amax):
    """amax [...] (float, >= 0) -> e = floor(log2(amax)) - 2 clamped to [-127, 127]; 0 where amax == 0.  frexp: amax = m * 2^x, m in
    [0.5, 1), so floor(log2(amax)) = x - 1 -- exact for denormals too."""
    amax = amax.double()
    _, x = torch.frexp(amax)
    e = (x.to(torch.int64) - 1 - EMAX_ELEM).clamp(-127, 127)
    return torch.where(amax == 0, torch.zeros_like(e), e)


def encode_tensor(v):
    """v (already scaled by 2^-e, float64) -> codes uint8, `e2m1_encode` vectorised: thresholds are the midpoints, ties to the even code."""
    a = v.abs()
    c = torch.zeros(v.shape, dtype=torch.uint8)
    # midpoint, and whether the midpoint itself rounds UP (to the even code above)
    for code, (mid, up) in enumerate([(0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False)], start=1):
        c = torch.where((a >= mid) if up else (a > mid), torch.full_like(c, code), c)
    return c | (torch.signbit(v).to(torch.uint8) << 3)


def quant_blocks(w):
    """w [N, K] (any float dtype; values taken as they are), K % 32 == 0 -> (q uint8 [N, K / 2], s uint8 [N, K / 32])."""
    wf = w.detach().cpu().double()
    N, K = wf.shape
    assert K % BLOCK == 0
    blk = wf.view(N, K // BLOCK, BLOCK)
    e = block_exponent(blk.abs().amax(dim=2))
    codes = encode_tensor(blk * torch.exp2(-e.double())[:, :, None]).view(N, K)        # the scaling is exact (a power of two)
    q = codes[:, 0::2] | (codes[:, 1::2] << 4)
    return q.contiguous(), (e + 127).to(torch.uint8)


def dequant(q, s):
    """(q [N, K / 2], s [N, K / 32]) -> fp32 [N, K] (every value is exact in fp32, and in bf16)."""
    q, s = q.cpu(), s.cpu()
    N = q.shape[0]
    tab = torch.tensor([e2m1_decode(c) for c in range(16)], dtype=torch.float64)
    codes = torch.stack([q & 15, q >> 4], dim=2).view(N, -1).long()
    sc = torch.exp2(s.double() - 127.0).repeat_interleave(BLOCK, dim=1)
    return (tab[codes] * sc).float()


def gemv(q, s, x, norm_w=None, eps=1e-5, res=None, bias=None, swiglu=False, rms=False, elem=torch.bfloat16):
    """y = W~ x (+ bias) (+ res) in fp64, W~ = dequant(q, s) (the block scale inside the weight, see the module docstring), x [K] in the 16-bit
    element type.  rms / norm_w: MistralRMSNorm on x first, its output rounded to the element type (HF:modeling_mistral.py:46-48).  swiglu: rows
    in blocks of 64 = 32 gate rows then 32 up rows.  The options of oracle/fp8_oracle.py gemv."""
    xf = x.detach().float().cpu()
    if rms or norm_w is not None:
        xf = xf * torch.rsqrt((xf * xf).mean() + eps)
        if norm_w is not None:
            xf = xf * norm_w.float().cpu()
        xf = xf.to(elem).float()
    y = dequant(q, s).double() @ xf.double()
    if swiglu:
        y = y.view(-1, 2, 32)
        g, u = y[:, 0].reshape(-1), y[:, 1].reshape(-1)
        y = torch.nn.functional.silu(g) * u
    if bias is not None:
        y = y + bias.double().cpu()
    if res is not None:
        y = y + res.double().cpu()
    return y
