// MXFP4 weights for the HBM-bound decode path: OCP Microscaling Formats v1.0 -- E2M1 elements (+-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, code bits
// s e e m), ONE E8M0 power-of-two scale per block of 32 consecutive k of a weight row: W[n][k] ~= 2^e(n, k / 32) * E2M1(q[n][k]), 4.25 bits per
// weight.  gfx950 reads the format natively: v_cvt_scalef32_pk_{bf16,f16}_fp4 turns one byte (two codes) and a scale into two 16-bit elements.
// Like the fp8 copies (k_fp8.h) this is an OPTIONAL arithmetic of the decode step (W4A16: activations stay 16-bit, fp32 sums); the reference has
// no such path, so the quantiser below IS the definition, restated in tests/mxfp4_oracle.py and held bit for bit against it.
//
// Storage: q [N, K / 2] bytes, byte j of a row = code of k = 2j in bits 3:0 and of k = 2j + 1 in bits 7:4 (the order the conversion instruction
// reads: result[0] from the low nibble); s [N, K / 32] bytes = e + 127.
//
//   quant_mxfp4_rows_kernel  : per block, amax = max|w|, e = floor(log2 amax) - 2 (the exponent field of amax, no log) clamped to [-127, 127],
//                              0 for a zero block; code = RNE of w * 2^-e onto the E2M1 grid, saturating at +-6 (OCP MX v1.0 section 6.3).
//                              The scaling is exact and the rounding is seven comparisons: reproducible bit for bit on any machine.
//   gemv_mxfp4_kernel        : y = W~ x for one token with the decode GEMVs' shared prologue and pair epilogue (k_decode.h gemv_stage_x,
//                              gemv_store_pair: fused RMSNorm, SwiGLU pairing, bias, residual, 16-bit / fp32 output).
//   gemv_mr_mxfp4_kernel     : 2..4 rows of x in one pass over q, every row bit for bit the single-row kernel (ONE body, MB a parameter).
//   gemm_skinny_mxfp4_kernel : M <= 64 rows on v_mfma_f32_16x16x32, the twin of gemm_skinny_fp8_kernel.
//
// THE SCALE RIDES IN THE CONVERSION in all of them: the element handed to v_dot2 / the MFMA is E2M1 * 2^e in the 16-bit element type.  bf16
// holds that product exactly (one significant bit pair, fp32's exponent range); IEEE half holds it exactly while it stays inside half's range
// (2^-24 .. 65504), which weights that were half to begin with do unless a block's maximum is below 2^-21.
#pragma once
#include "k_decode.h"
#include "k_skinny.h"

// byte B of dword w = two E2M1 codes -> two elements scaled by 2^(exponent of sc), packed like pack2bf (low nibble = low half)
template <int B>
__device__ __forceinline__ uint32_t mx4_cvt(uint32_t w, float sc) {
#ifdef VL2_ELEM_F16
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, B));
#else
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, B));
#endif
}
// an E8M0 byte as the fp32 whose exponent field the conversion reads (byte 0 = 2^-127 is a fp32 denormal: written as one)
__device__ __forceinline__ float mx4_scale(uint32_t sb) {
    return __builtin_bit_cast(float, sb ? sb << 23 : 0x00400000u);
}
// 8 codes (k .. k+7, one dword) -> the 8 elements of an MFMA fragment / four dot2 operands, in order
__device__ __forceinline__ u32x4 mx4_cvt8(uint32_t w, float sc) {
    return u32x4{mx4_cvt<0>(w, sc), mx4_cvt<1>(w, sc), mx4_cvt<2>(w, sc), mx4_cvt<3>(w, sc)};
}

// |v| (already scaled by 2^-e) -> E2M1 magnitude code, round to nearest, ties to the even code, saturating at 6 (code 7)
__device__ __forceinline__ uint32_t mx4_code(float v) {
    const float a = fabsf(v);
    const uint32_t c = a <= 0.25f ? 0u : a < 0.75f ? 1u : a <= 1.25f ? 2u : a < 1.75f ? 3u : a <= 2.5f ? 4u : a < 3.5f ? 5u : a <= 5.f ? 6u : 7u;
    return c | ((__builtin_bit_cast(uint32_t, v) >> 28) & 8u);
}

// grid = N rows, block 256.  w [N, ldw] 16-bit elements, q [N, ldq] bytes, s [N, lds] bytes, K % 32 == 0.  A lane owns 8 consecutive k, four
// lanes one block of 32.
__global__ __launch_bounds__(256) void quant_mxfp4_rows_kernel(const bf16_t* __restrict__ w, uint8_t* __restrict__ q, uint8_t* __restrict__ s,
                                                               int K, long ldw, long ldq, long lds) {
    const int tid = threadIdx.x;
    const bf16_t* row = w + (size_t)blockIdx.x * ldw;
    for (int k0 = 0; k0 < K; k0 += 2048) {               // uniform trip count: the four lanes of a block shuffle together
        const int k = k0 + tid * 8;
        const bool live = k < K;
        float v[8];
        unpack8(live ? *(const u32x4*)(row + k) : u32x4{0u, 0u, 0u, 0u}, v);
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
        amax = fmaxf(amax, __shfl_xor(amax, 1));
        amax = fmaxf(amax, __shfl_xor(amax, 2));
        // amax = 1.f * 2^x: floor(log2 amax) = x, the exponent field.  A denormal amax (only a bf16 denormal gets here) is below 2^-126:
        // x - 2 < -127 clamps.  4 * 2^e <= amax < 8 * 2^e unless clamped.
        const unsigned ab = __builtin_bit_cast(unsigned, amax);
        const int E = (int)((ab >> 23) & 0xffu);
        int e = E == 0 ? (ab ? -127 : 0) : E - 127 - 2;
        e = e < -127 ? -127 : (e > 127 ? 127 : e);
        const float inv = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);           // 2^-e: e = 127 -> 2^-127 cannot occur (amax < 2^128)
        if (live) {
            uint32_t o = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) o |= mx4_code(v[j] * inv) << (4 * j);
            *(uint32_t*)(q + (size_t)blockIdx.x * ldq + (k >> 1)) = o;
            if ((tid & 3) == 0) s[(size_t)blockIdx.x * lds + (k >> 5)] = (uint8_t)(e + 127);
        }
    }
}

struct Gemv4Args {
    const uint8_t* W;       // [N, ldw] bytes, two codes each (SWIGLU: packed blocks of 64 rows = 32 gate rows then 32 up rows, like the 16-bit layout)
    const uint8_t* scale;   // [N, lds] E8M0 bytes, one per 32 k
    const bf16_t* x;        // [K] (row 0 of [MB, ldx])
    const float* norm_w;    // fused RMSNorm prologue on x (or null)
    const bf16_t* res;      // [N_out] residual (or null)
    void* y;                // 16-bit or fp32 [N_out]
    int N, K, ldw, lds;
    float eps;
    const float* bias;      // [N_out] or null; not with SWIGLU
    int rms_plain;          // RMS-normalise x without a weight vector (folded into W before quantisation)
    int ldx, ldy, ldres;    // element strides between the rows of x / y / res (MB > 1)
};

// One 16-byte load per lane is 32 weights = exactly one scale block, so a lane's vector has ONE scale.  A wave owns NP PAIRS of weight rows per
// trip and keeps 16 vectors per lane (16 KiB per wave, gemv_fp8_kernel's footprint) in flight: rows of K <= 4096 are two vectors per lane, so
// NP = 4 (eight rows), longer rows NP = 1.  Pairs: gemv_pair_rows (k_decode.h; N even).
// x lives in LDS in the 16-bit element type as [MB][K], staged by gemv_stage_x like every decode GEMV's.  Per vector the 2 NP rows' dwords are
// converted once (v_cvt_scalef32_pk_*_fp4, the block scale in the conversion) and every x read from LDS serves all of them; each row's fp32 sum
// takes its products in k order whatever NP and MB are, so a row of the multi-row form is the single-row form bit for bit.
// grid = ceil(n_pairs / (4 NP)), block 256; dynamic LDS = MB * K * 2 bytes.  K % 32 == 0, MB * K <= 32704.
template <bool SWIGLU, bool OUT_F32, int NP, int MB>
__device__ __forceinline__ void gemv_mxfp4_body(const Gemv4Args& p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vl2_smem[];
    __shared__ float red[MB][4];
    bf16_t* xs = (bf16_t*)vl2_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_pairs = p.N / 2;
    const int nvec = p.K >> 5;                       // 16-B vectors (32 weights, one scale block) per row
    constexpr int SL = 8 / NP;                       // load slots per pair and pass
    const bool one_pass = nvec <= 64 * SL;
    u32x4 wv[8], uv[8];
    uint32_t ws[8], us[8];
    const int jp0 = (blockIdx.x * 4 + wave) * NP;    // this wave's first pair
    auto issue_rows = [&](int v0) {
#pragma unroll
        for (int pr = 0; pr < NP; ++pr) {
            int r0, r1;
            gemv_pair_rows<SWIGLU>(jp0 + pr, r0, r1);
            const bool live = jp0 + pr < n_pairs;
#pragma unroll
            for (int i = 0; i < SL; ++i) {
                const int v = v0 + i * 64 + lane;
                if (live && v < nvec) {
                    wv[pr * SL + i] = __builtin_nontemporal_load((const u32x4*)(p.W + (size_t)r0 * p.ldw + (size_t)v * 16));
                    uv[pr * SL + i] = __builtin_nontemporal_load((const u32x4*)(p.W + (size_t)r1 * p.ldw + (size_t)v * 16));
                    ws[pr * SL + i] = p.scale[(size_t)r0 * p.lds + v];
                    us[pr * SL + i] = p.scale[(size_t)r1 * p.lds + v];
                }
            }
        }
    };
    if (one_pass && jp0 < n_pairs) issue_rows(0);    // the weights do not depend on x: their latency overlaps the staging of x
    gemv_stage_x<MB>(p.x, p.ldx, p.norm_w, p.rms_plain, p.K, p.eps, xs, red);
    if (jp0 >= n_pairs) return;
    float a0[NP][MB], a1[NP][MB];
#pragma unroll
    for (int pr = 0; pr < NP; ++pr)
#pragma unroll
        for (int b = 0; b < MB; ++b) a0[pr][b] = a1[pr][b] = 0.f;
    for (int v0 = 0; v0 < nvec; v0 += 64 * SL) {
        if (!one_pass) issue_rows(v0);
#pragma unroll
        for (int i = 0; i < SL; ++i) {
            const int v = v0 + i * 64 + lane;
            if (v < nvec) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {        // dword q of the vector = k 8q .. 8q+7 of the block
                    u32x4 e0[NP], e1[NP];
#pragma unroll
                    for (int pr = 0; pr < NP; ++pr) {
                        e0[pr] = mx4_cvt8(wv[pr * SL + i][q], mx4_scale(ws[pr * SL + i]));
                        e1[pr] = mx4_cvt8(uv[pr * SL + i][q], mx4_scale(us[pr * SL + i]));
                    }
#pragma unroll
                    for (int b = 0; b < MB; ++b) {
                        const u32x4 xq = *(const u32x4*)(xs + (size_t)b * p.K + (size_t)v * 32 + 8 * q);
#pragma unroll
                        for (int pr = 0; pr < NP; ++pr) {
                            if (jp0 + pr >= n_pairs) continue;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                a0[pr][b] = dot2_bf16(e0[pr][j], xq[j], a0[pr][b]);
                                a1[pr][b] = dot2_bf16(e1[pr][j], xq[j], a1[pr][b]);
                            }
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int pr = 0; pr < NP; ++pr)
        if (jp0 + pr < n_pairs) gemv_store_pair<SWIGLU, OUT_F32, false, MB>(a0[pr], a1[pr], jp0 + pr, nullptr, p.bias, p.res, p.ldres, p.y, p.ldy);
}

template <bool SWIGLU, bool OUT_F32, int NP>
__global__ __launch_bounds__(256) void gemv_mxfp4_kernel(Gemv4Args p) { gemv_mxfp4_body<SWIGLU, OUT_F32, NP, 1>(p); }

template <bool SWIGLU, bool OUT_F32, int NP, int MB>
__global__ __launch_bounds__(256) void gemv_mr_mxfp4_kernel(Gemv4Args p) { gemv_mxfp4_body<SWIGLU, OUT_F32, NP, MB>(p); }

// ---- skinny-M GEMM on the MXFP4 weights (W4A16), 5..64 tokens per step:  C[M <= 64, N] = epilogue( A[M,K] . W~[N,K]^T ).
// gemm_skinny_body (k_skinny.h: gemm_skinny_kernel's grid, K split, x staging and MFMA sequence, WITH ITS LANE-TO-K ASSIGNMENT) behind the MXFP4
// weight policy: per 32-deep step a lane loads the 4 bytes
// that hold the 8 k of B[k = (lane>>4)*8 + j][n = lane&15] (they lie inside one scale block: one scale byte per load), converts them with the
// block scale to the element type and feeds v_mfma_f32_16x16x32.  The B operand is therefore the dequantised weight exactly, and the output is
// bit for bit gemm_skinny_kernel on dequant(q, s) provided the K split is the same -- the launcher picks it from N and K only.  The partials
// go through the workspace and skinny_reduce_kernel (unscaled form) in order.
struct Skinny4Args {
    const bf16_t* A;        // [M, lda]
    const uint8_t* Q;       // [N, ldq] bytes, two codes each
    const uint8_t* S;       // [N, lds] E8M0 bytes
    float* part;            // [KS][Mp][N] fp32 partial sums, Mp = 16 * MT
    int M, N, K, lda, ldq, lds;
    int kslice, kchunk;     // K per workgroup (multiple of kchunk), K per LDS chunk (multiple of 32)
};

// gemm_skinny_body's policy for the MXFP4 weights: 16 x (4 B of codes + the block's scale byte) in flight per lane
struct SkinnyWMx4 {
    using Args = Skinny4Args;
    static constexpr int NL = 16;
    struct word { uint32_t q, s; };                       // 8 codes and their block's scale byte
    const uint8_t *wrow, *srow;
    __device__ __forceinline__ SkinnyWMx4(const Args& p, int n, int k0, int lg)
        : wrow(p.Q + (size_t)n * p.ldq + (k0 >> 1) + lg * 4), srow(p.S + (size_t)n * p.lds + (k0 >> 5)) {}
    __device__ __forceinline__ word load(int kc, int s) const {
        return word{__builtin_nontemporal_load((const uint32_t*)(wrow + (kc >> 1) + s * 16)), srow[(kc >> 5) + s]};
    }
    static __device__ __forceinline__ bf16x8 frag(word w) { return __builtin_bit_cast(bf16x8, mx4_cvt8(w.q, mx4_scale(w.s))); }
    // the grouped form (k_moe_skinny.h, k_moe_mxfp4.h): expert e's codes and scales, q_stride / s_stride bytes apart
    static __device__ __forceinline__ void at_expert(Args& p, int e, long long q_stride, long long s_stride) {
        p.Q += (size_t)e * q_stride;
        p.S += (size_t)e * s_stride;
    }
};

template <int MT>
__global__ __launch_bounds__(256) void gemm_skinny_mxfp4_kernel(Skinny4Args p) { gemm_skinny_body<MT, SkinnyWMx4>(p); }
