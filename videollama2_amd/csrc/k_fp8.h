// fp8 weights for the HBM-bound decode path (the fp8 half of BASELINE.json configs[4]; the audio half has no source in the
// reference tree).  Format: OCP e4m3fn (what gfx950's conversion / MFMA instructions read -- NOT MI300X's fnuz), ONE fp32 scale per output
// row: W[n][k] ~= scale[n] * q[n][k].  Decode streams every weight once per token and is bound by that stream (61 % of
// 8 TB/s with bf16 weights), so halving the bytes is the lever; the activations stay in the 16-bit element type (W8A16), products and sums
// are fp32 exactly as in gemv_bf16_kernel.  The reference has no fp8 path ("needs a calibration story the reference does not have",
// SURVEY 8f-5): the quantiser below IS the definition, restated in oracle/fp8_oracle.py and held bit for bit against it.
//
//   quant_fp8_rows_kernel : row n of a 16-bit weight matrix -> scale[n] = 2^e, e the smallest integer with max|w[n][:]| <= 448 * 2^e (a
//                           power of two, as the hardware's own MX block scales are: applying and removing it is EXACT, so the quantiser is
//                           reproducible bit for bit on any machine -- no division, whose fast-math lowering on the GPU is a reciprocal);
//                           q = RNE_e4m3fn(w * 2^-e).  A zero (or denormal-only) row gets scale 1.
//   gemv_fp8_kernel       : y = scale * (q x) (+ bias) (+ res) for one token; the fused RMSNorm prologue of gemv_bf16_kernel (k_decode.h
//                           gemv_stage_x: x staged in LDS in the 16-bit element type), SwiGLU pairing and residual epilogue
//   gemv_mr_fp8_kernel    : 2..4 rows of x in one pass over q, every row bit for bit the single-row kernel (ONE body, MB a parameter)
#pragma once
#include "k_decode.h"

typedef float vl2_f32x2_t __attribute__((ext_vector_type(2)));
#ifndef VL2_CVT_PK_F32_FP8                      // two e4m3fn bytes of a dword -> two floats (v_cvt_pk_f32_fp8; the CPU test build defines its own)
#define VL2_CVT_PK_F32_FP8(w, hi) __builtin_amdgcn_cvt_pk_f32_fp8((int)(w), (hi))
#define VL2_CVT_PK_FP8_F32(a, b, old, hi) __builtin_amdgcn_cvt_pk_fp8_f32((a), (b), (old), (hi))
#endif

// ---- THE per-row arithmetic of every e4m3fn quantiser here (weight rows, activation rows, KV-cache rows in k_kv8.h): one copy, so they
// agree to the bit.  Scale: 448 = 1.75 * 2^8: amax = 1.f * 2^x  ->  e = x - 8 (+1 if 1.f > 1.75), clamped to [-100, 100]; sc = 2^e and
// inv = 2^-e are exact floats (a zero or denormal-only row: e = 0).
__device__ __forceinline__ void fp8_row_scale(float amax, float& sc, float& inv) {
    const unsigned ab = __builtin_bit_cast(unsigned, amax);
    const int E = (int)((ab >> 23) & 0xffu);
    int e = E == 0 ? 0 : (E - 127) - 8 + ((ab & 0x7fffffu) > 0x600000u ? 1 : 0);
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    sc = __builtin_bit_cast(float, (unsigned)(127 + e) << 23);
    inv = __builtin_bit_cast(float, (unsigned)(127 - e) << 23);
}
// two values -> two e4m3fn bytes (bits 15:0): RNE of v * inv (v_cvt_pk_fp8_f32)
__device__ __forceinline__ unsigned fp8_quant2(float v0, float v1, float inv) {
    return (unsigned)VL2_CVT_PK_FP8_F32(v0 * inv, v1 * inv, 0, false) & 0xffffu;
}
// eight consecutive values -> eight e4m3fn bytes
__device__ __forceinline__ u32x2 fp8_quant8(const float* v, float inv) {
    int lo = 0, hi = 0;
    lo = VL2_CVT_PK_FP8_F32(v[0] * inv, v[1] * inv, lo, false);
    lo = VL2_CVT_PK_FP8_F32(v[2] * inv, v[3] * inv, lo, true);
    hi = VL2_CVT_PK_FP8_F32(v[4] * inv, v[5] * inv, hi, false);
    hi = VL2_CVT_PK_FP8_F32(v[6] * inv, v[7] * inv, hi, true);
    return u32x2{(unsigned)lo, (unsigned)hi};
}

// grid = N rows, block 256.  w [N, ldw] 16-bit elements, q [N, K] bytes (K % 16 == 0), scale [N] fp32.
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(const bf16_t* __restrict__ w, uint8_t* __restrict__ q, float* __restrict__ scale,
                                                             int K, long ldw) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bf16_t* row = w + (size_t)blockIdx.x * ldw;
    float amax = 0.f;
    for (int k = tid * 8; k < K; k += 2048) {
        float v[8];
        unpack8(*(const u32x4*)(row + k), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
    }
    amax = wave_max(amax);
    if (lane == 0) red[wave] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sc, inv;
    fp8_row_scale(amax, sc, inv);
    if (tid == 0) scale[blockIdx.x] = sc;
    uint8_t* qrow = q + (size_t)blockIdx.x * K;
    for (int k = tid * 8; k < K; k += 2048) {
        float v[8];
        unpack8(*(const u32x4*)(row + k), v);
        *(u32x2*)(qrow + k) = fp8_quant8(v, inv);
    }
}

// ---- fp8 ACTIVATIONS for the prefill GEMMs on the fp8 matrix pipe (VL2_GEMM_FP8: v_mfma_f32_32x32x64_f8f6f4, k_gemm.h gemm3 / gemm4 FP8):
// row m of a 16-bit activation -> e4m3fn bytes with the same power-of-two row scale rule as the weights (sa[m] = 2^e, e the smallest integer
// with max|x[m][:]| <= 448 * 2^e; exact to apply and to remove), and the row's entry of the GEMM's row table (GemmArgs.row_norm, [M][2]):
// (0, sa[m]) or, for an RMS-norm-carrying GEMM (HF:modeling_mistral.py:46-48 with the weight folded into W), (0, sa[m] * rsqrt(mean x^2 + eps))
// -- the quantiser reads the whole row anyway, so the norm needs no statistics from the producer.  grid = M rows, block 256, K % 16 == 0.
__global__ __launch_bounds__(256) void quant_act_fp8_kernel(const bf16_t* __restrict__ x, long ldx, uint8_t* __restrict__ q, long ldq,
                                                            float* __restrict__ rowtab, int K, int rms, float eps) {
#pragma clang fp reassociate(off)
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bf16_t* row = x + (size_t)blockIdx.x * ldx;
    float amax = 0.f, ss = 0.f;
    for (int k = tid * 8; k < K; k += 2048) {
        float v[8];
        unpack8(*(const u32x4*)(row + k), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) { amax = fmaxf(amax, fabsf(v[j])); ss = __builtin_fmaf(v[j], v[j], ss); }
    }
    amax = wave_max(amax);
    ss = wave_sum(ss);
    if (lane == 0) { red[wave] = amax; red[4 + wave] = ss; }
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    ss = (red[4] + red[5]) + (red[6] + red[7]);
    float sc, inv;
    fp8_row_scale(amax, sc, inv);
    if (tid == 0) {
        rowtab[2 * (size_t)blockIdx.x] = 0.f;
        rowtab[2 * (size_t)blockIdx.x + 1] = rms ? sc * rsqrtf(ss / (float)K + eps) : sc;
    }
    uint8_t* qrow = q + (size_t)blockIdx.x * ldq;
    for (int k = tid * 8; k < K; k += 2048) {
        float v[8];
        unpack8(*(const u32x4*)(row + k), v);
        *(u32x2*)(qrow + k) = fp8_quant8(v, inv);
    }
}

struct Gemv8Args {
    const uint8_t* W;       // [N, ldw] e4m3fn bytes (SWIGLU: packed blocks of 64 rows = 32 gate rows then 32 up rows, like the 16-bit layout)
    const float* scale;     // [N] one per (packed) row
    const bf16_t* x;        // [K] (row 0 of [MB, ldx])
    const float* norm_w;    // fused RMSNorm prologue on x (or null)
    const bf16_t* res;      // [N_out] residual (or null)
    void* y;                // 16-bit or fp32 [N_out]
    int N, K, ldw;
    float eps;
    const float* bias;      // [N_out] or null; not with SWIGLU
    int rms_plain;          // RMS-normalise x without a weight vector (folded into W before quantisation)
    int ldx, ldy, ldres;    // element strides between the rows of x / y / res (MB > 1)
};

// ONE body, MB = rows of x per pass a parameter: gemv_fp8_kernel is MB = 1, gemv_mr_fp8_kernel MB = 2..4 (batched decode: y[b][:] = scale *
// (q x[b]) (+ bias) (+ res[b]) in one pass over q -- what gemv_mr_bf16_kernel is to gemv_bf16_kernel).
// A wave owns NP PAIRS of weight rows per trip and keeps all their loads in flight: 8 x 16 B per lane and row array = 16 KiB per wave,
// the 16-bit kernel's SwiGLU footprint -- the stream is bound by bytes in flight, so rows of K <= 4096 (four 16-B vectors per lane) run
// two pairs at a time (NP = 2), longer rows one.  Pairs: gemv_pair_rows (N even).  x lives in LDS in the 16-bit element type as [MB][K], staged
// by gemv_stage_x; a weight dword becomes two packed element pairs ONCE (v_cvt_pk_f32_fp8 + the pack: every e4m3fn value is exact in bf16 and
// in half) and meets the MB x vectors it serves in v_dot2: fp32 sums.  Each row's sum takes its products in the same order -- the per-lane
// walk over the 16-B weight vectors (lane, lane + 64, ...), the dot2 sequence per pair row -- whatever NP and MB are, and the prologue and
// epilogue are the shared ones, so a row of the multi-row form is the single-row form bit for bit.
// grid = ceil(n_pairs / (4 NP)), block 256; dynamic LDS = MB * K * 2 bytes (<= 64 KiB: the launcher splits larger batches).
// K % 16 == 0, K <= 32704; NP = 2 needs K <= 4096.
template <bool SWIGLU, bool OUT_F32, int NP, int MB>
__device__ __forceinline__ void gemv_fp8_body(const Gemv8Args& p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vl2_smem[];
    __shared__ float red[MB][4];
    bf16_t* xs = (bf16_t*)vl2_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_pairs = p.N / 2;
    const int nvec = p.K >> 4;                       // 16-B vectors (16 weights) per row
    constexpr int SL = 8 / NP;                       // load slots per pair and pass
    const bool one_pass = nvec <= 64 * SL;
    u32x4 wv[8], uv[8];
    const int jp0 = (blockIdx.x * 4 + wave) * NP;    // this wave's first pair
    auto issue_rows = [&](int v0) {
#pragma unroll
        for (int pr = 0; pr < NP; ++pr) {
            int r0, r1;
            gemv_pair_rows<SWIGLU>(jp0 + pr, r0, r1);
            const uint8_t* w0p = p.W + (size_t)r0 * p.ldw;
            const uint8_t* w1p = p.W + (size_t)r1 * p.ldw;
            const bool live = jp0 + pr < n_pairs;
#pragma unroll
            for (int i = 0; i < SL; ++i) {
                const int v = v0 + i * 64 + lane;
                if (live && v < nvec) {
                    wv[pr * SL + i] = __builtin_nontemporal_load((const u32x4*)(w0p + (size_t)v * 16));
                    uv[pr * SL + i] = __builtin_nontemporal_load((const u32x4*)(w1p + (size_t)v * 16));
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
        for (int pr = 0; pr < NP; ++pr) {
            if (jp0 + pr >= n_pairs) continue;
#pragma unroll
            for (int i = 0; i < SL; ++i) {
                const int v = v0 + i * 64 + lane;
                if (v < nvec) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const vl2_f32x2_t w0l = VL2_CVT_PK_F32_FP8(wv[pr * SL + i][q], false), w0h = VL2_CVT_PK_F32_FP8(wv[pr * SL + i][q], true);
                        const vl2_f32x2_t w1l = VL2_CVT_PK_F32_FP8(uv[pr * SL + i][q], false), w1h = VL2_CVT_PK_F32_FP8(uv[pr * SL + i][q], true);
                        const uint32_t e0l = pack2bf(w0l[0], w0l[1]), e0h = pack2bf(w0h[0], w0h[1]);
                        const uint32_t e1l = pack2bf(w1l[0], w1l[1]), e1h = pack2bf(w1h[0], w1h[1]);
#pragma unroll
                        for (int b = 0; b < MB; ++b) {
                            const u32x2 xq = *(const u32x2*)(xs + (size_t)b * p.K + (size_t)v * 16 + 4 * q);
                            a0[pr][b] = dot2_bf16(e0l, xq[0], a0[pr][b]);
                            a1[pr][b] = dot2_bf16(e1l, xq[0], a1[pr][b]);
                            a0[pr][b] = dot2_bf16(e0h, xq[1], a0[pr][b]);
                            a1[pr][b] = dot2_bf16(e1h, xq[1], a1[pr][b]);
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int pr = 0; pr < NP; ++pr)
        if (jp0 + pr < n_pairs) gemv_store_pair<SWIGLU, OUT_F32, true, MB>(a0[pr], a1[pr], jp0 + pr, p.scale, p.bias, p.res, p.ldres, p.y, p.ldy);
}

template <bool SWIGLU, bool OUT_F32, int NP>
__global__ __launch_bounds__(256) void gemv_fp8_kernel(Gemv8Args p) { gemv_fp8_body<SWIGLU, OUT_F32, NP, 1>(p); }

template <bool SWIGLU, bool OUT_F32, int NP, int MB>
__global__ __launch_bounds__(256) void gemv_mr_fp8_kernel(Gemv8Args p) { gemv_fp8_body<SWIGLU, OUT_F32, NP, MB>(p); }
