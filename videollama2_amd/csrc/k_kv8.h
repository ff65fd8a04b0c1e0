// fp8 KV cache for the decode step.  A batched decode step reads every resident K/V row once per layer; at 64 requests
// of context 1650 that is as many bytes as the 16-bit weights, and nothing else in the step is that large once the weights are fp8 or MXFP4.
// Format, per layer: k8 / v8 = uint8 [nkv, smax, 128] e4m3fn codes, ks / vs = fp32 [nkv, smax] -- ONE power-of-two scale 2^e per (kv head,
// position) row of 128 elements, K and V apart, e = the smallest integer with max|row| <= 448 * 2^e: the rule and the arithmetic of the weight
// rows (k_fp8.h fp8_row_scale / fp8_quant8; oracle/fp8_oracle.py quant_rows).  What is quantised is the 16-bit cache row as the 16-bit path
// stores it: K after RoPE and rounded to the element type, V as the projection wrote it.  head_dim 128.
//
//   kv_quant_rows_kernel   : rows [p0, p1) of one sequence's 16-bit K and V caches -> codes and scales at the same rows (after a prefill).
//   attn_decode_kv8_kernel : attn_decode_kernel<false> (k_decode.h) on this cache: same grid, 64-key slices and {m, l, o[128]} partials
//                            (attn_decode_combine_kernel consumes them unchanged), the new token's row quantised on its way in.
// Bits (bf16 build): code * 2^e is exact in bf16 (e4m3fn has 4 significant bits, |e| <= 100), and the kernel hands attn_slice_compute those
// values in the 16-bit kernel's lane layout -- so its output IS vl2_attn_decode's on the dequantised cache, for any resident rows and any q.
// (Both kernels append the new row first and the 16-bit one appends it unquantised: the outputs are equal when that row is on the fp8 grid
// and otherwise differ by exactly its quantisation.  fp16 build: code * 2^e is rounded to half where it is not a half number; equal to
// tolerance only.)
#pragma once
#include "k_decode.h"
#include "k_fp8.h"

// grid = ceil(2 * nkv * (p1 - p0) / 16), block 256: 16 lanes per row (16 B of the 16-bit row in, 8 code bytes out per lane), 16 rows per
// workgroup; rows are numbered K rows first (kv head major), then V rows.  Writes codes and scales of rows [p0, p1) only.
__global__ __launch_bounds__(256) void kv_quant_rows_kernel(const bf16_t* __restrict__ k16, const bf16_t* __restrict__ v16, uint8_t* __restrict__ k8,
                                                            uint8_t* __restrict__ v8, float* __restrict__ ks, float* __restrict__ vs, int nkv, int smax,
                                                            int p0, int p1) {
    constexpr int HD = 128;
    const int n = p1 - p0;
    const long nrows = 2L * nkv * n;
    const long r = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    const bool live = r < nrows;                           // (a dead row keeps its lanes for the shuffles below)
    const long rr = live ? r : nrows - 1;
    const bool isv = rr >= (long)nkv * n;
    const long rk = isv ? rr - (long)nkv * n : rr;
    const size_t row = (size_t)(rk / n) * smax + p0 + (int)(rk % n);          // (kv head, position)
    float v[8];
    unpack8(*(const u32x4*)((isv ? v16 : k16) + row * HD + sub * 8), v);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
#pragma unroll
    for (int msk = 8; msk >= 1; msk >>= 1) amax = fmaxf(amax, __shfl_xor(amax, msk));        // over the row's 16 lanes
    float sc, inv;
    fp8_row_scale(amax, sc, inv);
    if (!live) return;
    *(u32x2*)((isv ? v8 : k8) + row * HD + sub * 8) = fp8_quant8(v, inv);
    if (sub == 0) (isv ? vs : ks)[row] = sc;
}

// four e4m3fn codes of a dword, times the row's power-of-two scale, as two packed pairs of 16-bit elements
__device__ __forceinline__ u32x2 kv8_dequant4(uint32_t w, float sc) {
    const vl2_f32x2_t a = VL2_CVT_PK_F32_FP8(w, false), b = VL2_CVT_PK_F32_FP8(w, true);
    return u32x2{pack2bf(a[0] * sc, a[1] * sc), pack2bf(b[0] * sc, b[1] * sc)};
}

// grid = (nsplit_cap, nkv * sequences, ceil(group/4)), block 256 -- attn_decode_kernel<false>'s launch, arguments and early exits; the
// caches are the fp8 ones: sequence b's codes at k8 / v8 + b * cache_bs (bytes), its scales at ks / vs + b * scale_bs (floats).
// A lane is (key = lane & 15, head-in-block = lane >> 4) for K, as in the 16-bit kernel: it reads its key's 128-B row as 8 x 16 B and its
// key's two scales once.  V: the wave's 16 rows are 2 KiB in a row; lane l reads the dword at dims 4 (l & 31) .. + 3 of key 2 j + (l >> 5) in
// load j (8 loads of 4 B per lane, each 256 contiguous bytes per wave) and the pair (2 l, 2 l + 1) that attn_slice_compute wants from it
// comes from the lane that holds it (ds_bpermute), scaled by that key's scale (v_readlane).
__global__ __launch_bounds__(256) void attn_decode_kv8_kernel(const bf16_t* __restrict__ qkv, uint8_t* __restrict__ k8, uint8_t* __restrict__ v8,
                                                              float* __restrict__ ks, float* __restrict__ vs, const float* __restrict__ cos_t,
                                                              const float* __restrict__ sin_t, float* __restrict__ partial, int nh, int group,
                                                              int nkv, int smax, int pos_arg, const int* __restrict__ pos_dev, float scale_log2e,
                                                              long qkv_bs, long cache_bs, long scale_bs, long partial_bs) {
    constexpr int HD = 128, HALF = 64;
    __shared__ AttnSliceSmem sm;
    auto& qs = sm.qs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kl = lane & 15;
    const int split = blockIdx.x, hk = (int)blockIdx.y % nkv, bseq = (int)blockIdx.y / nkv, nsplit = gridDim.x;
    const int h0 = blockIdx.z * 4;
    const int ng = group - h0 < 4 ? group - h0 : 4;
    const int pos = pos_dev ? pos_dev[bseq] : pos_arg;
    qkv += (size_t)bseq * qkv_bs;
    partial += (size_t)bseq * partial_bs;
    if (pos >= smax) return;                               // a device-side position past the cache: touch nothing (see attn_decode_kernel)
    const int ctx = pos + 1;
    const int k0 = split * 64;
    if (k0 >= ctx) return;
    uint8_t* Kb = k8 + (size_t)bseq * cache_bs + (size_t)hk * smax * HD;
    uint8_t* Vb = v8 + (size_t)bseq * cache_bs + (size_t)hk * smax * HD;
    float* Ks = ks + (size_t)bseq * scale_bs + (size_t)hk * smax;
    float* Vs = vs + (size_t)bseq * scale_bs + (size_t)hk * smax;
    const float* cp = cos_t + (size_t)pos * HALF;
    const float* sp = sin_t + (size_t)pos * HALF;

    // roped q of this block's heads -> LDS, rounded through the element type (attn_decode_kernel's lines)
    for (int t = tid; t < ng * HALF; t += 256) {
        const int h = t / HALF, d = t % HALF;
        const bf16_t* qh = qkv + (size_t)(hk * group + h0 + h) * HD;
        float o1, o2;
        rope_pair(bf2f(qh[d]), bf2f(qh[d + HALF]), cp[d], sp[d], o1, o2);
        qs[h][d] = bf2f(f2bf(o1));
        qs[h][d + HALF] = bf2f(f2bf(o2));
    }
    // the slice that owns the new position: rope k_new, round it through the element type (the row the 16-bit kernel stores), quantise that
    // row and v_new's with the rows' own scales and append codes and scales, before anyone reads row `pos`.  One wave: lane d holds (d, d + 64).
    if (pos >= k0 && pos < k0 + 64 && tid < HALF) {
        const bf16_t* kn = qkv + (size_t)(nh + hk) * HD;
        const bf16_t* vn = qkv + (size_t)(nh + nkv + hk) * HD;
        float o1, o2;
        rope_pair(bf2f(kn[tid]), bf2f(kn[tid + HALF]), cp[tid], sp[tid], o1, o2);
        const float ka = bf2f(f2bf(o1)), kb = bf2f(f2bf(o2)), va = bf2f(vn[tid]), vb = bf2f(vn[tid + HALF]);
        float ksc, kinv, vsc, vinv;
        fp8_row_scale(wave_max(fmaxf(fabsf(ka), fabsf(kb))), ksc, kinv);
        fp8_row_scale(wave_max(fmaxf(fabsf(va), fabsf(vb))), vsc, vinv);
        const unsigned kq = fp8_quant2(ka, kb, kinv), vq = fp8_quant2(va, vb, vinv);
        Kb[(size_t)pos * HD + tid] = (uint8_t)kq;
        Kb[(size_t)pos * HD + tid + HALF] = (uint8_t)(kq >> 8);
        Vb[(size_t)pos * HD + tid] = (uint8_t)vq;
        Vb[(size_t)pos * HD + tid + HALF] = (uint8_t)(vq >> 8);
        if (tid == 0) { Ks[pos] = ksc; Vs[pos] = vsc; }
    }
    __syncthreads();       // workgroup-scope release/acquire: the appended row is visible to this workgroup's loads

    // everything is requested before anything is converted: the kernel stays ONE memory round trip
    const int kbase = k0 + wave * 16;
    uint32_t vraw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int key = kbase + 2 * j + (lane >> 5);
        key = key < ctx ? key : ctx - 1;
        vraw[j] = *(const uint32_t*)(Vb + (size_t)key * HD + (lane & 31) * 4);
    }
    const int key = kbase + kl;
    const bool valid = key < ctx;
    const int krow = valid ? key : ctx - 1;
    u32x4 kraw[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) kraw[c] = *(const u32x4*)(Kb + (size_t)krow * HD + c * 16);
    const float ksc = Ks[krow], vsc = Vs[krow];            // this lane's key: lanes 0 .. 15 of a wave hold its 16 keys' scales

    uint32_t vv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t w = (uint32_t)__shfl((int)vraw[i >> 1], (i & 1) * 32 + (lane >> 1));
        const float s = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, vsc), i));
        const vl2_f32x2_t f = VL2_CVT_PK_F32_FP8((lane & 1) ? w >> 16 : w, false);
        vv[i] = pack2bf(f[0] * s, f[1] * s);
    }
    u32x4 kreg[16];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const u32x2 a = kv8_dequant4(kraw[c][0], ksc), b = kv8_dequant4(kraw[c][1], ksc);
        const u32x2 d = kv8_dequant4(kraw[c][2], ksc), e = kv8_dequant4(kraw[c][3], ksc);
        kreg[2 * c] = u32x4{a[0], a[1], b[0], b[1]};        // elements 16 c .. 16 c + 7 of the row
        kreg[2 * c + 1] = u32x4{d[0], d[1], e[0], e[1]};
    }
    attn_slice_compute<false>(sm, tid, kreg, vv, valid, ng, scale_log2e, partial + ((size_t)(hk * group + h0) * nsplit + split) * 130,
                              (size_t)nsplit * 130, true);
}
