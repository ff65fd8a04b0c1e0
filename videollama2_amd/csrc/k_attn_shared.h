// Batched decode attention over a SHARED prompt prefix ("cascade" decode attention; vl2_attn_decode_shared): the nb
// requests of a step share the keys [0, P) of ONE cache [nkv][prefix_smax][128]; request b keeps only its own rows, from position P on, in a
// private cache [nkv][own_cap][128] (cache row = position - P).  Three launches, no atomics:
//   prefix phase : attn_append_kernel<true> (k_attn_append.h): the nb * group query rows of a kv head against one copy of the prefix, on
//                  the matrix pipe, split over the prefix keys -> the LEADING `nps` slices of each request's region of `partial`.
//   own rows     : attn_decode_own_kernel below = attn_decode_kernel<false> (k_decode.h) with a position base: the same 64-key slices
//                  (attn_slice_compute: the same arithmetic, so the same bits for the same rows), RoPE and cos/sin at the absolute position,
//                  k_new / v_new appended at private row pos - P -> slices nps + s of the request's region.
//   combine      : attn_combine_head over the nps + ceil((pos - P + 1) / 64) live slices, in slice order.
// partial: fp32 [nb][nh][nsplit_cap][130], nsplit_cap = nps + own_cap / 64.  A request whose position is outside [P, P + own_cap) touches
// nothing in any of the three (a device-side position that ran past its private cache under hipGraph replay: the host discards the step).
#pragma once
#include "k_attn_append.h"

// grid = (own_cap / 64, nkv * requests, ceil(group / 4)), block 256: attn_decode_kernel<false>'s launch and lines.
__global__ __launch_bounds__(256) void attn_decode_own_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kcache,
                                                              bf16_t* __restrict__ vcache, const float* __restrict__ cos_t,
                                                              const float* __restrict__ sin_t, float* __restrict__ partial,
                                                              int nh, int group, int nkv, int own_cap, int P, int nps, int nsplit_cap,
                                                              const int* __restrict__ pos_dev, float scale_log2e,
                                                              long qkv_bs, long cache_bs, long partial_bs) {
    constexpr int HD = 128, HALF = 64;
    __shared__ AttnSliceSmem sm;
    auto& qs = sm.qs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kl = lane & 15;
    const int split = blockIdx.x, hk = (int)blockIdx.y % nkv, bseq = (int)blockIdx.y / nkv;
    const int h0 = blockIdx.z * 4;
    const int ng = group - h0 < 4 ? group - h0 : 4;
    const int pos = pos_dev[bseq], own = pos - P;                  // own = the new token's row of the private cache
    if (own < 0 || own >= own_cap) return;
    const int ctx = own + 1;
    const int k0 = split * 64;
    if (k0 >= ctx) return;
    qkv += (size_t)bseq * qkv_bs;
    partial += (size_t)bseq * partial_bs;
    bf16_t* Kb = kcache + (size_t)bseq * cache_bs + (size_t)hk * own_cap * HD;
    bf16_t* Vb = vcache + (size_t)bseq * cache_bs + (size_t)hk * own_cap * HD;
    const float* cp = cos_t + (size_t)pos * HALF;
    const float* sp = sin_t + (size_t)pos * HALF;

    for (int t = tid; t < ng * HALF; t += 256) {
        const int h = t / HALF, d = t % HALF;
        const bf16_t* qh = qkv + (size_t)(hk * group + h0 + h) * HD;
        float o1, o2;
        rope_pair(bf2f(qh[d]), bf2f(qh[d + HALF]), cp[d], sp[d], o1, o2);
        qs[h][d] = bf2f(f2bf(o1));
        qs[h][d + HALF] = bf2f(f2bf(o2));
    }
    if (own >= k0 && own < k0 + 64 && tid < HALF) {
        const bf16_t* kn = qkv + (size_t)(nh + hk) * HD;
        const bf16_t* vn = qkv + (size_t)(nh + nkv + hk) * HD;
        float o1, o2;
        rope_pair(bf2f(kn[tid]), bf2f(kn[tid + HALF]), cp[tid], sp[tid], o1, o2);
        Kb[(size_t)own * HD + tid] = f2bf(o1);
        Kb[(size_t)own * HD + tid + HALF] = f2bf(o2);
        Vb[(size_t)own * HD + tid] = vn[tid];
        Vb[(size_t)own * HD + tid + HALF] = vn[tid + HALF];
    }
    __syncthreads();

    uint32_t vv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        int key = k0 + wave * 16 + i;
        key = key < ctx ? key : ctx - 1;
        vv[i] = *(const uint32_t*)(Vb + (size_t)key * HD + lane * 2);
    }
    const int key = k0 + wave * 16 + kl;
    const bool valid = key < ctx;
    const bf16_t* kr = Kb + (size_t)(valid ? key : ctx - 1) * HD;
    u32x4 kreg[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) kreg[c] = *(const u32x4*)(kr + c * 8);

    attn_slice_compute<false>(sm, tid, kreg, vv, valid, ng, scale_log2e,
                              partial + ((size_t)(hk * group + h0) * nsplit_cap + nps + split) * 130, (size_t)nsplit_cap * 130, true);
}

// grid = (nh, requests), block 128: the nps prefix splits, then the request's own slices, merged in slice order.
__global__ __launch_bounds__(128) void attn_shared_combine_kernel(const float* __restrict__ partial, bf16_t* __restrict__ out, int P, int nps,
                                                                  int own_cap, int nsplit_cap, const int* __restrict__ pos_dev,
                                                                  long partial_bs, long out_bs) {
    __shared__ float wgt[COMBINE_CHUNK];
    __shared__ float red[2];
    const int h = blockIdx.x, d = threadIdx.x, bseq = blockIdx.y;
    const int own = pos_dev[bseq] - P;
    if (own < 0 || own >= own_cap) return;
    const int nlive = nps + ((own + 64) >> 6);                 // <= nsplit_cap: own_cap is a multiple of 64
    const float* src = partial + (size_t)bseq * partial_bs + (size_t)h * nsplit_cap * 130;
    attn_combine_head<false>(src, nlive, d, wgt, red, out + (size_t)bseq * out_bs + h * 128, true);
}
