// Paged KV cache in fp8 for the batched decode step (vl2_attn_decode_kv8_paged / vl2_kv_page_quant): the pages of section
// 19 (k_attn_paged.h) holding the rows of section 16 (k_kv8.h).  Per layer, four pools:
//   k8pool / v8pool : uint8 [n_pages][nkv][64][128] e4m3fn codes -- the bytes the contiguous fp8 cache holds for those positions;
//   kspool / vspool : fp32  [n_pages][nkv][64]      one power-of-two scale per (kv head, row), k_kv8.h's format.
// Page ids, the page table and the parking page are k_attn_paged.h's: one id names the same page in all four pools of every layer.
// A page is exactly the 64-key slice one workgroup of attn_decode_kv8_kernel reads, so paging is ONE table lookup per workgroup and no change
// to any sum:
//   attn_decode_kv8_paged_kernel : attn_decode_kv8_kernel's lines with the page looked up as attn_decode_paged_kernel does it -- the same
//                                  arithmetic on the same values in the same lanes, so the same bits as vl2_attn_decode_kv8_batched on
//                                  contiguous copies of the same codes and scales; same grid and `partial` layout, the combine unchanged.
//   kv_page_quant_kernel         : kv_quant_rows_kernel's arithmetic with kv_page_scatter_kernel's store address: rows [p0, p1) of one
//                                  sequence's 16-bit staging caches -> codes and scales in its pages.
#pragma once
#include "k_kv8.h"
#include "k_attn_paged.h"

// grid = (nsplit_cap, nkv * sequences, ceil(group/4)), block 256 -- attn_decode_kv8_kernel's launch.  nsplit_cap <= seq_cap / 64 <= table_bs
// (checked by the host), so the table read below is inside row bseq for every workgroup.
__global__ __launch_bounds__(256) void attn_decode_kv8_paged_kernel(const bf16_t* __restrict__ qkv, uint8_t* __restrict__ k8pool,
                                                                    uint8_t* __restrict__ v8pool, float* __restrict__ kspool,
                                                                    float* __restrict__ vspool, const int* __restrict__ page_table,
                                                                    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                    float* __restrict__ partial, int nh, int group, int nkv, int seq_cap,
                                                                    int n_pages, int table_bs, const int* __restrict__ pos_dev,
                                                                    float scale_log2e, long qkv_bs, long partial_bs) {
    constexpr int HD = 128, HALF = 64;
    __shared__ AttnSliceSmem sm;
    auto& qs = sm.qs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kl = lane & 15;
    const int split = blockIdx.x, hk = (int)blockIdx.y % nkv, bseq = (int)blockIdx.y / nkv, nsplit = gridDim.x;
    const int h0 = blockIdx.z * 4;
    const int ng = group - h0 < 4 ? group - h0 : 4;
    const int pos = pos_dev[bseq];
    // wave-uniform (a scalar load), requested beside the position: it is first needed after the q RoPE below
    const int page = page_table[(size_t)bseq * table_bs + split];
    qkv += (size_t)bseq * qkv_bs;
    partial += (size_t)bseq * partial_bs;
    if (pos >= seq_cap) return;                            // a device-side position past the table: touch nothing (see attn_decode_kernel)
    const int ctx = pos + 1;
    const int k0 = split * KV_PAGE_ROWS;
    if (k0 >= ctx) return;
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
    // a slice without a page (not assigned, or an id outside the pool): the whole workgroup leaves before it touches any of the four pools --
    // the one that owns `pos` and would append included -- and before the cross-lane V exchange below, so no wave shuffles with missing lanes
    // (blockIdx and the table entry are workgroup-uniform).  The request's output is then unspecified; the host discards it.
    if (page < 0 || page >= n_pages) return;
    uint8_t* Kb = k8pool + ((size_t)page * nkv + hk) * (KV_PAGE_ROWS * HD);    // the page's rows of this kv head: row = key - k0
    uint8_t* Vb = v8pool + ((size_t)page * nkv + hk) * (KV_PAGE_ROWS * HD);
    float* Ks = kspool + ((size_t)page * nkv + hk) * KV_PAGE_ROWS;
    float* Vs = vspool + ((size_t)page * nkv + hk) * KV_PAGE_ROWS;
    const int last = ctx - 1 - k0;                         // the last visible row of this page (>= 0: k0 < ctx); 63 for a full slice
    // the slice that owns the new position: attn_decode_kv8_kernel's quantise-and-append, into row pos - k0 == last of its page, before anyone
    // reads that row.  One wave: lane d holds (d, d + 64).
    if (pos >= k0 && pos < k0 + KV_PAGE_ROWS && tid < HALF) {
        const bf16_t* kn = qkv + (size_t)(nh + hk) * HD;
        const bf16_t* vn = qkv + (size_t)(nh + nkv + hk) * HD;
        float o1, o2;
        rope_pair(bf2f(kn[tid]), bf2f(kn[tid + HALF]), cp[tid], sp[tid], o1, o2);
        const float ka = bf2f(f2bf(o1)), kb = bf2f(f2bf(o2)), va = bf2f(vn[tid]), vb = bf2f(vn[tid + HALF]);
        float ksc, kinv, vsc, vinv;
        fp8_row_scale(wave_max(fmaxf(fabsf(ka), fabsf(kb))), ksc, kinv);
        fp8_row_scale(wave_max(fmaxf(fabsf(va), fabsf(vb))), vsc, vinv);
        const unsigned kq = fp8_quant2(ka, kb, kinv), vq = fp8_quant2(va, vb, vinv);
        Kb[(size_t)last * HD + tid] = (uint8_t)kq;
        Kb[(size_t)last * HD + tid + HALF] = (uint8_t)(kq >> 8);
        Vb[(size_t)last * HD + tid] = (uint8_t)vq;
        Vb[(size_t)last * HD + tid + HALF] = (uint8_t)(vq >> 8);
        if (tid == 0) { Ks[last] = ksc; Vs[last] = vsc; }
    }
    __syncthreads();       // workgroup-scope release/acquire: the appended row is visible to this workgroup's loads

    // everything is requested before anything is converted (attn_decode_kv8_kernel's loads with the row index inside the page; ragged keys
    // are clamped to the last visible row, which lies in this page)
    const int rbase = wave * 16;
    uint32_t vraw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int row = rbase + 2 * j + (lane >> 5);
        row = row <= last ? row : last;
        vraw[j] = *(const uint32_t*)(Vb + (size_t)row * HD + (lane & 31) * 4);
    }
    const int row = rbase + kl;
    const bool valid = row <= last;
    const int krow = valid ? row : last;
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

// grid = ceil(2 * nkv * (p1 - p0) / 16), block 256: kv_quant_rows_kernel's launch and row numbering (16 lanes per row: 16 B of the 16-bit row
// in, 8 code bytes out per lane; K rows first, kv head major, then V rows).  table_row: the sequence's row of the page table, ceil(smax / 64)
// entries.  A dead row (past the last one) and a row whose page id is outside [0, n_pages) keep their lanes for the shuffles of the max
// reduction and leave after it; nothing else in the four pools is written.
__global__ __launch_bounds__(256) void kv_page_quant_kernel(const bf16_t* __restrict__ k16, const bf16_t* __restrict__ v16,
                                                            uint8_t* __restrict__ k8pool, uint8_t* __restrict__ v8pool,
                                                            float* __restrict__ kspool, float* __restrict__ vspool,
                                                            const int* __restrict__ table_row, int nkv, int smax, int n_pages, int p0, int p1) {
    constexpr int HD = 128;
    const int n = p1 - p0;
    const long nrows = 2L * nkv * n;
    const long r = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    const bool live = r < nrows;                           // (a dead row keeps its lanes for the shuffles below)
    const long rr = live ? r : nrows - 1;
    const bool isv = rr >= (long)nkv * n;
    const long rk = isv ? rr - (long)nkv * n : rr;
    const int hk = (int)(rk / n), p = p0 + (int)(rk % n);                       // (kv head, position)
    const int page = table_row[p / KV_PAGE_ROWS];
    float v[8];
    unpack8(*(const u32x4*)((isv ? v16 : k16) + ((size_t)hk * smax + p) * HD + sub * 8), v);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
#pragma unroll
    for (int msk = 8; msk >= 1; msk >>= 1) amax = fmaxf(amax, __shfl_xor(amax, msk));        // over the row's 16 lanes
    float sc, inv;
    fp8_row_scale(amax, sc, inv);
    if (!live || page < 0 || page >= n_pages) return;
    const size_t row = ((size_t)page * nkv + hk) * KV_PAGE_ROWS + p % KV_PAGE_ROWS;
    *(u32x2*)((isv ? v8pool : k8pool) + row * HD + sub * 8) = fp8_quant8(v, inv);
    if (sub == 0) (isv ? vspool : kspool)[row] = sc;
}
