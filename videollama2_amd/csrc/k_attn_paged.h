// Paged KV cache for the batched decode step (vl2_attn_decode_paged / vl2_kv_page_scatter).  The requests of a step keep
// their 16-bit K/V rows in PAGES of 64 consecutive positions drawn from one pool per layer instead of a private cache of max_seq_len rows:
//   page       : [nkv][64][128] elements, the bytes the contiguous cache holds for those positions (K roped and rounded, V as projected);
//   pools      : kpool / vpool = [n_pages] pages per layer; one page id names the same page in every layer's K and V pool;
//   page table : int32 [B][table_bs]; entry j of row b = the page of positions [64 j, 64 j + 64) of request b, -1 = not assigned.
// attn_decode_kernel<false> (k_decode.h) gives one workgroup to one 64-key slice of one kv head: a page is exactly one workgroup's rows, so
// paging is ONE table lookup per workgroup and no change to any sum.
//   attn_decode_paged_kernel : attn_decode_kernel<false>'s lines on attn_slice_compute<false> (the same arithmetic on the same values in the
//                              same lanes, so the same bits), same grid and `partial` layout; attn_decode_combine_kernel consumes the
//                              partials unchanged.
//   kv_page_scatter_kernel   : rows [p0, p1) of one sequence's contiguous caches (a prefill's staging cache) -> its pages, byte for byte.
#pragma once
#include "k_decode.h"

constexpr int KV_PAGE_ROWS = 64;                           // positions per page = keys per slice of the decode attention

// grid = (nsplit_cap, nkv * sequences, ceil(group/4)), block 256 -- attn_decode_kernel<false>'s launch.  nsplit_cap <= seq_cap / 64 <=
// table_bs (checked by the host), so the table read below is inside row bseq for every workgroup.
__global__ __launch_bounds__(256) void attn_decode_paged_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kpool,
                                                                bf16_t* __restrict__ vpool, const int* __restrict__ page_table,
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
    // a slice without a page (not assigned, or an id outside the pool): the whole workgroup leaves before it touches either pool -- the
    // one that owns `pos` and would append included.  The request's output is then unspecified; the host discards it.
    if (page < 0 || page >= n_pages) return;
    bf16_t* Kb = kpool + ((size_t)page * nkv + hk) * (KV_PAGE_ROWS * HD);      // the page's rows of this kv head: row = key - k0
    bf16_t* Vb = vpool + ((size_t)page * nkv + hk) * (KV_PAGE_ROWS * HD);
    const int last = ctx - 1 - k0;                         // the last visible row of this page (>= 0: k0 < ctx); 63 for a full slice
    // the slice that owns the new position appends roped k_new and v_new to its page before anyone reads that row
    if (pos >= k0 && pos < k0 + KV_PAGE_ROWS && tid < HALF) {
        const bf16_t* kn = qkv + (size_t)(nh + hk) * HD;
        const bf16_t* vn = qkv + (size_t)(nh + nkv + hk) * HD;
        float o1, o2;
        rope_pair(bf2f(kn[tid]), bf2f(kn[tid + HALF]), cp[tid], sp[tid], o1, o2);
        Kb[(size_t)last * HD + tid] = f2bf(o1);            // (pos - k0 == last in this slice)
        Kb[(size_t)last * HD + tid + HALF] = f2bf(o2);
        Vb[(size_t)last * HD + tid] = vn[tid];
        Vb[(size_t)last * HD + tid + HALF] = vn[tid + HALF];
    }
    __syncthreads();       // workgroup-scope release/acquire: the appended rows are visible to this workgroup's loads

    // V rows of this wave's 16 keys, then the lane's K row: attn_decode_kernel's loads with the row index inside the page; ragged keys are
    // clamped to the last visible row, which lies in this page
    uint32_t vv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        int row = wave * 16 + i;
        row = row <= last ? row : last;
        vv[i] = *(const uint32_t*)(Vb + (size_t)row * HD + lane * 2);
    }
    const int row = wave * 16 + kl;
    const bool valid = row <= last;
    const bf16_t* kr = Kb + (size_t)(valid ? row : last) * HD;
    u32x4 kreg[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) kreg[c] = *(const u32x4*)(kr + c * 8);

    attn_slice_compute<false>(sm, tid, kreg, vv, valid, ng, scale_log2e,
                              partial + ((size_t)(hk * group + h0) * nsplit + split) * 130, (size_t)nsplit * 130, true);
}

// grid = ceil(2 * nkv * (p1 - p0) / 16), block 256: 16 lanes per row of 256 B (one 16-byte load and store per lane), 16 rows per workgroup;
// rows are numbered K rows first (kv head major), then V rows (kv_quant_rows_kernel's numbering).  table_row: the sequence's row of the page
// table, ceil(smax / 64) entries.  A row whose page id is outside [0, n_pages) is skipped; nothing else in the pools is written.
__global__ __launch_bounds__(256) void kv_page_scatter_kernel(const bf16_t* __restrict__ k16, const bf16_t* __restrict__ v16,
                                                              bf16_t* __restrict__ kpool, bf16_t* __restrict__ vpool,
                                                              const int* __restrict__ table_row, int nkv, int smax, int n_pages, int p0, int p1) {
    constexpr int HD = 128;
    const int n = p1 - p0;
    const long nrows = 2L * nkv * n;
    const long r = (long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    if (r >= nrows) return;
    const bool isv = r >= (long)nkv * n;
    const long rk = isv ? r - (long)nkv * n : r;
    const int hk = (int)(rk / n), p = p0 + (int)(rk % n);                       // (kv head, position)
    const int page = table_row[p / KV_PAGE_ROWS];
    if (page < 0 || page >= n_pages) return;
    const u32x4 w = *(const u32x4*)((isv ? v16 : k16) + ((size_t)hk * smax + p) * HD + sub * 8);
    *(u32x4*)((isv ? vpool : kpool) + (((size_t)page * nkv + hk) * KV_PAGE_ROWS + p % KV_PAGE_ROWS) * HD + sub * 8) = w;
}
