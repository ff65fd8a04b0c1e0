// Batched decode attention over a shared prompt prefix whose rows live ONCE in the page pool (vl2_attn_decode_shared_paged /
// vl2_kv_page_gather): section 17's cascade through section 19's page lookups.  Only WHOLE pages are shared: P is a
// multiple of 64, prefix_pages[j] (device int32, P / 64 entries) is the page of positions [64 j, 64 j + 64) for every request, and request
// b's own rows from position P on are the pages page_table[b * table_bs + P / 64 + s].  Three launches, no atomics:
//   prefix phase : attn_prefix_paged_kernel = attn_append_kernel<true>'s lines (k_attn_append.h); the only difference is where a 64-key
//                  tile's rows live: the tile's buffer resources are built on its page.
//   own rows     : attn_decode_own_paged_kernel = attn_decode_own_kernel's lines (k_attn_shared.h) with the slice's rows read from (and the
//                  new token's rows appended to) the page the table names, indexed inside the page as attn_decode_paged_kernel does.
//   combine      : attn_shared_combine_kernel, launched unchanged.
// The same arithmetic on the same values in the same lanes: bit for bit vl2_attn_decode_shared on contiguous copies of the same rows.
//   kv_page_gather_kernel : the inverse of kv_page_scatter_kernel (k_attn_paged.h).
#pragma once
#include "k_attn_paged.h"
#include "k_attn_shared.h"

// SharedPrefixArgs with the prefix in pages: k / v = the pools, smax unused; P % 64 == 0.
struct SharedPrefixPagedArgs : SharedPrefixArgs {
    const int* prefix_pages;          // [P / 64]
    int n_pages;
};

// grid = (prefix splits, nkv, ceil(B * group / 128)), block 256 -- attn_append_kernel<true>'s launch.
__global__ __launch_bounds__(256, 2) void attn_prefix_paged_kernel(SharedPrefixPagedArgs p) {
    constexpr int D = 128, KCH = D / 8, KPT = 64 * KCH / 256, VPT = 32 * KCH / 256, NKS = D / 16, NDB = D / 32;
    constexpr int KS_BYTES = 64 * D * 2, VT_BYTES = D * 128;
    constexpr int PAGE_BYTES = KV_PAGE_ROWS * D * 2;                 // one kv head's rows of a page
    __shared__ __attribute__((aligned(16))) unsigned char lds[KS_BYTES + VT_BYTES];
    unsigned char* const Ks = lds;
    unsigned char* const Vt = lds + KS_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int split = blockIdx.x, hk = blockIdx.y, r0 = blockIdx.z * 128;
    const int R = p.n * p.group, nk = p.P;
    // keys of this split: [ks0, kmax)
    const int ks0 = split * p.chunk;
    int kmax = ks0 + p.chunk < nk ? ks0 + p.chunk : nk;
    if (ks0 >= kmax) return;
    const int ntiles = (kmax - ks0 + 63) >> 6;
    // page ids of the split's tiles: wave-uniform scalar loads, each requested a whole tile before the software prefetch that needs it
    const int* const pg = p.prefix_pages + (ks0 >> 6);
    int page_cur = pg[0];
    int page_next = ntiles > 1 ? pg[1] : -1;

    // this lane's row: Q^T fragments (lane (q, hi) holds Q[q][16 ks + 8 hi .. +7]), clamped to the last row
    const int wr0 = r0 + wave * 32;
    const bool wave_live = wr0 < R;
    const int row = wr0 + l31, row_c = row < R ? row : R - 1;
    const int qi = row_c / p.group, hq = hk * p.group + row_c % p.group;
    const int lim_row = p.P - 1;                                    // last visible key of the row
    const int lim_wave0 = p.P - 1;
    const bf16_t* Q = p.q + (size_t)qi * p.q_rs + (size_t)hq * D;
    bf16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *(const bf16x8*)(Q + ks * 16 + hi * 8);
    bool row_live = true;
    {
        // the lane holds both halves of its rotate-half pairs: d = 16 ks + 8 hi + j (ks < 4) and d + 64 (ks + 4)
        const int pos = p.pos_dev[qi];
        row_live = pos >= p.P && pos - p.P < p.own_cap;
        const float* cp = p.cos_t + (size_t)(row_live ? pos : p.P) * 64;
        const float* sp = p.sin_t + (size_t)(row_live ? pos : p.P) * 64;
#pragma unroll
        for (int ks = 0; ks < NKS / 2; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int d = ks * 16 + hi * 8 + j;
                float o1, o2;
                rope_pair(bf2f_s(qf[ks][j]), bf2f_s(qf[ks + NKS / 2][j]), cp[d], sp[d], o1, o2);
                qf[ks][j] = (short)f2bf(o1);
                qf[ks + NKS / 2][j] = (short)f2bf(o2);
            }
    }

    // raw buffer loads (k_attn.h) on the tile's PAGE: 64 rows of this kv head.  A page id outside [0, n_pages) gives zero-length
    // resources on the pools' base: nothing is read, every element is 0 and the outputs are unspecified.
    u32x4 kreg[KPT], vreg[VPT][2];
    auto load_tile = [&](int page) {
        const bool ok = page >= 0 && page < p.n_pages;
        const size_t skip = ok ? ((size_t)page * p.nkv + hk) * PAGE_BYTES : 0;
        const int left = ok ? PAGE_BYTES : 0, left1 = ok ? PAGE_BYTES - D * 2 : 0;
        const auto rsK = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.k + skip), 0, left, 0x00020000);
        const auto rsV = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.v + skip), 0, left, 0x00020000);
        const auto rsV1 = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.v + skip + (ok ? D * 2 : 0)), 0, left1, 0x00020000);
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int c = tid + 256 * i;
            kreg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsK, ((c / KCH) * D + (c % KCH) * 8) * 2, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int c = tid + 256 * i, off = (2 * (c / KCH) * D + (c % KCH) * 8) * 2;
            vreg[i][0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsV, off, 0, 0));
            vreg[i][1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsV1, off, 0, 0));
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const int c = tid + 256 * i;
            *(u32x4*)(Ks + attn_k_off<D>(c / KCH, c % KCH)) = kreg[i];
        }
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int c = tid + 256 * i, kp = c / KCH, ch = c % KCH;
            const int k16 = (2 * kp) & 15;
            const int c16 = ((2 * kp) >> 4) * 2 + ((k16 >> 2) & 1);
            const int eoff = ((k16 >> 3) * 4 + (k16 & 3)) * 2;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned a = (vreg[i][0][j >> 1] >> ((j & 1) * 16)) & 0xffffu;
                const unsigned bb = (vreg[i][1][j >> 1] >> ((j & 1) * 16)) & 0xffffu;
                *(unsigned*)(Vt + attn_vt_off<D>(ch * 8 + j, c16) + eoff) = a | (bb << 16);
            }
        }
    };

    f32x16 oT[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oT[i][r] = 0.f;
    float m = -1e30f, l = 0.f;
    const float c = p.scale_log2e;

    load_tile(page_cur);
    for (int t = 0; t < ntiles; ++t) {
        const int kv0 = ks0 + t * 64;
        __syncthreads();
        store_tile();
        __syncthreads();
        if (t + 1 < ntiles) {
            load_tile(page_next);
            page_next = t + 2 < ntiles ? pg[t + 2] : -1;
        }
        if (!wave_live) continue;                 // rows past R: the wave only helps stage the tiles

        f32x16 sT[2];
        const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const bf16x8 kf = *(const bf16x8*)(Ks + attn_k_off<D>(kh * 32 + l31, ks * 2 + hi));
                sT[kh] = VL2_MFMA32(kf, qf[ks], ks == 0 ? zero16 : sT[kh]);
            }
        // lane owns keys kv0 + 32kh + (r&3) + 8(r>>2) + 4hi of its row; P is a multiple of 64, so every tile is full and this never fires
        if (kv0 + 63 > lim_wave0) {
#pragma unroll
            for (int kh = 0; kh < 2; ++kh)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kv0 + kh * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    sT[kh][r] = key <= lim_row ? sT[kh][r] : -1e30f;
                }
        }
        float mt = -3.0e38f;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int r = 0; r < 16; ++r) mt = fmaxf(mt, sT[kh][r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32)) * c;
        constexpr float THR = 6.0f;              // deferred rescale, decided per row (attn_append_kernel<true>)
        if (mt - m > THR) {
            const float m_new = fmaxf(fmaxf(m, mt), -1e28f);
            const float alpha = __builtin_amdgcn_exp2f(m - m_new);
            m = m_new;
            l *= alpha;
#pragma unroll
            for (int i = 0; i < NDB; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oT[i][r] *= alpha;
        }
        float rsum = 0.f;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(fmaf(sT[kh][r], c, -m));
                sT[kh][r] = pv;
                rsum += pv;
            }
        l += rsum + __shfl_xor(rsum, 32);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int ks2 = 0; ks2 < 2; ++ks2) {
                u32x4 pw;
#pragma unroll
                for (int j = 0; j < 4; ++j) pw[j] = pack2bf(sT[kh][ks2 * 8 + 2 * j], sT[kh][ks2 * 8 + 2 * j + 1]);
                const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
                const int c16 = (kh * 2 + ks2) * 2 + hi;
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    const bf16x8 vf = *(const bf16x8*)(Vt + attn_vt_off<D>(db * 32 + l31, c16));
                    oT[db] = VL2_MFMA32(vf, pf, oT[db]);
                }
            }
    }
    // partial of (row, split): lane (q, hi) holds o[d] for d = 32 db + 8 g + 4 hi + j
    if (!wave_live || row >= R || ks0 > lim_row || !row_live) return;
    float* dst = p.ws + (size_t)qi * p.partial_bs + ((size_t)hq * p.nsplit_cap + split) * 130;
    if (hi == 0) *(f32x2*)dst = f32x2{m, l};
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            // 130-float slices are only 8-byte aligned: two f32x2 stores
            float* o = dst + 2 + db * 32 + 8 * g + 4 * hi;
            *(f32x2*)o = f32x2{oT[db][4 * g], oT[db][4 * g + 1]};
            *(f32x2*)(o + 2) = f32x2{oT[db][4 * g + 2], oT[db][4 * g + 3]};
        }
}

// grid = (own_cap / 64, nkv * requests, ceil(group / 4)), block 256: attn_decode_own_kernel's launch and lines.  P / 64 + own_cap / 64 <=
// table_bs (checked by the host), so the table read below is inside row bseq for every workgroup.
__global__ __launch_bounds__(256) void attn_decode_own_paged_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kpool,
                                                                    bf16_t* __restrict__ vpool, const int* __restrict__ page_table,
                                                                    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                                    float* __restrict__ partial, int nh, int group, int nkv, int own_cap, int P,
                                                                    int nps, int nsplit_cap, int n_pages, int table_bs,
                                                                    const int* __restrict__ pos_dev, float scale_log2e, long qkv_bs,
                                                                    long partial_bs) {
    constexpr int HD = 128, HALF = 64;
    __shared__ AttnSliceSmem sm;
    auto& qs = sm.qs;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kl = lane & 15;
    const int split = blockIdx.x, hk = (int)blockIdx.y % nkv, bseq = (int)blockIdx.y / nkv;
    const int h0 = blockIdx.z * 4;
    const int ng = group - h0 < 4 ? group - h0 : 4;
    const int pos = pos_dev[bseq], own = pos - P;                  // own = the new token's row among the request's own rows
    // wave-uniform (a scalar load), requested beside the position: it is first needed after the q RoPE below
    const int page = page_table[(size_t)bseq * table_bs + (P >> 6) + split];
    if (own < 0 || own >= own_cap) return;
    const int ctx = own + 1;
    const int k0 = split * KV_PAGE_ROWS;
    if (k0 >= ctx) return;
    qkv += (size_t)bseq * qkv_bs;
    partial += (size_t)bseq * partial_bs;
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
    // a slice without a page (not assigned, or an id outside the pool): the whole workgroup leaves before it touches either pool -- the
    // one that owns `pos` and would append included.  The request's output is then unspecified; the host discards it.
    if (page < 0 || page >= n_pages) return;
    bf16_t* Kb = kpool + ((size_t)page * nkv + hk) * (KV_PAGE_ROWS * HD);      // the page's rows of this kv head: row = own row - k0
    bf16_t* Vb = vpool + ((size_t)page * nkv + hk) * (KV_PAGE_ROWS * HD);
    const int last = ctx - 1 - k0;                         // the last visible row of this page (>= 0: k0 < ctx); 63 for a full slice
    if (own >= k0 && own < k0 + KV_PAGE_ROWS && tid < HALF) {
        const bf16_t* kn = qkv + (size_t)(nh + hk) * HD;
        const bf16_t* vn = qkv + (size_t)(nh + nkv + hk) * HD;
        float o1, o2;
        rope_pair(bf2f(kn[tid]), bf2f(kn[tid + HALF]), cp[tid], sp[tid], o1, o2);
        Kb[(size_t)last * HD + tid] = f2bf(o1);            // (own - k0 == last in this slice)
        Kb[(size_t)last * HD + tid + HALF] = f2bf(o2);
        Vb[(size_t)last * HD + tid] = vn[tid];
        Vb[(size_t)last * HD + tid + HALF] = vn[tid + HALF];
    }
    __syncthreads();

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
                              partial + ((size_t)(hk * group + h0) * nsplit_cap + nps + split) * 130, (size_t)nsplit_cap * 130, true);
}

// The inverse of kv_page_scatter_kernel, same grid and row numbering: rows [p0, p1) of the pages a table row names -> one sequence's contiguous
// caches [nkv, smax, 128], byte for byte.  A row whose page id is outside [0, n_pages) is skipped; nothing else in the caches is written.
__global__ __launch_bounds__(256) void kv_page_gather_kernel(const bf16_t* __restrict__ kpool, const bf16_t* __restrict__ vpool,
                                                             bf16_t* __restrict__ k16, bf16_t* __restrict__ v16,
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
    const u32x4 w = *(const u32x4*)((isv ? vpool : kpool) + (((size_t)page * nkv + hk) * KV_PAGE_ROWS + p % KV_PAGE_ROWS) * HD + sub * 8);
    *(u32x4*)((isv ? v16 : k16) + ((size_t)hk * smax + p) * HD + sub * 8) = w;
}
