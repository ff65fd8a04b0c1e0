// Append attention (split-KV, "flash-decoding" generalised to many query rows): n new query rows at positions P .. P+n-1 of ONE
// sequence attend causally to the P + n keys of its cache [nkv, smax, 128] (key j is visible to row i iff j <= P + i).  The prefill
// of a chat turn on top of a resident KV cache (decoder.extend).
//
// Rows of a kv head: r = i * group + h (query i, q head h of the group) -> R = n * group rows; a workgroup takes 128 of them
// (4 waves x 32 rows, blockIdx.z) and ONE split of the keys (blockIdx.x, `chunk` keys = a multiple of 64): its K/V tiles are staged
// through LDS once for all of its rows.  The tile math is attn_fwd_kernel's (k_attn.h): the transposed formulation on
// v_mfma_f32_32x32x16 (S^T = K . Q^T, O^T += V^T . P^T with the V^T image of attn_vt_off), online softmax in the exp2 domain.
// Each (row, split) leaves an fp32 partial {m, l, o[128]} in `ws` ([nh][n][nsplit][130], the layout attn_combine_head reads);
// attn_append_combine_kernel merges the live splits of a row in split order (k_decode.h attn_combine_head: fixed-order FMAs).
// No atomics: the bits do not depend on scheduling.
#pragma once
#include "dev_common.h"
#include "k_attn.h"
#include "k_decode.h"
#include <type_traits>

#define APPEND_MAX_SPLITS 32          // = COMBINE_EARLY: the combine is one memory round trip

struct AppendArgs {
    const bf16_t* q; long q_rs;       // roped q rows [n][nh*128] (row stride q_rs elements)
    const bf16_t* k; const bf16_t* v; // caches [nkv][smax][128]
    int smax, P, n, nh, nkv, group;
    int chunk, nsplit;                // keys per split (multiple of 64), splits
    float scale_log2e;
    float* ws;                        // [nh][n][nsplit][130]
};
// SHARED form (the prefix phase of vl2_attn_decode_shared, k_attn_shared.h): the n rows are n REQUESTS of a batched decode step that share
// the keys [0, P) of one cache.  q / q_rs = the step's un-roped fused qkv rows and their stride: row b is roped here, at pos_dev[b], and
// rounded through the element type as attn_decode_kernel rounds its qs.  Every prefix key is visible to every row (only the ragged last
// tile at P is masked); nsplit = the prefix splits.  The partial of (request b, q head, split) goes to ws + b*partial_bs +
// (head * nsplit_cap + split) * 130: the leading slices of the request's region of the decode `partial` buffer.  A request whose position
// is outside [P, P + own_cap) writes nothing.
struct SharedPrefixArgs : AppendArgs {
    const int* pos_dev; const float* cos_t; const float* sin_t;      // cos / sin: fp32 [positions][64]
    int own_cap, nsplit_cap;
    long partial_bs;
};

template <bool SHARED>
__global__ __launch_bounds__(256, 2) void attn_append_kernel(std::conditional_t<SHARED, SharedPrefixArgs, AppendArgs> p) {
    constexpr int D = 128, KCH = D / 8, KPT = 64 * KCH / 256, VPT = 32 * KCH / 256, NKS = D / 16, NDB = D / 32;
    constexpr int KS_BYTES = 64 * D * 2, VT_BYTES = D * 128;
    __shared__ __attribute__((aligned(16))) unsigned char lds[KS_BYTES + VT_BYTES];
    unsigned char* const Ks = lds;
    unsigned char* const Vt = lds + KS_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int split = blockIdx.x, hk = blockIdx.y, r0 = blockIdx.z * 128;
    const int R = p.n * p.group, nk = SHARED ? p.P : p.P + p.n;
    // keys of this split that any row of the block can see: [ks0, kmax)
    const int ks0 = split * p.chunk;
    const int rlast = (r0 + 127 < R ? r0 + 127 : R - 1);
    int kmax = ks0 + p.chunk < nk ? ks0 + p.chunk : nk;
    const int lim = SHARED ? nk : p.P + rlast / p.group + 1;
    kmax = lim < kmax ? lim : kmax;
    if (ks0 >= kmax) return;                     // no row of the block reaches this split (the combine does not read it)
    const int ntiles = (kmax - ks0 + 63) >> 6;

    // this lane's row: Q^T fragments (lane (q, hi) holds Q[q][16 ks + 8 hi .. +7]), clamped to the last row
    const int wr0 = r0 + wave * 32;
    const bool wave_live = wr0 < R;
    const int row = wr0 + l31, row_c = row < R ? row : R - 1;
    const int qi = row_c / p.group, hq = hk * p.group + row_c % p.group;
    const int lim_row = SHARED ? p.P - 1 : p.P + qi;                // last visible key of the row
    const int lim_wave0 = SHARED ? p.P - 1 : p.P + (wr0 < R ? wr0 : R - 1) / p.group;  // ... of the wave's first row (the smallest)
    const bf16_t* Q = p.q + (size_t)qi * p.q_rs + (size_t)hq * D;
    bf16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *(const bf16x8*)(Q + ks * 16 + hi * 8);
    bool row_live = true;
    if constexpr (SHARED) {
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

    const bf16_t* K = p.k + (size_t)hk * p.smax * D;
    const bf16_t* V = p.v + (size_t)hk * p.smax * D;
    // raw buffer loads (k_attn.h): rows at or past nk fall outside NUM_RECORDS and read as 0 (masked scores, p = 0)
    u32x4 kreg[KPT], vreg[VPT][2];
    const int kv_bytes = nk * D * 2;
    auto load_tile = [&](int kv0) {
        const int skip = kv0 * D * 2;
        const int left = kv_bytes > skip ? kv_bytes - skip : 0, left1 = kv_bytes > skip + D * 2 ? kv_bytes - skip - D * 2 : 0;
        const auto rsK = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)K + skip), 0, left, 0x00020000);
        const auto rsV = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)V + skip), 0, left, 0x00020000);
        const auto rsV1 = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)V + skip + D * 2), 0, left1, 0x00020000);
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

    load_tile(ks0);
    for (int t = 0; t < ntiles; ++t) {
        const int kv0 = ks0 + t * 64;
        __syncthreads();
        store_tile();
        __syncthreads();
        if (t + 1 < ntiles) load_tile(kv0 + 64);
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
        // lane owns keys kv0 + 32kh + (r&3) + 8(r>>2) + 4hi of its row; visible iff key <= P + i (which also keeps key < nk)
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
        constexpr float THR = 6.0f;              // deferred rescale, as attn_fwd_kernel
        // SHARED: the rows of a wave belong to several requests, so the decision is each row's own (both halves of a row hold the same mt
        // and m; the branch holds no cross-lane operation) -- a wave vote would let a neighbour's jump move this row's m, and with it
        // the rounding of its P and its partial
        if (SHARED ? mt - m > THR : !__all(mt - m <= THR)) {
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
    float* dst;
    if constexpr (SHARED) dst = p.ws + (size_t)qi * p.partial_bs + ((size_t)hq * p.nsplit_cap + split) * 130;
    else dst = p.ws + (((size_t)hq * p.n + qi) * p.nsplit + split) * 130;
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

// grid = (nh, n), block 128: row i of q head h = the splits 0 .. nlive-1 that reach key P + i, merged in split order.
__global__ __launch_bounds__(128) void attn_append_combine_kernel(const float* __restrict__ ws, bf16_t* __restrict__ out, long o_rs, int n,
                                                                  int P, int chunk, int nsplit) {
    __shared__ float wgt[COMBINE_CHUNK];
    __shared__ float red[2];
    const int h = blockIdx.x, i = blockIdx.y, d = threadIdx.x;
    int nlive = (P + i) / chunk + 1;
    nlive = nlive < nsplit ? nlive : nsplit;
    attn_combine_head<false>(ws + ((size_t)h * n + i) * nsplit * 130, nlive, d, wgt, red, out + (size_t)i * o_rs + (size_t)h * 128, true);
}
