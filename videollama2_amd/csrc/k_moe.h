// Sparse mixture-of-experts block of the Mixtral decoder (HF:models/mixtral/modeling_mixtral.py MixtralSparseMoeBlock =
// MixtralTopKRouter + MixtralExperts):
//   logits = RMSNorm(x1) Wr^T (fp32), p = softmax(logits), (w, e) = topk(p, k), w /= sum(w),
//   x = x1 + sum_j w_j * down_e(silu(gate_e(h)) * up_e(h)),  e = e_j,  h = RMSNorm(x1)
// The RMSNorm weight is folded into Wr (fp32, exact) and into every expert's gate/up rows (weights.fold_norm) at pack time, so the
// kernels normalise with a unit weight.
//
// Prefill (S tokens), every table on the device -- no count ever goes to the host, so the block captures into a graph:
//   moe_router_kernel   one wave per token: rstd, E fp32 dot products, softmax, top-k (ties -> the lower expert index),
//                       renormalised weights.  The same kernel with S = 1 is the decode step's router GEMV.
//   moe_scan_kernel     ONE workgroup: per-expert counts, row offsets padded to the grouped GEMM's row tile, the gather
//                       table (permuted row -> token, -1 = padding) and the inverse map ((token, slot) -> permuted row).
//                       Inside an expert the rows are in ascending token order (ballot + popcount over token chunks), so
//                       every table is a pure function of the expert ids: nothing depends on the order of atomics.
//   moe_gather_kernel   the permuted activation rows and their (0, rstd) row-norm entries (one workgroup per row).
//   moe_gemm_kernel     ONE launch for all experts: workgroup -> (row tile, column tile) of the permuted rows; the expert
//                       of a row tile comes from the offsets on the device; tiles past offs[E] return at once.  Each tile
//                       runs k_gemm9.h gemm_l8_16_body (128 x 128, v_mfma_f32_16x16x32_bf16) on a GemmArgs of its own
//                       (A / C / row-norm rows of the tile, the expert's W panel), so a row has the bits of the library's
//                       dense 16 x 16 x 32 GEMMs on the same rows.  The body's empty-wave skip covers the ragged last
//                       tile of an expert (waves whose 32 rows are all past the expert's count issue no MFMA).
//   moe_combine_kernel  x[t] = x1[t] + sum_j w_tj y[inv(t, j)] in fp32, slot order, rounded once; also (0, rstd) of the
//                       new row for the next layer's norm-carrying q/k/v GEMM.  No float atomics.
// Decode (one token, graph-replayable: expert ids and weights are read from device memory):
//   moe_router_kernel (S = 1), moe_gemv_gu_kernel (gate/up + SwiGLU of the k chosen experts, k_decode.h gemv_bf16_body),
//   moe_gemv_down_kernel (both experts' dot products of the same output rows, weighted, + residual).
#pragma once
#include "k_decode.h"
#include "k_gemm9.h"

#define MOE_MAX_E 64
#define MOE_MAX_K 4
#define MOE_BM GEMM_BM                 // row tile of the grouped GEMM (gemm_l8_16_body)
#define MOE_SCAN_MAX 16384             // S * k ids staged in the scan kernel's LDS

// (value, index) of the larger probability, ties to the lower index
__device__ __forceinline__ void moe_argmax_pair(float& v, int& i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float v2 = __shfl_xor(v, m);
        const int i2 = __shfl_xor(i, m);
        if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
    }
}

// a / b for the renormalised routing weights.  The library is built with -ffast-math, which turns `a / b` into a * rcp(b): p / p could then be
// 1 - 2^-24 and p / (2 p) one step off 0.5, where MixtralTopKRouter's top_k_weights / sum gives exactly 1 for k = 1 and exactly 1 / k for k tied
// experts.  One residual step on the hardware reciprocal is independent of the build's flags: q = a rcp(b), r = a - b q (exact in the fma),
// q + r rcp(b).  For a = b and for b = k a with k a power of two the correction lands on 1 resp. 1 / k exactly (the error left is ~2^-47).
__device__ __forceinline__ float moe_div(float a, float b) {
#pragma clang fp reassociate(off)
    const float r = __builtin_amdgcn_rcpf(b);
    const float q = a * r;
    return __builtin_fmaf(__builtin_fmaf(-b, q, a), r, q);
}

// grid = ceil(S / 4), block 256: one wave per token.  x [S][ldx], wr [E][D] fp32 (router rows times the norm weight: the product of two
// 16-bit numbers is exact in fp32, so folding the norm costs the router no rounding -- a rounded fold moves logits by ~1e-3 relative and
// flips top-k decisions whose margin is a few 1e-3).  Outputs ids / wts [S][k], rstd [S]
// (or null), logits [S][E] fp32 (or null).
__global__ __launch_bounds__(256) void moe_router_kernel(const bf16_t* __restrict__ x, int ldx, const float* __restrict__ wr, int S, int D, int E,
                                                         int k, float eps, int* __restrict__ ids, float* __restrict__ wts,
                                                         float* __restrict__ rstd_out, float* __restrict__ logits) {
#pragma clang fp reassociate(off)
    const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= S) return;                                            // (no barriers in this kernel)
    const bf16_t* xr = x + (size_t)t * ldx;
    const int nvec = D >> 3;
    float ss = 0.f;
    for (int v = lane; v < nvec; v += 64) {
        float f[8];
        unpack8(*(const u32x4*)(xr + (size_t)v * 8), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(f[j], f[j], ss);
    }
    ss = wave_sum(ss);
    const float rstd = rsqrtf(ss / (float)D + eps);
    float mine = -__builtin_inff();                                        // lane e holds logit e
    for (int e = 0; e < E; ++e) {
        const float* w = wr + (size_t)e * D;
        float a = 0.f;
        for (int v = lane; v < nvec; v += 64) {
            float f[8];
            unpack8(*(const u32x4*)(xr + (size_t)v * 8), f);
            const f32x4 w0 = *(const f32x4*)(w + (size_t)v * 8), w1 = *(const f32x4*)(w + (size_t)v * 8 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) a = __builtin_fmaf(f[j], w0[j], a);
#pragma unroll
            for (int j = 0; j < 4; ++j) a = __builtin_fmaf(f[j + 4], w1[j], a);
        }
        a = wave_sum(a) * rstd;
        if (lane == e) mine = a;
    }
    if (logits && lane < E) logits[(size_t)t * E + lane] = mine;
    const float mx = wave_max(mine);
    const float ex = lane < E ? __expf(mine - mx) : 0.f;
    const float p = ex / wave_sum(ex);
    bool taken = false;
    float sel_v[MOE_MAX_K];
    int sel_i[MOE_MAX_K];
#pragma unroll
    for (int j = 0; j < MOE_MAX_K; ++j) {
        if (j >= k) break;
        float v = (lane < E && !taken) ? p : -1.f;
        int i = lane;
        moe_argmax_pair(v, i);
        sel_v[j] = v; sel_i[j] = i;
        if (lane == i) taken = true;
    }
    if (lane == 0) {
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) sum += sel_v[j];
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) {
                ids[(size_t)t * k + j] = sel_i[j];
                wts[(size_t)t * k + j] = moe_div(sel_v[j], sum);
            }
        if (rstd_out) rstd_out[t] = rstd;
    }
}

// ONE workgroup of 1024 threads.  ids [S][k] -> counts [E], offs [E + 1] (offs[e + 1] - offs[e] = counts[e] rounded up to BM),
// gather [P] (permuted row -> token, -1 for padding and for rows past offs[E]), inv [S][k] ((token, slot) -> permuted row).
__global__ __launch_bounds__(1024) void moe_scan_kernel(const int* __restrict__ ids, int S, int E, int k, int BM, int P,
                                                        int* __restrict__ counts, int* __restrict__ offs, int* __restrict__ gather,
                                                        int* __restrict__ inv) {
    __shared__ int sid[MOE_SCAN_MAX];
    __shared__ int cnt[MOE_MAX_E], off[MOE_MAX_E + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = S * k;
    for (int i = tid; i < n; i += 1024) sid[i] = ids[i];
    __syncthreads();
    // slot of expert e in token t's row, or -1 (the k ids of a token are distinct)
    auto slot_of = [&](int t, int e) {
        int s = -1;
        if (t < S)
            for (int j = 0; j < k; ++j)
                if (sid[t * k + j] == e) s = j;
        return s;
    };
    for (int e = wave; e < E; e += 16) {
        int c = 0;
        for (int t0 = 0; t0 < S; t0 += 64)
            c += __popcll(__ballot(slot_of(t0 + lane, e) >= 0));
        if (lane == 0) cnt[e] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int o = 0;
        for (int e = 0; e < E; ++e) {
            off[e] = o;
            offs[e] = o;
            counts[e] = cnt[e];
            o += (cnt[e] + BM - 1) / BM * BM;
        }
        off[E] = o;
        offs[E] = o;
    }
    __syncthreads();
    for (int e = wave; e < E; e += 16) {
        int r = off[e];
        for (int t0 = 0; t0 < S; t0 += 64) {
            const int t = t0 + lane, s = slot_of(t, e);
            const unsigned long long b = __ballot(s >= 0);
            if (s >= 0) {
                const int row = r + __popcll(b & ((1ull << lane) - 1ull));
                gather[row] = t;
                inv[t * k + s] = row;
            }
            r += __popcll(b);
        }
        for (int row = r + lane; row < off[e + 1]; row += 64) gather[row] = -1;
    }
    for (int row = off[E] + tid; row < P; row += 1024) gather[row] = -1;
}

// grid = P, block 256: xg[p] = x[gather[p]], rn[p] = (0, rstd[gather[p]]); padding rows are left alone (no GEMM tile reads them:
// the body clamps its A rows to the expert's count).
__global__ __launch_bounds__(256) void moe_gather_kernel(const bf16_t* __restrict__ x, int ldx, const int* __restrict__ gather,
                                                         const float* __restrict__ rstd, int D, bf16_t* __restrict__ xg,
                                                         float* __restrict__ rn) {
    const int p = blockIdx.x, t = gather[p];
    if (t < 0) return;
    const bf16_t* src = x + (size_t)t * ldx;
    bf16_t* dst = xg + (size_t)p * D;
    for (int v = threadIdx.x; v < (D >> 3); v += 256) *(u32x4*)(dst + (size_t)v * 8) = *(const u32x4*)(src + (size_t)v * 8);
    if (threadIdx.x == 0) { rn[2 * (size_t)p] = 0.f; rn[2 * (size_t)p + 1] = rstd[t]; }
}

// The grouped GEMM.  g = the call's GemmArgs over the WHOLE permuted row space (A = permuted rows [P][lda], C [P][ldc], W = expert 0,
// row_norm [P][2] or null); w_stride = elements between two experts' weight matrices; rt_cap = row tiles of the worst case.
struct MoeGemmArgs {
    GemmArgs g;
    const int* offs;          // [E + 1]
    const int* counts;        // [E]
    long long w_stride;
    int E, rt_cap;
};

template <bool SWIGLU>
__global__ __launch_bounds__(512, 1) void moe_gemm_kernel(MoeGemmArgs q) {
    // consecutive logical ids = the row tiles of one column panel, on one XCD: an expert's tiles share its W panel in that L2
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int rt = t % q.rt_cap, tn = t / q.rt_cap;
    const int m0 = rt * MOE_BM;
    if (m0 >= __builtin_amdgcn_readfirstlane(q.offs[q.E])) return;                // past the last expert's padded rows
    int e = 0;
    while (e + 1 < q.E && __builtin_amdgcn_readfirstlane(q.offs[e + 1]) <= m0) ++e;
    const int row0 = __builtin_amdgcn_readfirstlane(q.offs[e]), cnt = __builtin_amdgcn_readfirstlane(q.counts[e]);
    const int rows = cnt - (m0 - row0);
    if (rows <= 0) return;
    GemmArgs p = q.g;
    p.A = q.g.A + (size_t)m0 * q.g.lda;
    p.W = q.g.W + (size_t)e * q.w_stride + (size_t)tn * GEMM_BN * q.g.ldw;
    p.M = rows < MOE_BM ? rows : MOE_BM;
    p.N = GEMM_BN;
    const size_t ccol = SWIGLU ? (size_t)tn * (GEMM_BN / 2) : (size_t)tn * GEMM_BN;
    p.C = (void*)((bf16_t*)q.g.C + (size_t)m0 * q.g.ldc + ccol);
    if (q.g.row_norm) p.row_norm = q.g.row_norm + 2 * (size_t)m0;
    p.tiles_m = 1; p.tiles_n = 1;
    gemm_l8_16_body<SWIGLU>(p, 0, 1);
}

// grid = S, block 256 (out may be x1: a thread reads each of its vectors before it writes it).  x[t] = bf16(x1[t] + sum_j w_tj * y[inv[t][j]]) (fp32, slot order); rn[t] = (0, rstd of the stored row).
__global__ __launch_bounds__(256) void moe_combine_kernel(const bf16_t* x1, int ldx1, const bf16_t* __restrict__ y, int ldy,
                                                          const int* __restrict__ inv, const float* __restrict__ wts, int k, int D, float eps,
                                                          bf16_t* out, int ldo, float* __restrict__ rn) {
#pragma clang fp reassociate(off)
    __shared__ float red[4];
    const int t = blockIdx.x, tid = threadIdx.x;
    int rows[MOE_MAX_K];
    float w[MOE_MAX_K];
#pragma unroll
    for (int j = 0; j < MOE_MAX_K; ++j)
        if (j < k) { rows[j] = inv[(size_t)t * k + j]; w[j] = wts[(size_t)t * k + j]; }
    float ss = 0.f;
    for (int v = tid; v < (D >> 3); v += 256) {
        float acc[8], f[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) {
                unpack8(*(const u32x4*)(y + (size_t)rows[j] * ldy + (size_t)v * 8), f);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(w[j], f[i], acc[i]);
            }
        unpack8(*(const u32x4*)(x1 + (size_t)t * ldx1 + (size_t)v * 8), f);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = f[i] + acc[i];
        const u32x4 o = pack8(acc);
        *(u32x4*)(out + (size_t)t * ldo + (size_t)v * 8) = o;
        unpack8(o, f);
#pragma unroll
        for (int i = 0; i < 8; ++i) ss = __builtin_fmaf(f[i], f[i], ss);
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    if (tid == 0 && rn) {
        rn[2 * (size_t)t] = 0.f;
        rn[2 * (size_t)t + 1] = rsqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)D + eps);
    }
}

// Decode gate/up: grid = (ceil(I / 4), k), block 256, dynamic LDS = K * 2.  Slot j = blockIdx.y runs the SwiGLU GEMV of expert ids[j]
// (w = wgu + ids[j] * w_stride, packed per expert like the dense gate/up) on RMSNorm(x) into a + j * lda.
__global__ __launch_bounds__(256) void moe_gemv_gu_kernel(GemvArgs g, const int* __restrict__ ids, long long w_stride, int lda) {
    const int j = blockIdx.y;
    const int e = __builtin_amdgcn_readfirstlane(ids[j]);
    GemvArgs p = g;
    p.W = g.W + (size_t)e * w_stride;
    p.y = (void*)((bf16_t*)g.y + (size_t)j * lda);
    gemv_bf16_body<true, false, 1>(p, blockIdx.x);
}

// Decode down: grid = ceil(N / 4), block 256, dynamic LDS = KS * K * 2 (the k SwiGLU rows a [KS][K]).  One output row per wave:
// the KS experts' dot products of that row are streamed together, then y[n] = bf16(res[n] + sum_j w_j dot_j) (fp32, slot order).
// (the body takes the workgroup index and one token's pointers so that k_moe_skinny.h can run it per token of a batch)
template <int KS>
__device__ __forceinline__ void moe_gemv_down_body(const bf16_t* __restrict__ W, long long w_stride, int ldw, const bf16_t* __restrict__ a,
                                                   const int* __restrict__ ids, const float* __restrict__ wts,
                                                   const bf16_t* __restrict__ res, bf16_t* __restrict__ y, int N, int K, int bid) {
#pragma clang fp reassociate(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char vl2_smem[];
    bf16_t* as = (bf16_t*)vl2_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nvec = K >> 3;
    for (int v = tid; v < KS * nvec; v += 256) *(u32x4*)(as + (size_t)v * 8) = *(const u32x4*)(a + (size_t)v * 8);
    const bf16_t* wp[KS];
    float wj[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        wp[s] = W + (size_t)__builtin_amdgcn_readfirstlane(ids[s]) * w_stride;
        wj[s] = wts[s];
    }
    __syncthreads();
    const int n = bid * 4 + wave;
    if (n >= N) return;
    float acc[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) acc[s] = 0.f;
    for (int v0 = 0; v0 < nvec; v0 += 64 * 8) {
        u32x4 wv[KS][8];
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int v = v0 + i * 64 + lane;
                if (v < nvec) wv[s][i] = __builtin_nontemporal_load((const u32x4*)(wp[s] + (size_t)n * ldw + (size_t)v * 8));
            }
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int v = v0 + i * 64 + lane;
                if (v < nvec) {
                    const u32x4 xv = *(const u32x4*)(as + ((size_t)s * nvec + v) * 8);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[s] = dot2_bf16(wv[s][i][q], xv[q], acc[s]);
                }
            }
    }
    float o = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) o = __builtin_fmaf(wj[s], wave_sum(acc[s]), o);
    if (lane == 0) {
        if (res) o = bf2f(res[n]) + o;
        y[n] = f2bf(o);
    }
}

template <int KS>
__global__ __launch_bounds__(256) void moe_gemv_down_kernel(const bf16_t* __restrict__ W, long long w_stride, int ldw, const bf16_t* __restrict__ a,
                                                            const int* __restrict__ ids, const float* __restrict__ wts,
                                                            const bf16_t* __restrict__ res, bf16_t* __restrict__ y, int N, int K) {
    moe_gemv_down_body<KS>(W, w_stride, ldw, a, ids, wts, res, y, N, K, blockIdx.x);
}
