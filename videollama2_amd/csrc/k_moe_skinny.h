// Batched decode of the Mixtral sparse MoE block: nb tokens per step, every routing table on the device.
//
// Few tokens (nb < MOE_GEMM_BATCH): the solo step's GEMVs with a token index in the grid (moe_gemv_gu_rows_kernel,
// moe_gemv_down_rows_kernel): the SAME bodies as k_moe.h's solo kernels, so a row has the solo step's bits by construction.
//
// 5 .. 64 tokens: moe_skinny_kernel, the grouped form of k_skinny.h gemm_skinny_body.  grid = (N / 64, KS, E), block 256: workgroup
// (x, y, e) streams K slice y of 64 weight rows of expert e GEMV-style into v_mfma_f32_16x16x32_bf16 against the rows routed to e.
//   * the expert's row count and first permuted row come from the device tables (moe_scan_kernel with a row tile of 1: offs[e + 1] - offs[e]
//     = counts[e], offs[E] = nb * k), read wave-uniform; an expert nobody chose returns before any weight load and costs no bytes;
//   * fragment row r stages A[rowmap ? rowmap[row0 + r] : row0 + r] for r < count and zeros above; 16-row groups above the count issue
//     no MFMA; the fp32 partials of permuted rows row0 .. row0 + count - 1 alone are stored (row0 + count is the next expert's);
//   * the K split, the weight loads (the SkinnyWBf16 policy), the MFMA order over K and the reduce (skinny_reduce_kernel over the nb * k
//     permuted rows) are gemm_skinny_kernel's.  MFMA rows are independent and the split is a function of N and K only, so a permuted row is
//     bit for bit gemm_skinny_kernel on that one row with the expert's weights.
// MT (16-row groups staged) is chosen on the host from nb: an expert can receive every token, and the counts never reach the host.
#pragma once
#include "k_moe.h"
#include "k_skinny.h"

// (GA = the weight format's argument struct, k_skinny.h: SkinnyArgs here, Skinny8Args for the fp8 expert weights of k_moe_fp8.h, Skinny4Args
// for the MXFP4 expert weights of k_moe_mxfp4.h)
template <class GA>
struct MoeSkinnyArgsT {
    GA g;                     // A [a_rows, lda], W = expert 0, part [KS][R][N], M unused, N, K, lda, ldw, kslice, kchunk
    const int* counts;        // [E]
    const int* offs;          // [E + 1]
    const int* rowmap;        // [R] permuted row -> row of A, or null (A holds the permuted rows)
    long long w_stride;
    int R, a_rows;            // permuted rows (nb * k), rows of A
    long long s_stride;       // MXFP4 only: bytes between two experts' scale arrays (the 16-bit and fp8 policies ignore it)
};
typedef MoeSkinnyArgsT<SkinnyArgs> MoeSkinnyArgs;

// WF = the weight-format policy of gemm_skinny_body (k_skinny.h); WF::at_expert moves the arguments to expert e's matrix
template <int MT, class WF = SkinnyWBf16>
__global__ __launch_bounds__(256) void moe_skinny_kernel(MoeSkinnyArgsT<typename WF::Args> q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vl2_smem[];
    constexpr int Mp = 16 * MT, NL = WF::NL;
    const int e = blockIdx.z;
    const int row0 = __builtin_amdgcn_readfirstlane(q.offs[e]);
    int cnt = __builtin_amdgcn_readfirstlane(q.counts[e]);
    // tables that the scan wrote satisfy all of this; anything else must not reach past the buffers
    if (cnt > Mp) cnt = Mp;
    if (row0 < 0 || row0 > q.R) return;
    if (cnt > q.R - row0) cnt = q.R - row0;
    if (cnt <= 0) return;                                  // an idle expert: no weight load
    typename WF::Args p = q.g;
    WF::at_expert(p, e, q.w_stride, q.s_stride);
    bf16_t* xs = (bf16_t*)vl2_smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * 64 + wave * 16;
    const int k0 = blockIdx.y * p.kslice;
    const int pitch = p.kchunk + 8;
    const int l15 = lane & 15, lg = lane >> 4;
    const WF w(p, n0 + l15, k0, lg);
    const int live = (cnt + 15) & ~15;                     // fragment rows that an MFMA reads

    f32x4v acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = f32x4v{0.f, 0.f, 0.f, 0.f};

    const int cvec = p.kchunk >> 3;
    for (int kc = 0; kc < p.kslice; kc += p.kchunk) {
        const int nstep = p.kchunk >> 5;
        typename WF::word wv[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i)
            if (i < nstep) wv[i] = w.load(kc, i);
        __syncthreads();
        for (int v = tid; v < live * cvec; v += 256) {
            const int r = v / cvec, c = v - r * cvec;
            u32x4 x = u32x4{0u, 0u, 0u, 0u};
            if (r < cnt) {
                const int src = q.rowmap ? q.rowmap[row0 + r] : row0 + r;
                if ((unsigned)src < (unsigned)q.a_rows) x = *(const u32x4*)(p.A + (size_t)src * p.lda + k0 + kc + c * 8);
            }
            *(u32x4*)(xs + (size_t)r * pitch + c * 8) = x;
        }
        __syncthreads();
        for (int s0 = 0; s0 < nstep; s0 += NL) {
            if (s0) {
#pragma unroll
                for (int i = 0; i < NL; ++i)
                    if (s0 + i < nstep) wv[i] = w.load(kc, s0 + i);
            }
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                if (s0 + i < nstep) {
                    const bf16x8 bfrag = WF::frag(wv[i]);
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        if (m * 16 < cnt) {
                            const bf16x8 afrag = *(const bf16x8*)(xs + (size_t)(m * 16 + l15) * pitch + (s0 + i) * 32 + lg * 8);
                            acc[m] = VL2_MFMA16(afrag, bfrag, acc[m]);
                        }
                    }
                }
            }
        }
    }
    // D[row = (lane>>4)*4 + r][col = lane&15] -> permuted row row0 + row
    float* dst = p.part + ((size_t)blockIdx.y * q.R + row0) * p.N;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m * 16 + lg * 4 + r;
            if (row < cnt) dst[(size_t)row * p.N + n0 + l15] = acc[m][r];
        }
}

// Gate/up of every (token, slot) pair in one launch: grid = (ceil(I / 4), k, S), block 256, dynamic LDS = K * 2.  Pair (t, j) runs
// moe_gemv_gu_kernel's body on token t's row with expert ids[t][j] into a[t * k + j].
__global__ __launch_bounds__(256) void moe_gemv_gu_rows_kernel(GemvArgs g, const int* __restrict__ ids, long long w_stride, int lda, int ldx) {
    const int j = blockIdx.y, k = gridDim.y, t = blockIdx.z;
    const int e = __builtin_amdgcn_readfirstlane(ids[t * k + j]);
    GemvArgs p = g;
    p.W = g.W + (size_t)e * w_stride;
    p.x = g.x + (size_t)t * ldx;
    p.y = (void*)((bf16_t*)g.y + ((size_t)t * k + j) * lda);
    gemv_bf16_body<true, false, 1>(p, blockIdx.x);
}

// Down of every token in one launch: grid = (ceil(N / 4), S), block 256, dynamic LDS = KS * K * 2.  Token t runs moe_gemv_down_kernel's
// body on its KS SwiGLU rows a[t * KS ..], its ids / weights and its residual row.
template <int KS>
__global__ __launch_bounds__(256) void moe_gemv_down_rows_kernel(const bf16_t* __restrict__ W, long long w_stride, int ldw, const bf16_t* __restrict__ a,
                                                                 const int* __restrict__ ids, const float* __restrict__ wts,
                                                                 const bf16_t* __restrict__ res, int ldres, bf16_t* __restrict__ y, int ldy, int N, int K) {
    const int t = blockIdx.y;
    moe_gemv_down_body<KS>(W, w_stride, ldw, a + (size_t)t * KS * K, ids + t * KS, wts + t * KS, res ? res + (size_t)t * ldres : nullptr,
                           y + (size_t)t * ldy, N, K, blockIdx.x);
}
