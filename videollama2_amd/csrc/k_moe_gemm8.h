// Tiled grouped GEMM on the fp8 expert weights (W8A16) for the batched decode step of the Mixtral sparse MoE block:
//   C[p, n] = epilogue( scale[e(p)][n] * (A[p, :] . q[e(p)][n, :]) )   over the permuted rows p of k_moe.h moe_scan_kernel (row tile 128).
//
// gemm_l8_16_w8_body is the 128 x 128 tile of k_gemm9.h gemm_l8_16_body -- eight waves, wave tile 32 x 64, v_mfma_f32_16x16x32 in the element
// type of the build, an LDS-DMA ring with one raw barrier per 64-deep K-tile, the empty-wave skip, gemm_row_stats / gemm_park_row_stats, the
// LDS patch epilogue gemm_store_patch -- with the W operand arriving as OCP e4m3fn bytes.  The weights are the stacks of ops.moe_quant_fp8:
// q [E, N, K] bytes with one power-of-two fp32 scale per expert and output row (k_moe_fp8.h); activations stay 16-bit, products and sums fp32.
// The A half of a stage (16 KiB: image, piece map, clamp of the rows past M, fragment read) is gemm_l8_16_body's, literally.
//
// W staging.  A K-tile's W slab is 128 rows x 64 k = 8 KiB of bytes = 512 pieces of 16 B (16 k of one row): ONE LDS-DMA piece per lane and
// stage, where the 16-bit body moves two of 8 k.  The image is lane-linear (LDS-DMA writes base + lane * 16), so the swizzle lives on the
// per-lane SOURCE address and on the fragment read's address: a 256-B LDS bank row R holds four tile rows 4 R .. 4 R + 3 = 16 slots of 16 B,
// and slot s = 4 (row & 3) + c (c = 16-k chunk 0..3 of the row) is stored at s ^ (R & 3):
//     byte offset(row, c) = (16 R + (s ^ (R & 3))) * 16,   R = row >> 2,  s = 4 (row & 3) + c.
// Fragment read: ds_read_b64 per lane and block; lane l of k-step kk reads the 8 bytes k = 32 kk + 8 (l >> 4) .. + 7 of row 16 b + (l & 15),
// i.e. chunk c = 2 kk + (l >> 5), half (l >> 4) & 1 of its slot.  A 32-lane half reads 16 rows = bank rows R0 .. R0 + 3 (R0 % 4 == 0) at ONE
// chunk c: bank row R0 + i supplies the four slots 4 j + (c ^ i), j = 0..3 -- the low two slot bits differ between the four bank rows, so the
// 16 slots are all different, the 32 lanes x 8 B cover each of the 64 banks exactly once: 0 bank conflicts (bank = (addr / 4) % 64).
//
// Conversion: the 8 bytes become the 8 elements of the B fragment in registers (k_skinny_fp8.h fp8x8_to_frag: v_cvt_pk_f32_fp8 and the pack to
// the element type; every e4m3fn value is exact in bf16 and in half).
//
// k order, the contract: fragment rows 16 b + (lane & 15), k = 32 step + 8 (lane >> 4) + j, k-steps in ascending k -- gemm9_body's index
// function, so every dot product is the same sequence of 32-product accumulation steps as in moe_gemm_kernel, and scaling by a power of two
// is exact: the output is bit for bit moe_gemm_kernel on the dequantised stack q * scale (which the 16-bit element holds exactly).
//
// Ring: MOE8_STAGES = 6 stages of 24 KiB (A 16 KiB + W 8 KiB) = 144 KiB of the 160 KiB of LDS (the epilogue's patches, 69 KiB, reuse the
// ring); five stages in flight = 40 KiB of weight bytes per workgroup, where the 16-bit ring copied as is (4 stages) would keep 24 KiB.
// A stage is 3 DMA pieces per wave (2 A + 1 W), so the wait before K-tile kt is vmcnt(3 * newer), newer = the stages issued behind kt
// (at most MOE8_STAGES - 2).  Protocol of gemm_l8_16_body: raw s_barrier only while a DMA is in flight; the buffer refilled behind the
// barrier of K-tile kt is the one read in kt - 1.  Any K % 64 == 0: fewer K-tiles than stages simply leave stages unused.
#pragma once
#include "k_gemm9.h"
#include "k_moe.h"
#include "k_skinny_fp8.h"

#define MOE8_STAGES 6
#define MOE8_STAGE_BYTES 24576          // A 16384 (gemm_l8_16_body's image) + W 8192 (bytes)
#define MOE8_LDS_BYTES (MOE8_STAGES * MOE8_STAGE_BYTES)

__device__ __forceinline__ int moe8_w_off(int row, int chunk) {      // byte offset of the 16-B piece `chunk` (16 k) of W tile row `row`
    const int R = row >> 2;
    const int s = ((row & 3) << 2) | chunk;
    return ((R << 4) + (s ^ (R & 3))) << 4;
}

// p: gemm_l8_16_body's arguments (p.W unused); Q = the e4m3fn rows [N, ldq] of the tile's expert, p.col_scale = their scales
template <bool SWIGLU>
__device__ __forceinline__ void gemm_l8_16_w8_body(const GemmArgs& p, const uint8_t* __restrict__ Q, int ldq, int bid, int nwg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vl2_smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;                    // wm 0..3 (32 rows each), wn 0..1 (64 columns each)
    const int t = xcd_remap(bid, nwg);
    const int tm = t % p.tiles_m, tn = t / p.tiles_m;
    const int m0 = tm * GEMM_BM, n0 = tn * GEMM_BN;
    const int nt = p.K / GEMM_BK;
    const f32x2 rst = gemm_row_stats(p, m0, tid, GEMM_BM);
    const bool live = m0 + wm * 32 < p.M;                       // (gemm_l8_16_body: a wave whose 32 rows all lie past M moves its pieces and meets the barriers only)

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, 0x7fffffff, 0x00020000);
    const auto rsQ = __builtin_amdgcn_make_buffer_rsrc((void*)Q, 0, 0x7fffffff, 0x00020000);
    unsigned a_vo[2], w_vo;                                     // 2 A pieces (piece i = +64 rows) + 1 W piece per wave
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int slot = ((i * 8 + wave) << 6) + lane;
        const int R = slot >> 4, sx = (slot & 15) ^ (R & 15);
        int am = m0 + 2 * R + (sx >> 3);
        am = am < p.M ? am : p.M - 1;
        a_vo[i] = ((unsigned)am * (unsigned)p.lda + (sx & 7) * 8) * 2;
    }
    {
        const int slot = (wave << 6) + lane;                    // 0..511: bank row R = slot >> 4 holds tile rows 4 R .. 4 R + 3
        const int R = slot >> 4, sx = (slot & 15) ^ (R & 3);
        w_vo = (unsigned)(n0 + 4 * R + (sx >> 2)) * (unsigned)ldq + (sx & 3) * 16;
    }
    const int frow = lane & 15, fchk = lane >> 4;
    unsigned a_rd[2][2], b_rd[2][4];                            // [k-step][block]
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int i = 0; i < 2; ++i) a_rd[kk][i] = gemm_lds_off(wm * 32 + i * 16 + frow, kk * 4 + fchk);
#pragma unroll
        for (int j = 0; j < 4; ++j) b_rd[kk][j] = 16384 + moe8_w_off(wn * 64 + j * 16 + frow, kk * 2 + (fchk >> 1)) + (fchk & 1) * 8;
    }
    auto stage = [&](int kt, unsigned lds_buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(vl2_smem + lds_buf + ((i * 8 + wave) << 10)),
                                                     16, a_vo[i], (unsigned)kt * (GEMM_BK * 2), 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQ, (__attribute__((address_space(3))) void*)(vl2_smem + lds_buf + 16384 + (wave << 10)),
                                                 16, w_vo, (unsigned)kt * GEMM_BK, 0, 0);
    };
#pragma unroll
    for (int s = 0; s < MOE8_STAGES - 1; ++s)
        if (s < nt) stage(s, (unsigned)s * MOE8_STAGE_BYTES);
    unsigned cur = 0, fill = (MOE8_STAGES - 1) * MOE8_STAGE_BYTES;      // byte offsets of buffer kt % STAGES and (kt + STAGES - 1) % STAGES
    for (int kt = 0; kt < nt; ++kt) {
        const int newer = nt - 1 - kt < MOE8_STAGES - 2 ? nt - 1 - kt : MOE8_STAGES - 2;
        if (newer >= 4) VL2_WAIT_VMCNT(12); else if (newer == 3) VL2_WAIT_VMCNT(9); else if (newer == 2) VL2_WAIT_VMCNT(6);
        else if (newer == 1) VL2_WAIT_VMCNT(3); else VL2_WAIT_VMCNT(0);
        VL2_PHASE_BARRIER();                                        // everyone's pieces of tile kt landed; the buffer read in kt - 1 is free
        if (kt + MOE8_STAGES - 1 < nt) stage(kt + MOE8_STAGES - 1, fill);
        const unsigned lds_buf = cur;
        cur = cur + MOE8_STAGE_BYTES == MOE8_LDS_BYTES ? 0u : cur + MOE8_STAGE_BYTES;
        fill = fill + MOE8_STAGE_BYTES == MOE8_LDS_BYTES ? 0u : fill + MOE8_STAGE_BYTES;
        if (!live) continue;                                        // (see `live` above: loads and barriers only)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[2], fb[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *(const bf16x8*)(vl2_smem + lds_buf + a_rd[kk][i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = fp8x8_to_frag(*(const u32x2*)(vl2_smem + lds_buf + b_rd[kk][j]));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = VL2_MFMA16(fa[i], fb[j], acc[i][j]);
        }
    }
    VL2_WAIT_LGKMCNT0();
    VL2_PHASE_BARRIER();

    float* ep = (float*)vl2_smem + wave * (32 * 68);
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                ep[(ib * 16 + 4 * (lane >> 4) + r) * 68 + jb * 16 + (lane & 15)] = acc[ib][jb][r];
    float* rowtab = (float*)vl2_smem + 8 * (32 * 68);
    gemm_park_row_stats(p, rowtab, rst, tid, GEMM_BM);
    __syncthreads();
    gemm_store_patch<ACT_NONE, SWIGLU, false>(p, ep, m0 + wm * 32, n0 + wn * 64, lane, rowtab, wm * 32);
}

// The grouped form: moe_gemm_kernel's dispatch (k_moe.h) on the fp8 stacks.  g = the call's GemmArgs over the whole permuted row space (A, C,
// row_norm; W unused); q = expert 0's bytes [N, ldq], q_stride bytes between two experts; scale = expert 0's row scales, s_stride floats apart.
struct MoeGemm8Args {
    GemmArgs g;
    const int* offs;          // [E + 1]
    const int* counts;        // [E]
    const uint8_t* q;
    const float* scale;
    long long q_stride, s_stride;
    int ldq, E, rt_cap;
};

template <bool SWIGLU>
__global__ __launch_bounds__(512, 1) void moe_gemm8_kernel(MoeGemm8Args a) {
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int rt = t % a.rt_cap, tn = t / a.rt_cap;
    const int m0 = rt * MOE_BM;
    if (m0 >= __builtin_amdgcn_readfirstlane(a.offs[a.E])) return;                // past the last expert's padded rows
    int e = 0;
    while (e + 1 < a.E && __builtin_amdgcn_readfirstlane(a.offs[e + 1]) <= m0) ++e;
    const int row0 = __builtin_amdgcn_readfirstlane(a.offs[e]), cnt = __builtin_amdgcn_readfirstlane(a.counts[e]);
    const int rows = cnt - (m0 - row0);
    if (rows <= 0) return;                                                        // an idle expert: before any weight byte is requested
    GemmArgs p = a.g;
    p.A = a.g.A + (size_t)m0 * a.g.lda;
    p.M = rows < MOE_BM ? rows : MOE_BM;
    p.N = GEMM_BN;
    const size_t ccol = SWIGLU ? (size_t)tn * (GEMM_BN / 2) : (size_t)tn * GEMM_BN;
    p.C = (void*)((bf16_t*)a.g.C + (size_t)m0 * a.g.ldc + ccol);
    if (a.g.row_norm) p.row_norm = a.g.row_norm + 2 * (size_t)m0;
    p.col_scale = a.scale + (size_t)e * a.s_stride + (size_t)tn * GEMM_BN;
    p.tiles_m = 1; p.tiles_n = 1;
    gemm_l8_16_w8_body<SWIGLU>(p, a.q + (size_t)e * a.q_stride + (size_t)tn * GEMM_BN * a.ldq, a.ldq, 0, 1);
}
