// Tiled grouped GEMM on the MXFP4 expert weights (W4A16) for the batched decode step of the Mixtral sparse MoE block:
//   C[p, n] = epilogue( A[p, :] . W~[e(p)][n, :] ),  W~[n][k] = 2^e(n, k / 32) * E2M1(q[n][k])   over the permuted rows p of moe_scan_kernel.
//
// gemm_l8_16_w4_body is the W4 twin of k_moe_gemm8.h gemm_l8_16_w8_body: gemm_l8_16_body's 128 x 128 tile -- eight waves, wave tile 32 x 64,
// v_mfma_f32_16x16x32 in the element type of the build, an LDS-DMA ring with one raw barrier per 64-deep K-tile, the empty-wave skip,
// gemm_row_stats / gemm_park_row_stats, the LDS patch epilogue gemm_store_patch -- with the W operand arriving as the stacks of
// ops.moe_quant_mxfp4 (k_mxfp4.h): q [E, N, K / 2] bytes of two E2M1 codes, s [E, N, K / 32] E8M0 bytes; activations stay 16-bit, products and
// sums fp32.  The A half of a stage (16 KiB: image, piece map, clamp of the rows past M, fragment read) is gemm_l8_16_body's, literally.
//
// W staging.  A K-tile's W slab is 128 rows x 64 k = 128 x 32 B of codes = 256 pieces of 16 B, and 128 x 2 scale bytes.  One 16-B piece is 32
// codes = ONE scale block of one row.  Waves 0..3 move one code piece per lane, waves 4..7 one scale BYTE per lane (buffer_load_ubyte ... lds):
// every wave issues 3 LDS-DMA pieces per stage (2 A + 1), so the fp8 body's vmcnt(3 * newer) protocol holds unchanged.  No ordinary global load
// lives inside the ring (the compiler would drain the ring with vmcnt(0) at its first use).
//
// Code image (4 KiB at +16384).  The image is lane-linear (LDS-DMA writes base + lane * 16), so the swizzle lives on the per-lane SOURCE
// address and on the fragment read's address: a 256-B LDS bank row R holds the eight tile rows 8 R .. 8 R + 7 = 16 slots of 16 B, and slot
// s = 2 (row & 7) + blk (blk = which 32-k block of the K-tile) is stored at s ^ (R & 1):
//     byte offset(row, blk) = (16 R + (s ^ (R & 1))) * 16,   R = row >> 3,  s = 2 (row & 7) + blk.
// Neighbouring lanes fetch the two blocks of one row: 32 contiguous source bytes.
// Fragment read: ds_read_b32 per lane, block and k-step; lane l of k-step kk reads the dword of the 8 codes k = 32 kk + 8 (l >> 4) .. + 7 of row
// 16 b + (l & 15): dword l >> 4 of slot (row, kk).  A 32-lane half reads 16 rows = the bank rows R0, R0 + 1 (R0 even) at ONE blk = kk: bank row
// R0 supplies the slots 2 i + kk, bank row R0 + 1 the slots 2 i + (kk ^ 1), i = 0..7 -- the 16 slot positions are all different, so the 16 rows
// cover the 64 banks in disjoint groups of four and the half's two dword indices (l >> 4 = 0, 1 or 2, 3) pick two different banks of each
// group: 32 lanes, 32 banks, 0 bank conflicts (bank = (addr / 4) % 64).  The other half reads the other two banks of each group.
//
// Scale image (1 KiB at +20480).  A 1-byte LDS-DMA piece writes lane l's byte, zero-extended, as the DWORD at base + 4 l -- confirmed on the
// device (every exact case of tests/test_gpu_moe_gemm4.py fails if the byte is read anywhere else), and NOT base + lane * size as the 4-, 12-
// and 16-byte pieces would suggest.  The read below takes the low byte.  So the 256 scales of a stage take 256
// dwords.  Lane l of wave 4 + w carries index i = 64 w + l = 2 row + blk (neighbouring lanes fetch neighbouring source bytes); the fragment
// read is one ds_read_u8 per block and k-step at 4 (2 row + kk): the 16 rows of a fragment hit the 16 banks 2 (row & 31) + kk, the four
// lanes of one row read the same address (a broadcast).
//
// Conversion: B fragment = mx4_cvt8(dword of 8 codes, mx4_scale(byte)) = E2M1 * 2^e in the element type (k_mxfp4.h: exact in bf16; exact in
// half while inside half's range).  A k-step of 32 is exactly one scale block, so the 8 elements of a fragment share one scale byte.
//
// k order, the contract: fragment rows 16 b + (lane & 15), k = 32 step + 8 (lane >> 4) + j, k-steps in ascending k -- gemm9_body's index
// function, so every dot product is the same sequence of 32-product accumulation steps as in moe_gemm_kernel: the output is bit for bit
// moe_gemm_kernel on the dequantised stack (which the 16-bit element holds exactly, see above).
//
// Ring: MOE4_STAGES = 7 stages of 21 KiB (A 16 KiB + codes 4 KiB + scales 1 KiB) = 147 KiB of the 160 KiB of LDS (the epilogue's patches,
// 69 KiB, reuse the ring); six stages in flight = 24 KiB of code bytes (+ 1.5 KiB of scales) = 48 Ki weights per workgroup, beside the fp8
// body's 40 KiB (40 Ki weights) and the 16-bit body's 48 KiB (24 Ki weights).  The wait before K-tile kt is vmcnt(3 * newer), newer = the
// stages issued behind kt (at most MOE4_STAGES - 2).  Protocol of gemm_l8_16_body: raw s_barrier only while a DMA is in flight; the buffer
// refilled behind the barrier of K-tile kt is the one read in kt - 1.  Any K % 64 == 0: fewer K-tiles than stages leave stages unused.
#pragma once
#include "k_gemm9.h"
#include "k_moe.h"
#include "k_mxfp4.h"

#define MOE4_STAGES 7
#define MOE4_W_OFF 16384                // after A's 16384 (gemm_l8_16_body's image): 4096 bytes of codes
#define MOE4_S_OFF 20480                // 256 scales, one dword each (see the header)
#define MOE4_STAGE_BYTES 21504
#define MOE4_LDS_BYTES (MOE4_STAGES * MOE4_STAGE_BYTES)

__device__ __forceinline__ int moe4_w_off(int row, int blk) {        // byte offset of the 16-B piece `blk` (32 codes) of W tile row `row`
    const int R = row >> 3;
    const int s = ((row & 7) << 1) | blk;
    return ((R << 4) + (s ^ (R & 1))) << 4;
}

// p: gemm_l8_16_body's arguments (p.W, p.col_scale unused); Q = the code rows [N, ldq bytes] of the tile's expert, S = their scale rows [N, lds]
template <bool SWIGLU>
__device__ __forceinline__ void gemm_l8_16_w4_body(const GemmArgs& p, const uint8_t* __restrict__ Q, int ldq, const uint8_t* __restrict__ S, int lds,
                                                   int bid, int nwg) {
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
    const auto rsS = __builtin_amdgcn_make_buffer_rsrc((void*)S, 0, 0x7fffffff, 0x00020000);
    unsigned a_vo[2], w_vo;                                     // 2 A pieces (piece i = +64 rows) + 1 W piece (waves 0..3: codes, 4..7: a scale byte)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int slot = ((i * 8 + wave) << 6) + lane;
        const int R = slot >> 4, sx = (slot & 15) ^ (R & 15);
        int am = m0 + 2 * R + (sx >> 3);
        am = am < p.M ? am : p.M - 1;
        a_vo[i] = ((unsigned)am * (unsigned)p.lda + (sx & 7) * 8) * 2;
    }
    const bool codes = wave < 4;                                // wave-uniform
    {
        const int slot = ((wave & 3) << 6) + lane;              // 0..255
        const int R = slot >> 4, sx = (slot & 15) ^ (R & 1);    // codes: bank row R holds tile rows 8 R .. 8 R + 7
        w_vo = codes ? (unsigned)(n0 + 8 * R + (sx >> 1)) * (unsigned)ldq + (sx & 1) * 16
                     : (unsigned)(n0 + (slot >> 1)) * (unsigned)lds + (slot & 1);
    }
    const int frow = lane & 15, fchk = lane >> 4;
    unsigned a_rd[2][2], b_rd[2][4], s_rd[4];                   // [k-step][block]; the scale of k-step kk is at s_rd + 4 kk
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int i = 0; i < 2; ++i) a_rd[kk][i] = gemm_lds_off(wm * 32 + i * 16 + frow, kk * 4 + fchk);
#pragma unroll
        for (int j = 0; j < 4; ++j) b_rd[kk][j] = MOE4_W_OFF + moe4_w_off(wn * 64 + j * 16 + frow, kk) + fchk * 4;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s_rd[j] = MOE4_S_OFF + (wn * 64 + j * 16 + frow) * 8;
    auto stage = [&](int kt, unsigned lds_buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(vl2_smem + lds_buf + ((i * 8 + wave) << 10)),
                                                     16, a_vo[i], (unsigned)kt * (GEMM_BK * 2), 0, 0);
        if (codes)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQ, (__attribute__((address_space(3))) void*)(vl2_smem + lds_buf + MOE4_W_OFF + (wave << 10)),
                                                     16, w_vo, (unsigned)kt * (GEMM_BK / 2), 0, 0);
        else
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsS, (__attribute__((address_space(3))) void*)(vl2_smem + lds_buf + MOE4_S_OFF + ((wave & 3) << 8)),
                                                     1, w_vo, (unsigned)kt * (GEMM_BK / 32), 0, 0);
    };
#pragma unroll
    for (int s = 0; s < MOE4_STAGES - 1; ++s)
        if (s < nt) stage(s, (unsigned)s * MOE4_STAGE_BYTES);
    unsigned cur = 0, fill = (MOE4_STAGES - 1) * MOE4_STAGE_BYTES;      // byte offsets of buffer kt % STAGES and (kt + STAGES - 1) % STAGES
    for (int kt = 0; kt < nt; ++kt) {
        const int newer = nt - 1 - kt < MOE4_STAGES - 2 ? nt - 1 - kt : MOE4_STAGES - 2;
        if (newer >= 5) VL2_WAIT_VMCNT(15); else if (newer == 4) VL2_WAIT_VMCNT(12); else if (newer == 3) VL2_WAIT_VMCNT(9);
        else if (newer == 2) VL2_WAIT_VMCNT(6); else if (newer == 1) VL2_WAIT_VMCNT(3); else VL2_WAIT_VMCNT(0);
        VL2_PHASE_BARRIER();                                        // everyone's pieces of tile kt landed; the buffer read in kt - 1 is free
        if (kt + MOE4_STAGES - 1 < nt) stage(kt + MOE4_STAGES - 1, fill);
        const unsigned lds_buf = cur;
        cur = cur + MOE4_STAGE_BYTES == MOE4_LDS_BYTES ? 0u : cur + MOE4_STAGE_BYTES;
        fill = fill + MOE4_STAGE_BYTES == MOE4_LDS_BYTES ? 0u : fill + MOE4_STAGE_BYTES;
        if (!live) continue;                                        // (see `live` above: loads and barriers only)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 fa[2], fb[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *(const bf16x8*)(vl2_smem + lds_buf + a_rd[kk][i]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                fb[j] = __builtin_bit_cast(bf16x8, mx4_cvt8(*(const uint32_t*)(vl2_smem + lds_buf + b_rd[kk][j]),
                                                            mx4_scale(*(const uint8_t*)(vl2_smem + lds_buf + s_rd[j] + kk * 4))));
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

// The grouped form: moe_gemm8_kernel's dispatch on the MXFP4 stacks.  g = the call's GemmArgs over the whole permuted row space (A, C,
// row_norm; W, col_scale unused); q = expert 0's code rows [N, ldq bytes], q_stride bytes between two experts; scale = expert 0's E8M0 rows
// [N, lds bytes], s_stride bytes apart.
struct MoeGemm4Args {
    GemmArgs g;
    const int* offs;          // [E + 1]
    const int* counts;        // [E]
    const uint8_t* q;
    const uint8_t* scale;
    long long q_stride, s_stride;
    int ldq, lds, E, rt_cap;
};

template <bool SWIGLU>
__global__ __launch_bounds__(512, 1) void moe_gemm4_kernel(MoeGemm4Args a) {
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
    p.tiles_m = 1; p.tiles_n = 1;
    gemm_l8_16_w4_body<SWIGLU>(p, a.q + (size_t)e * a.q_stride + (size_t)tn * GEMM_BN * a.ldq, a.ldq,
                               a.scale + (size_t)e * a.s_stride + (size_t)tn * GEMM_BN * a.lds, a.lds, 0, 1);
}
