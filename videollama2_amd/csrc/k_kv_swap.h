// Swapping pages of the paged KV cache between a pool and a packed device arena (vl2_kv_pages_move): the only data path
// of a preemption.  A page is opaque here -- page_bytes bytes, a multiple of 16 -- so ONE body serves every pool kind of sections 19 and 21:
//   16-bit rows   [n_pages][nkv][64][128] x 2 bytes,   e4m3 codes [n_pages][nkv][64][128] x 1 byte,   fp32 row scales [n_pages][nkv][64] x 4 bytes.
//   pool     : [n_pages][page_bytes]            arena : [n][page_bytes] (device memory; the host leg is a copy_ on the same stream)
//   page_ids : device int32 [n]; slot i of the arena pairs with pool page page_ids[i]
//   to_arena : != 0 gather (pool page -> arena slot i), 0 scatter (arena slot i -> pool page)
// An id outside [1, n_pages) is skipped: page 0 is the parking page and is never moved; the slot or page of a skipped id is left untouched.
// Nothing but the n arena slots (gather) or the named pages (scatter) is written.
#pragma once
#include "dev_common.h"

constexpr int KV_MOVE_UNROLL = 4;                          // 16-byte vectors in flight per lane: 4 loads are issued before the first store

// grid = (gx, n), block 256: blockIdx.y = arena slot (its page id is one uniform load per workgroup), the gx workgroups of a slot stride over
// the page's vpp = page_bytes / 16 vectors, KV_MOVE_UNROLL * 256 at a time.  The host sizes gx so that gx * n stays near 2048 workgroups.
__global__ __launch_bounds__(256) void kv_pages_move_kernel(u32x4* __restrict__ pool, u32x4* __restrict__ arena,
                                                            const int* __restrict__ page_ids, int n_pages, long vpp, int to_arena) {
    const int slot = blockIdx.y;
    const int page = page_ids[slot];
    if (page < 1 || page >= n_pages) return;
    u32x4* in_pool = pool + (size_t)page * vpp;
    u32x4* in_arena = arena + (size_t)slot * vpp;
    const u32x4* src = to_arena ? in_pool : in_arena;
    u32x4* dst = to_arena ? in_arena : in_pool;
    const long step = (long)gridDim.x * (KV_MOVE_UNROLL * 256);
    for (long v0 = (long)blockIdx.x * (KV_MOVE_UNROLL * 256) + threadIdx.x; v0 < vpp; v0 += step) {
        u32x4 w[KV_MOVE_UNROLL];
#pragma unroll
        for (int j = 0; j < KV_MOVE_UNROLL; ++j)
            if (v0 + j * 256 < vpp) w[j] = src[v0 + j * 256];
#pragma unroll
        for (int j = 0; j < KV_MOVE_UNROLL; ++j)
            if (v0 + j * 256 < vpp) dst[v0 + j * 256] = w[j];
    }
}
