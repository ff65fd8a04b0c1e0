// The launch plan of the skinny-M GEMMs (k_skinny.h), shared by every weight format's entry point (vl2_abi.hip) and by the CPU emulator
// build of the tests.  Plain host C++: no HIP types.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct SkinnyPlan {
    int mt, Mp;             // 16-row MFMA tiles of x (1, 2 or 4), padded rows = 16 * mt
    int ks, kslice;         // K split (gridDim.y) and K per workgroup
    int kchunk;             // K per LDS chunk: the largest 32-multiple divisor of the slice whose x chunk fits lds_cap
    size_t lds;             // dynamic LDS bytes = Mp * (kchunk + 8) * 2
    int64_t ws_need;        // bytes of fp32 partials: ks * Mp * N * 4
};
enum { SKINNY_PLAN_OK = 0, SKINNY_PLAN_WS_SMALL = 1, SKINNY_PLAN_NO_CHUNK = 2 };

// M <= 64, N % 64 == 0, K % 32 == 0 (the callers check).  K split: enough (column group, K slice) waves to keep ~4096 in flight, a divisor
// of the 32-deep steps -- a function of N and K only, so a row's bits do not depend on the other rows of the batch.  shrink_to_ws (the
// 16-bit entry alone): a split whose partials exceed the workspace is made smaller until they fit; otherwise a workspace that is too
// small is an error, and the plan never depends on it.
static inline int skinny_plan(int M, int N, int K, int64_t ws_bytes, bool shrink_to_ws, SkinnyPlan& p, size_t lds_cap = 65536) {
    p.mt = M <= 16 ? 1 : M <= 32 ? 2 : 4;
    p.Mp = 16 * p.mt;
    const int steps = K / 32;
    int ks = (4096 + N / 16 - 1) / (N / 16);
    ks = ks < 1 ? 1 : ks > 32 ? 32 : ks;
    while (ks > 1 && (steps % ks || (shrink_to_ws && (int64_t)ks * p.Mp * N * 4 > ws_bytes))) --ks;
    p.ks = ks;
    p.ws_need = (int64_t)ks * p.Mp * N * 4;
    if (p.ws_need > ws_bytes) return SKINNY_PLAN_WS_SMALL;
    p.kslice = K / ks;
    int kchunk = p.kslice;
    while (kchunk > 32 && (p.kslice % kchunk || kchunk % 32 || (size_t)p.Mp * (kchunk + 8) * 2 > lds_cap)) kchunk -= 32;
    p.kchunk = kchunk;
    p.lds = (size_t)p.Mp * (kchunk + 8) * 2;
    if (p.kslice % kchunk || p.lds > lds_cap) return SKINNY_PLAN_NO_CHUNK;
    return SKINNY_PLAN_OK;
}
