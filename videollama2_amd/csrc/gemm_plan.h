// The launch plan of vl2_gemm (vl2_abi.hip): which kernel form of the GEMM family (k_gemm.h, k_gemm6/7/8/9.h) a call gets, on which rows, with which
// tile counts and template switches.  Plain host C++: no HIP types -- the ABI turns a planned launch into its instantiation (launch_planned), and a CPU
// test holds the plan against a recorded table (tests/test_gemm_plan_host.py).  Every form of the 32 x 32 x 16 family produces the same bits, so a slip
// here changes speed only: that table is what pins the choice.
#pragma once
#include <assert.h>
#include <stdint.h>

#define SK_GRID 512                  // persistent stream-K workgroups: 2 per CU
#define SPLITK_MAX_WG 1024           // split-K: at most this many (tile, split) workgroups -> 64 MiB of fp32 partials
#define SPLITK_MAX_TILES 192         // split-K only when the plain grid leaves most of the 512 resident slots empty

// kernel forms; the tile is tile_h x tile_w of the launch
enum GemmForm {
    GF_128 = 0,          // gemm_bf16_kernel: 128 x 128, two barriers per K-tile
    GF_128_SPLITK,       //   ... K split over gridDim.y through the workspace
    GF_128_STREAMK,      //   ... (lab) persistent stream-K, gemm_sk_bf16_kernel
    GF_64,               // gemm_s_bf16_kernel: 64 x 64 small-M form
    GF_L8,               // gemm_l8_bf16_kernel: one-round 8-wave 128 x 128
    GF_128x256,          // gemm3_bf16_kernel: 128 x 256 ping-pong
    GF_G4_256,           // gemm4_bf16_kernel on 256-row tiles
    GF_G4_192,           //   ... 192-row tiles
    GF_G4_160,           //   ... (lab) 160-row tiles
    GF_GEMM6,            // gemm6_bf16_kernel: persistent ping-pong, tile_h 256 / 192
    GF_GEMM7,            // gemm7_bf16_kernel: fill-the-round tiles, tile_h 224 / 192 x 128
    GF_GEMM8,            // (lab) gemm8_bf16_kernel: 256 x 256 on four waves
    GF_GEMM9,            // gemm9_bf16_kernel: 256 x 256 on the 16 x 16 x 32 instruction, `mode` = its MODE
    GF_MIX,              // gemm_mix_bf16_kernel: 256-row tiles of [m0, m0 + rows) + 8-wave 128 x 128 tiles of the tail rows in one launch
    GF_MIX16,            // gemm_mix16_bf16_kernel: the same on the 16 x 16 x 32 instruction, `mode` 0 / 9
    GF_L8_16,            // gemm_l8_16_bf16_kernel: one-round 128 x 128 of the 16 x 16 x 32 set
    GF_GEMM7_16,         // (lab) gemm7_16_bf16_kernel: fill-the-round tiles of the 16 x 16 x 32 set
    GF_REMAP,            // gemm_bf16_kernel, row-remap instance (patch embed)
    GF_FP8_128x256,      // gemm3_fp8_kernel
    GF_FP8_256,          // gemm4_fp8_kernel on 256-row tiles
    GF_FP8_192,          //   ... 192-row tiles
    GF_COUNT
};
static const char* const kGemmFormName[] = {"GF_128", "GF_128_SPLITK", "GF_128_STREAMK", "GF_64", "GF_L8", "GF_128x256", "GF_G4_256", "GF_G4_192", "GF_G4_160", "GF_GEMM6",
    "GF_GEMM7", "GF_GEMM8", "GF_GEMM9", "GF_MIX", "GF_MIX16", "GF_L8_16", "GF_GEMM7_16", "GF_REMAP", "GF_FP8_128x256", "GF_FP8_256", "GF_FP8_192"};
static_assert(sizeof(kGemmFormName) / sizeof(kGemmFormName[0]) == GF_COUNT, "one name per kernel form");

// everything the decision reads
struct GemmPlanIn {
    int M, N, K;                     // of this chunk; fp8: K counts e4m3fn elements (bytes)
    bool act;                        // an activation in the epilogue (which one does not matter here)
    bool swiglu, f32, gather, remap, fp8;
    bool res, stats_out, norm, row_norm, row_norm_out, tile_ctr, ws;      // optional operands present (tile_ctr: the descriptor's or the workspace's)
    int64_t ws_bytes;
    int variant;
    bool splitk, persist, no_mix, no_fill, weave, weave4, no_weave4;     // the descriptor's bits as given
    bool mfma16;                     // DECIDED: want_mfma16() of the whole call's bits (a column chunk does not decide again)
    int cus;                         // compute units of the device (read only where the persistent form is a candidate)
    bool lab;                        // the build carries the lab forms (-DVL2_LAB)
};

struct GemmLaunch {
    int form;                        // GemmForm
    int tile_h, tile_w;
    int m0, rows;                    // rows [m0, m0 + rows) of the chunk
    int tiles_m, tiles_n;            // GemmArgs::tiles_m / tiles_n of the launch
    int grid_x, grid_y;
    bool tr;                         // C^T epilogue (gemm_store_tr)
    bool woven;                      // LDS-DMA issue woven into the matrix phases
    int mode;                        // gemm9 / mix16 MODE
    bool acc2;                       // gemm6: two accumulator sets
    int split;                       // split-K factor (1 = none)
    int dyn;                         // gemm6 tile hand-out: 0 static walk (tile_ctr unwired), 1 through the counter block, 2 the first tile of a workgroup too
    int tile_group;                  // GemmArgs::tile_group
    bool ws_wired;                   // sk_ws (and the form's flags / counters) point into the workspace
    bool needs_finalize;             // row_norm_out is wanted and this kernel has no producer-side finalize (gemm_rows_ticket): vl2_gemm appends row_norm_finalize
    int tail_rows, tail_tiles_m, tail_tiles_n, tail_tile_group;      // mixed forms: rows [m0 + rows, m0 + rows + tail_rows) as the launch's second part
};

// One launch, or two for a row split sent as two launches: the tail of a split is never split again (case (1) of m_split_rows leaves at most 96 rows,
// case (2) less than one round of row tiles, and either needs 1024).
#define GEMM_PLAN_MAX 2
struct GemmPlan {
    int n;
    GemmLaunch l[GEMM_PLAN_MAX];
};

static inline int gemm_t128(const GemmPlanIn& a) { return ((a.M + 127) / 128) * (a.N / 128); }      // the 128 x 128 grid (int, as GemmArgs' tile counts)

// stream-K form: measured 0.5-0.6x of the plain grid on this workload's shapes (per-tile prologue/epilogue of the persistent
// workgroups, ~15 us of partial-tile exchange, worse L2 locality of strided tile ownership) -> only on explicit request.
static inline bool want_stream_k(const GemmPlanIn& a) { return a.ws && a.variant == 2 && !a.norm && !a.stats_out; }

// Tile-shape choice (auto): expected efficiency = how full the last round of resident workgroups is x rows wasted by the
// M edge x the kernel's measured rate on well-quantised shapes (128x128 two-barrier kernel 1.0, 128x256 ping-pong 1.07,
// 256x256 ping-pong 1.2: profiles/r01_gemm_experiments.md).  Fitted to the measured shapes of the T=16 workload: the LLM
// o/gate-up/down projections and the STC 4096x4096 convs take 128x256, ViT qkv/wo/fc2 and the LLM qkv take 256x256,
// short-K GEMMs (STC b1) stay on 128x128.  Returns 1, 4 (gemm3), 8 (gemm4) or 12 (gemm4 on 192-row tiles).
static inline int choose_gemm_kernel(const GemmPlanIn& a, double* eff = nullptr) {
    if (eff) *eff = 0.0;
    if (a.N % 256) return 1;
    // at most one 128x128 tile per CU: a bigger tile only halves the CUs in use and doubles the latency of the single round
    // (measured, T=8: 845x4096x4096 44.6 us here vs 50.2 us on 128x256; 945x4096x4096 47.2 vs 51.2)
    if ((long)((a.M + 127) / 128) * (a.N / 128) <= 256) return 1;
    const auto fill = [](double rounds) { return rounds / (double)(long)(rounds + 0.999999); };
    const double m128 = (double)a.M / (((a.M + 127) / 128) * 128.0), m256 = (double)a.M / (((a.M + 255) / 256) * 256.0);
    const double e1 = fill((double)((a.M + 127) / 128) * (a.N / 128) / 512.0) * m128;           // 2 WG/CU
    const double e3 = fill((double)((a.M + 127) / 128) * (a.N / 256) / 256.0) * m128 * 1.07;    // 1 WG/CU
    const double e4 = fill((double)((a.M + 255) / 256) * (a.N / 256) / 256.0) * m256 * 1.2;     // 1 WG/CU
    int best = 1;
    double eb = 1.03 * e1;
    if (a.K >= 2048 && e3 > eb) { best = 4; eb = e3; }
    if (a.K >= 512 && e4 > eb) { best = 8; eb = e4; }
    // the 256x256 kernel on 192-row tiles (variant 12): the same rate per FLOP over whole rounds (sq 4096^3: 85 us per round of 192-row
    // tiles against 117), a little less in practice (fc1 at 3.06 rounds 105.9 us vs 95.4 on 256 rows) -> 1.13.  Takes the shapes whose
    // 256-row grid leaves a round badly filled: ViT out_proj / fc2 at 16 frames (148 -> 196 tiles: 30.7 -> 28.9 us, 84.6 -> 81.3), the
    // LLM q/k/v at S = 1621 (168 -> 216 tiles: 84.0 -> 81.2), the STC K = 1024 conv (576 = 2.25 rounds -> 768 = 3.0: 87.6 -> 82.2).
    // scripts/ubench/gemm_lab.hip (bit-identical, hash-checked) and scripts/kernel_bench.py, profiles/r03_gemm_lab_t192.txt
    const double m192 = (double)a.M / (((a.M + 191) / 192) * 192.0);
    const double e5 = fill((double)((a.M + 191) / 192) * (a.N / 256) / 256.0) * m192 * 1.13;
    if (a.K >= 512 && e5 > eb * 1.02) { best = 12; eb = e5; }
    // ... and on 160-row tiles (variant 10, round 6: the 192-row tile without group 1's third row block): ONE-round grids only, where a finer tile
    // shortens the single round -- ViT out_proj / fc2 at 16 frames: 196 tiles of 192 rows (77 % of the CUs) -> 232 tiles of 160 rows (91 %).  Rate 1.08:
    // a SIMD issues 20 MFMAs per slab behind the same load phases (24 on 192 rows).
    // MEASURED AND NOT TAKEN (profiles/r06_tile160_bench.txt, interleaved on one box): fc2 9232 x 1024 x 4096 79.2 us on 192 rows, 82.7 on 160; out_proj 30.4 vs
    // 30.9; 18464 rows: 163.5 vs 166.5.  A one-round grid at 77 % of the CUs is NOT 77 % of the chip: the part runs at its power limit, and 196 workgroups at a
    // higher clock do what 232 do at a lower one -- filling the round buys nothing where watts, not CUs, are the budget.  The tile stays a lab form (variant 10).
    if (eff) *eff = best == 1 ? e1 : eb;
    return best;
}

// gemm7 (k_gemm7.h): 224 x 128 / 192 x 128 tiles for GEMMs that are ONE round of workgroups whatever the tile -- 0 = not this call, else R1
// (3 = 224 rows, 2 = 192 rows).  Same efficiency model as choose_gemm_kernel: fill of the last round x rows wasted at the M edge x the
// kernel's rate relative to the 128x128 kernel (GEMM7_RATE, measured: profiles/r05_experiments.md).  Only where the 128x128 grid is
// more than one tile per CU (below that the one-round 128x128 / 64x64 kernels own the shape) and the K loop is long enough to pay for
// the image epilogue.
#define GEMM7_RATE 0.88
static inline int choose_gemm7(const GemmPlanIn& a, bool gather) {
    if (a.N % 128 || a.K < 1024 || a.remap) return 0;
    const long t128 = (long)((a.M + 127) / 128) * (a.N / 128);
    if (t128 <= 256) return 0;
    const auto fill = [](double rounds) { return rounds / (double)(long)(rounds + 0.999999); };
    double eb = 0.0;
    if (gather) eb = fill((double)t128 / 512.0) * ((double)a.M / (((a.M + 127) / 128) * 128.0));     // the gathered form has the 128x128 kernel only
    else choose_gemm_kernel(a, &eb);
    int best = 0;
    for (int r1 = 3; r1 >= 2; --r1) {
        const int bm = 128 + 32 * r1;
        const long t7 = (long)((a.M + bm - 1) / bm) * (a.N / 128);
        if (t7 > 256) continue;                                          // one round only: beyond it the 256-row kernels' rate wins
        const double e7 = fill((double)t7 / 256.0) * ((double)a.M / (((a.M + bm - 1) / bm) * (double)bm)) * GEMM7_RATE;
        if (e7 > eb * 1.03) { best = r1; eb = e7; }
    }
    return best;
}

// Split-K factor for the 128x128 kernel (1 = do not split).  Only for grids that leave most resident slots empty: a lone
// workgroup streams its K-tiles at ~0.64 us each (0.95 us when two share a CU), so a 96-tile grid with K = 4096 takes 42 us
// however idle the chip is (scripts/kernel_bench.py --small).  Cost model in us per launch, d over the divisors of the
// K-tile count: (K-tiles / d) x per-tile time at the resulting occupancy + partial write/reduce.
static inline int choose_splitk(const GemmPlanIn& a) {
    if (!a.ws || !a.splitk || (a.variant != 0 && a.variant != 1)) return 1;
    const int tiles = gemm_t128(a), nt = a.K / 64;
    if (tiles > SPLITK_MAX_TILES || nt < 32) return 1;       // measured: K = 1024 GEMMs lose (14.0 -> 19.7 us)
    int best = 1;
    double cb = 1e30;
    for (int d = 1; d <= 32 && d * tiles <= SPLITK_MAX_WG; ++d) {
        if (nt % d || nt / d < 4) continue;
        const int wg = tiles * d;
        const double per = wg <= 256 ? 0.64 : 0.95 * ((wg + 511) / 512);
        const double cst = (nt / d) * per + (d > 1 ? 2.0 + 0.3 * d : 0.0);
        if (cst < cb * (d > 1 ? 0.85 : 1.0)) { cb = cst; best = d; }
    }
    return best;
}

// Small-M form (64x64 tiles, gemm_s_bf16_kernel): when the 128x128 grid cannot even give every CU one tile, quartering the
// tile spreads the operand stream over the idle CUs (a workgroup streams at ~55 GB/s whatever the chip does).  Same K order
// as every other kernel -> same bits.  Measured crossover (scripts/kernel_bench.py --small): see profiles/.
static inline bool want_small_m(const GemmPlanIn& a) {
    if (a.variant == 32) return true;
    if (a.variant != 0) return false;
    return gemm_t128(a) <= 128 && a.K >= 512;   // measured crossover: wins at <= 128 tiles, loses at 152-160
}

// Epilogue form of the two ping-pong kernels (k_gemm.h gemm_store_tr): bf16 outputs WITHOUT a residual go through the
// register-resident C^T epilogue (measured on MI355X, scripts/ubench/gemm_lab.hip: fc1 + QuickGELU 101.8 -> 95.6 us, gate/up
// 393 -> 384 us, STC 1x1 convs -1.5..-4 %), outputs with a residual keep the LDS-transposing one (the residual's row-contiguous
// 16-B loads, all requested up front, beat the 8-B pieces the C^T layout needs: 31.2 vs 35.8 us on the ViT out_proj).  Both forms
// produce the same bits (hash-checked per shape), so the choice is invisible to every caller.  (The fp32 outputs have the LDS epilogue only.)
static inline bool want_tr_epilogue(const GemmPlanIn& a) { return !a.f32 && !a.res; }

// ---- persistent ping-pong GEMM (k_gemm6.h): ONE workgroup per CU walks its tiles, the LDS ring runs across tile boundaries, the stores
// of a tile are never waited for, the epilogue vectors arrive by LDS-DMA.  For bf16 outputs without residual / statistics / gather / remap
// whose 256-row grid is more than one round of workgroups (a one-round grid has nothing to overlap).  Measured in the C++ lab on one box,
// interleaved with the one-tile-per-workgroup kernels and bit-identical to them (profiles/r04_gemm_lab_persistent.txt): ViT q/k/v
// 9232x3072x1024 65.8 -> 59.6 us, ViT fc1 + QuickGELU 94.5 -> 87.3 (101.8 -> 89.9 with the LayerNorm carried), STC K = 1024 conv
// 81.8 -> 75.8, STC 4096x4096 conv 258.8 -> 254.0, 8192x4096x4096 216.2 -> 212.3 (1295 TF/s).
static inline bool gemm6_ok(const GemmPlanIn& a, int bm) {
    return !a.res && !a.stats_out && !a.gather && !a.remap && (!a.norm || a.row_norm) && a.N % 256 == 0 && a.K % 32 == 0 && a.K >= 1024 && a.M >= bm;
}
// 0 = not this call; 70 = 256-row tiles, 71 = 192-row tiles: the smaller makespan in units of a 256-row tile (a 192-row tile costs 0.75)
static inline int choose_gemm6(const GemmPlanIn& a) {
    // only with a counter block (dynamic tile hand-out): the static walk is as slow as its slowest CU (k_gemm6.h)
    if (!gemm6_ok(a, 256) || !a.tile_ctr) return 0;
    const int cus = a.cus;
    const long t256 = (long)((a.M + 255) / 256) * (a.N / 256), t192 = (long)((a.M + 191) / 192) * (a.N / 256);
    if (t256 <= cus) return 0;
    const double ms256 = (double)((t256 + cus - 1) / cus), ms192 = 0.75 * (double)((t192 + cus - 1) / cus);
    return ms192 < ms256 ? 71 : 70;
}

// The persistent form on request: 60 / 61 / 62 static tile walk (256- / 192-row tiles / 192 rows + two accumulator sets, measured slower, kept for the
// lab), 70 / 71 = 60 / 61 through the counter block, 80 / 81: the first tile of a workgroup from the counter too.  0 = not asked for, or the call does not qualify.
static inline int forced_gemm6(const GemmPlanIn& a) {
    const int v = a.variant;
    return (v == 60 || v == 61 || v == 62 || ((v == 70 || v == 71 || v == 80 || v == 81) && a.tile_ctr)) &&
           gemm6_ok(a, v == 60 || v == 70 || v == 80 ? 256 : 192) && (v != 62 || a.K >= 32 * 28) ? v : 0;
}

// Row split (returns the number of leading rows that go to the 256x256 kernel, 0 = no split).  Two cases, both two launches on the
// same stream; every kernel accumulates K in the same order and shares one epilogue, so the output bits do not change (asserted
// in tests/test_gpu_ops.py):
//  (1) M = 1621 leaves the 256-row kernel a 7th row tile with 85 live rows (9.5 % of its MFMA work wasted) and the 128-row kernel
//      is slower per FLOP.  When N is wide enough for both parts to fill the chip, the first floor(M/256)*256 rows go to the
//      256x256 kernel and the remaining rows to whatever the chooser picks for them.  Measured: 1621x28672x4096 + SwiGLU
//      362 -> 345 us; loses on N <= 6144 and on M % 256 > 128.
//  (2) whole rounds + a short tail: 9216x4096x4096 (the STC s1 convolutions) is 576 tiles = 2.25 rounds of 256 workgroups; the
//      quarter round costs most of a full one.  The rows of the whole rounds stay on the 256x256 kernel, the tail rows (at most
//      half a round of big tiles) go through the chooser, which gives them a finer-tiled one-round kernel
//      (2 rounds 224 us + 1024 rows on the 8-wave 128x128 kernel ~40 us against 287 us for the single launch).
static inline int m_split_rows(const GemmPlanIn& a, int variant) {
    if (variant != 0 || a.remap || a.N % 256 || a.K < 1024 || a.M < 1024) return 0;
    const int r = a.M % 256, m1_tiles = a.M / 256, n_tiles = a.N / 256;
    if (r != 0 && r <= 96 && n_tiles >= 64) {
        const long t4 = (long)m1_tiles * n_tiles;
        if ((double)t4 / (double)(((t4 + 255) / 256) * 256) >= 0.85) return m1_tiles * 256;   // the 256-row part fills its rounds
    }
    if (256 % n_tiles == 0) {
        const int per_round = 256 / n_tiles;                       // row tiles in one full round of 256 workgroups
        const int mt = (a.M + 255) / 256, rounds = mt / per_round, tail = mt - rounds * per_round;
        if (rounds >= 1 && tail > 0 && tail * n_tiles <= 128) return rounds * per_round * 256;
    }
    return 0;
}

// The 16 x 16 x 32 kernels (k_gemm9.h; other bits than the family's): built for plain rows, bf16 output, no activation, no statistics out of a
// SwiGLU call.  The flag is a wish (ignored where the kernel is not built), variants 16 ... 23 / 25 ... 29 a demand (vl2_gemm refuses them when this is false).
static inline bool gemm_ok16(const GemmPlanIn& a) { return !a.gather && !a.f32 && !a.remap && !a.act && a.N % 256 == 0 && !(a.stats_out && a.swiglu); }
static inline bool gemm_v16(int v) { return (v >= 16 && v <= 23) || (v >= 25 && v <= 29); }      // 17 ... 23, 25, 27 ... 29: lab forms
static inline bool want_mfma16(const GemmPlanIn& a, bool flag) {      // flag: VL2_GEMM_MFMA16; a: the whole call
    const int v = a.variant;
    return gemm_ok16(a) && (gemm_v16(v) || ((v == 0 || ((v == 256 || v == 224 || v == 192) && !a.swiglu)) && flag));
}

// a launch of `form` on rows [m0, m0 + a.M) with th x tw tiles, one workgroup per tile
static inline GemmLaunch gemm_launch(const GemmPlanIn& a, int m0, int form, int th, int tw) {
    GemmLaunch l{};
    l.form = form; l.tile_h = th; l.tile_w = tw;
    l.m0 = m0; l.rows = a.M;
    l.tiles_m = (a.M + th - 1) / th; l.tiles_n = a.N / tw;
    l.grid_x = l.tiles_m * l.tiles_n; l.grid_y = 1;
    l.split = 1;
    return l;
}
// the 256 x 256 ping-pong kernel on bm-row tiles.  The product builds ONE issue order per tile height: woven (WEAVE4) on the 192-row tiles, load-phase
// on the 256-row tiles; the other order of each is a lab form (VL2_GEMM_NO_WEAVE4 / VL2_GEMM_WEAVE4) -- in the product the two bits are accepted and ignored
static inline GemmLaunch gemm4_launch(const GemmPlanIn& a, int m0, int bm, bool weave4) {
    GemmLaunch l = gemm_launch(a, m0, bm == 256 ? GF_G4_256 : bm == 192 ? GF_G4_192 : GF_G4_160, bm, 256);
    if (bm == 160) return l;                       // one form: LDS epilogue, load-phase issue
    l.tr = want_tr_epilogue(a);
    l.woven = !a.f32 && (a.lab ? weave4 : bm == 192);
    return l;
}
// the ONE mixed launch of a row split: whole 256-row tiles of the first M1 rows + 128 x 128 tiles of the tail rows, when the tail is 129..512 tiles
static inline bool gemm_mix_launch(const GemmPlanIn& a, int m0, int M1, int form, GemmLaunch& l) {
    const long t_big = (long)(M1 / 256) * (a.N / 256), t_tail = (long)((a.M - M1 + 127) / 128) * (a.N / 128);
    if (!(t_tail > 128 && t_tail <= 512)) return false;
    l = gemm_launch(a, m0, form, 256, 256);
    l.rows = M1; l.tiles_m = M1 / 256;
    l.tail_rows = a.M - M1; l.tail_tiles_m = (a.M - M1 + 127) / 128; l.tail_tiles_n = a.N / 128;
    l.grid_x = (int)(t_big + t_tail);
    return true;
}

// rows [m0, m0 + a.M) of a chunk; no_persist: the automatic choice without the persistent form (variant 24)
static inline void gemm_plan_rows(const GemmPlanIn& a, bool no_persist, int m0, GemmPlan& p) {
    assert(p.n < GEMM_PLAN_MAX);
    GemmLaunch& l = p.l[p.n++];
    const int v = a.variant;
    if (a.mfma16) {                                         // (plain rows, bf16 output, no activation: gemm_ok16)
        if (v == 23 || v == 25) {                         // the stamps need room for 8 waves x 6 u64 per workgroup
            l = gemm_launch(a, m0, GF_GEMM9, 256, 256);
            l.mode = v == 23 ? 7 : 8;
            l.ws_wired = a.ws && a.ws_bytes >= (int64_t)l.grid_x * 8 * 6 * 8;
            return;
        }
        // a row-split call keeps its ONE mixed launch (k_gemm9.h gemm_mix16_bf16_kernel): whole 256-row tiles on gemm9_body, the tail rows on the
        // 128 x 128 body of the same instruction -- the same bits row by row, so the split stays invisible (as in the 32 x 32 x 16 family)
        if (v == 0 || v == 16 || v == 26 || (a.lab && v >= 27 && v <= 29)) {
            if (const int M1 = m_split_rows(a, 0); M1 > 0 && !a.no_mix && gemm_mix_launch(a, m0, M1, GF_MIX16, l)) {
                if (a.lab && v >= 27) l.tile_group = v == 27 ? 8 : v == 28 ? 0 : 6;      // lab: variant 26 with another group depth
                if (a.lab && v == 28) l.tail_tile_group = -1;                            // lab: variant 26 with the tail's empty waves computing (as before round 6's skip)
                // the big tiles with 64-deep phases on the 5-stage ring (the whole 160 KiB of LDS): the flag's form and variant 26 (gate/up at
                // S = 945 / 1621 / 2973: 195.9 / 334.8 / 609.5 -> 192.4 / 332.2 / 596.9 us, profiles/r06_mix16_bench_64deep.txt); 16 = the 32-deep form
                // (SwiGLU calls only: without SwiGLU the tail body ends in gemm_rows_ticket, whose LDS word does not fit beside the 160-KiB ring)
                l.mode = a.swiglu && v != 16 ? 9 : 0;
                return;
            }
        }
        if (!a.swiglu) {
            // the other two tiles of the 16 x 16 x 32 set (round 6: the decoder's o / down projections): at most one 128 x 128 tile per CU -> the one-round
            // 128 x 128 body; a one-round grid of fill-the-round tiles where the family's rule picks them -> gemm7 on this instruction; else the 256 x 256 tile
            if (v == 0 || v == 256 || v == 224 || v == 192) {       // (256 / 224 / 192 with the flag: that tile of the set on demand)
                if (v == 256 || (v == 0 && (long)gemm_t128(a) <= 256)) { l = gemm_launch(a, m0, GF_L8_16, 128, 128); return; }
                // (lab: the fill-the-round tiles on this instruction, k_gemm7.h gemm7_loop16 -- bit-identical with the rest of the set, measured at parity
                //  with their 32 x 32 x 16 twins on the one-round grids they exist for: no call site uses them)
                if (const int r1 = !a.lab ? 0 : v == 224 ? 3 : v == 192 ? 2 : a.no_fill ? 0 : choose_gemm7(a, false); r1 != 0) {
                    l = gemm_launch(a, m0, GF_GEMM7_16, 128 + 32 * r1, 128);
                    return;
                }
            }
        }
        // only the shipped form (MODE 0) finalizes its rows itself.  QUIRK kept: 224 / 192 + MFMA16 fall through to MODE 0 in the product and finalize twice
        const bool fin = v != 0 && v != 16 && a.row_norm_out;
        l = gemm_launch(a, m0, GF_GEMM9, 256, 256);
        l.mode = v == 26 ? 9 : (a.lab && v >= 17 && v <= 23) ? v - 16 : 0;      // lab: variants 17 ... 23 = MODE 1 ... 7 (k_gemm9.h)
        l.needs_finalize = fin;
        return;
    }
    if (!a.swiglu) {
        // fill-the-round tiles (k_gemm7.h): variants 224 / 192 on request (any shape with N % 128 == 0), or by the rule of choose_gemm7
        const int r1 = v == 224 ? 3 : v == 192 ? 2 : (v == 0 && !a.no_fill) ? choose_gemm7(a, a.gather) : 0;
        // (225 / 193 = 224 / 192 with the LDS-DMA issue woven into the MFMA phases, as VL2_GEMM_WEAVE selects it: lab form, see gemm3 below;
        //  in the product VL2_GEMM_WEAVE is accepted and ignored)
        const int r1v = v == 225 ? 3 : v == 193 ? 2 : r1;
        if (r1v) {
            l = gemm_launch(a, m0, GF_GEMM7, 128 + 32 * r1v, 128);
            l.woven = a.lab && (a.weave || v == 225 || v == 193);
            return;
        }
    }
    if (!a.gather && !a.f32) {
        // persistent form: on request (forced_gemm6) or by the rule of choose_gemm6
        const int k6 = v == 0 ? (a.persist && !no_persist ? choose_gemm6(a) : 0) : forced_gemm6(a);
        if (k6) {
            l = gemm_launch(a, m0, GF_GEMM6, k6 % 10 == 0 ? 256 : 192, 256);
            l.dyn = k6 >= 80 ? 2 : k6 >= 70 ? 1 : 0;
            l.acc2 = k6 == 62;
            if (l.grid_x > a.cus) l.grid_x = a.cus;                        // one workgroup per CU
            return;
        }
        // (K < 2048 with an activation in the epilogue -- ViT fc1 + QuickGELU -- stays on its single launch: in the pipeline's rocprofv3 trace the
        //  mixed form took 105 us against 98.6 for the 128x128 kernel, although it wins the isolated micro-benchmark; end to end the two are equal:
        //  encode 12.52 vs 12.52 ms over three alternations)
        if (const int M1 = (a.K < 2048 && a.act) ? 0 : m_split_rows(a, v); M1 > 0) {
            // ONE launch (k_gemm.h gemm_mix_bf16_kernel) when the tail is 129..512 tiles of the 8-wave 128x128 body: its workgroups start on
            // the CUs that run out of big tiles instead of behind a second launch.  Measured against the two launches on one box
            // (scripts/gpu_r3_k.sh): gate/up at S = 1621 383.0 -> 369.7 us (prefill 26.0 -> 25.6 ms), STC 4096x4096 conv 274.7 -> 265.0,
            // STC K = 1024 conv 85.9 -> 82.2, ViT fc1 99.2 -> 96.5 (T = 8: 54.7 -> 49.9); in the pipeline the K = 1024 cases are neutral at T = 16
            // (encode 12.90 vs 12.89 ms) and the prefill gains 0.4 ms.  VL2_GEMM_NO_MIX in the descriptor keeps two launches / the single kernel.
            if (!a.no_mix && gemm_mix_launch(a, m0, M1, GF_MIX, l)) {
                l.tr = want_tr_epilogue(a);
                l.woven = a.lab && a.weave4;          // lab: the big tiles with the woven LDS-DMA issue (VL2_GEMM_WEAVE4)
                return;
            }
            if (a.K >= 2048) {                       // two launches (measured wins at K >= 2048 only: profiles/r02_experiments.md section 3)
                GemmPlanIn big = a, tail = a;
                big.M = M1; tail.M = a.M - M1;
                l = gemm4_launch(big, m0, 256, a.weave4);
                gemm_plan_rows(tail, no_persist, m0 + M1, p);
                return;
            }
        }
    }
    const int split = choose_splitk(a);
    if (!a.swiglu && !a.f32 && split <= 1 && want_small_m(a)) {
        l = gemm_launch(a, m0, GF_64, 64, 64);
        l.needs_finalize = a.row_norm_out;
        return;
    }
    if (split > 1) {
        l = gemm_launch(a, m0, GF_128_SPLITK, 128, 128);
        l.split = l.grid_y = split;
        l.ws_wired = true;
        l.needs_finalize = a.row_norm_out;
        return;
    }
    if (!a.gather) {
        // measured (scripts/kernel_bench.py --frames 8): wins 15-20 % at <= 256 tiles with K >= 4096, loses at K = 1024 and beyond one round
        if (v == 256 || (v == 0 && (long)gemm_t128(a) <= 256 && a.K >= 4096)) { l = gemm_launch(a, m0, GF_L8, 128, 128); return; }
        const int kern = v == 0 ? choose_gemm_kernel(a) : v;
        const bool n256 = a.N % 256 == 0;
        if ((kern == 4 || kern == 5) && n256) {
            // WEAVE (k_gemm.h gemm3_body; same bits): the LDS-DMA issue woven into the MFMA phases.  Measured round 5 (profiles/r05_experiments.md):
            // -2...-9 % back to back with the operands warm in the Infinity Cache, but +4...+12 % IN THE PIPELINE (down 206 -> 218 us, o 66 -> 69,
            // Conv3d on the 192-row tiles 425 -> 476): the woven pieces have 1.5 phases of flight instead of 3, which cold weights do not forgive.
            // So it is a lab switch: variant 5 or VL2_GEMM_WEAVE.
            l = gemm_launch(a, m0, GF_128x256, 128, 256);
            l.woven = a.lab && (kern == 5 || a.weave);
            l.tr = want_tr_epilogue(a);
            return;
        }
        if (a.lab && kern == 9 && n256) {                                  // lab / forced: the four-wave 256 x 256 kernel (k_gemm8.h)
            l = gemm_launch(a, m0, GF_GEMM8, 256, 256);
            l.tr = want_tr_epilogue(a);
            return;
        }
        if ((kern == 8 || (a.f32 && kern == 12)) && n256) { l = gemm4_launch(a, m0, 256, a.weave4); return; }      // (the 192-row form is built for bf16 outputs only)
        if (!a.f32 && !a.swiglu && a.lab && kern == 10 && n256) { l = gemm4_launch(a, m0, 160, false); return; }    // lab: 160-row tiles (measured: not faster than the 192-row tiles)
        if (!a.f32 && kern == 12 && n256) {
            // 192-row tiles take the woven LDS-DMA issue by default (round 5, scripts/weave4_bench.py, interleaved on one box, same bits): their load
            // phase carries 3-4 pieces + 10 fragment reads under a partner's TWELVE MFMAs -- ViT fc2 82.5 -> 79.4 us, out_proj 30.1 -> 29.3, the
            // decoder's q/k/v 82.0 -> 81.6; the 256-row bodies measure the same either way (16 MFMAs cover the load phase) and keep the load-phase issue
            l = gemm4_launch(a, m0, 192, !a.no_weave4);
            return;
        }
        if (a.lab && want_stream_k(a)) {
            l = gemm_launch(a, m0, GF_128_STREAMK, 128, 128);
            l.grid_x = SK_GRID;
            l.ws_wired = true;
            return;
        }
    }
    l = gemm_launch(a, m0, GF_128, 128, 128);
}

// ---- fp8 form (VL2_GEMM_FP8): the kernels see a row of K bytes as K / 2 16-bit "elements" (k_gemm.h gemm3 / gemm4 FP8).  128 x 256, 256 x 256 or
// 192 x 256 ping-pong tiles by the efficiency model of the 16-bit choice (the 128 x 128 kernels are not built for fp8), LDS epilogue with the row
// table and the column scales.
static inline GemmLaunch gemm_plan_fp8(const GemmPlanIn& in) {
    GemmPlanIn a = in;
    a.K = in.K / 2;
    int kern = a.variant ? a.variant : choose_gemm_kernel(a);
    if (kern != 4 && kern != 8 && kern != 12) kern = 4;
    if (a.f32 && kern == 12) kern = 8;
    return kern == 4 ? gemm_launch(a, 0, GF_FP8_128x256, 128, 256) : gemm_launch(a, 0, kern == 8 ? GF_FP8_256 : GF_FP8_192, kern == 8 ? 256 : 192, 256);
}

// one chunk of a validated call (every operand within the kernels' 32-bit buffer offsets) -> its launches, in order
static inline GemmPlan gemm_plan(const GemmPlanIn& a) {
    GemmPlan p{};
    if (a.fp8) p.l[p.n++] = gemm_plan_fp8(a);
    else if (a.remap) p.l[p.n++] = gemm_launch(a, 0, GF_REMAP, 128, 128);      // row-remap epilogue (patch-embed): dedicated instantiation
    else if (!a.gather && !a.f32 && (a.variant == 24 || (a.variant >= 60 && a.variant <= 81)) && !forced_gemm6(a)) {
        // 24 = the automatic choice WITHOUT the persistent form (A/B); a forced persistent variant the call does not qualify for becomes the same
        GemmPlanIn a0 = a;
        a0.variant = 0;
        gemm_plan_rows(a0, true, 0, p);
    } else gemm_plan_rows(a, false, 0, p);
    return p;
}
