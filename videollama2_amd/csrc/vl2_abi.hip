// libvl2hip.so: extern "C" launchers (include/vl2hip.h) over the gfx950 kernels in k_*.h.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC vl2_abi.hip -o libvl2hip.so   (see build.py)
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>

#define VL2_EXPERIMENTAL 1      // this translation unit DEFINES the experimental entry points too
#include "../../include/vl2hip.h"
#include "k_attn.h"
#include "k_attn2.h"
#include "k_decode.h"
#include "k_fp8.h"
#include "k_gemm.h"
#include "k_gemm6.h"
#include "k_gemm7.h"
#include "k_gemm9.h"
// libvl2hip.so = the default path + the documented options.  The experiments that were measured and lost (the four-wave 256x256 tile, the
// issue-order / stamped forms of the 16x16x32 kernel, the woven LDS-DMA issue outside the 192-row tiles, the two-accumulator persistent
// form, stream-K, the decode tail engine, attention + elected combine in one launch) are compiled only with -DVL2_LAB into
// libvl2hip_lab.so (scripts/build_lab_lib.sh); in the product build a request for one of them is refused with VL2_E_UNSUPP.
#ifdef VL2_LAB
#include "k_decode_tail.h"
#include "k_gemm8.h"
static constexpr bool kLab = true;
#else
static constexpr bool kLab = false;
#endif
#include "k_norm.h"
#include "k_pack.h"
#include "k_sample.h"
#include "k_skinny.h"
#include "k_skinny_fp8.h"
#include "gemm_plan.h"
#include "skinny_plan.h"
#include "k_mxfp4.h"
#include "k_stc.h"
#include "k_vit.h"
#include "k_moe.h"
#include "k_moe_skinny.h"
#include "k_moe_fp8.h"
#include "k_moe_mxfp4.h"
#include "k_moe_gemm8.h"
#include "k_moe_gemm4.h"
#include "k_attn_append.h"
#include "k_attn_shared.h"
#include "k_kv8.h"
#include "k_attn_paged.h"
#include "k_attn_paged_shared.h"
#include "k_attn_paged_kv8.h"
#include "k_kv_swap.h"

static thread_local char g_err[512] = "";
static int32_t fail(int32_t code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
// set-up calls in front of a launch (LDS opt-in, flag re-arming): the first failure is kept and reported by `launched`
static thread_local hipError_t g_setup_err = hipSuccess;
static inline void check(hipError_t e) { if (e != hipSuccess && g_setup_err == hipSuccess) g_setup_err = e; }
static int32_t launched(const char* what) {
    const hipError_t last = hipGetLastError();
    const hipError_t e = g_setup_err != hipSuccess ? g_setup_err : last;
    g_setup_err = hipSuccess;
    if (e != hipSuccess) return fail((int32_t)e, "%s: %s", what, hipGetErrorString(e));
    return 0;
}
#define ST(s) ((hipStream_t)(s))
#define ALIGNED16(p) ((((uintptr_t)(p)) & 15) == 0)

// Dynamic-LDS opt-in of a kernel instance (> 64 KiB needs hipFuncSetAttribute once per device).  Thread-safe and idempotent:
// one atomic bit per device ordinal; two threads racing on the first launch both set the same attribute.
template <auto Kern>
static void lds_attr(int bytes) {
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    check(hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        check(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        done.fetch_or(bit, std::memory_order_release);
    }
}
// the opt-in and the launch of a kernel instance with `lds` bytes of dynamic LDS
template <auto Kern, class... Args>
static void launch(dim3 grid, dim3 block, int lds, hipStream_t s, const Args&... args) {
    lds_attr<Kern>(lds);
    hipLaunchKernelGGL(Kern, grid, block, lds, s, args...);
}

extern "C" int32_t vl2_version(void) { return VL2_ABI_VERSION; }
extern "C" const char* vl2_elem_name(void) { return VL2_ELEM_NAME; }
extern "C" const char* vl2_last_error_string(void) { return g_err; }

// (SK_GRID, SPLITK_MAX_WG, SPLITK_MAX_TILES: gemm_plan.h)
// workspace layout: [SPLITK_MAX_WG][64][256] fp32 partial tiles (stream-K uses the first SK_GRID) | stream-K flags
// [SK_GRID + 1] | split-K tile counters [SPLITK_MAX_TILES] (zero when allocated, re-armed by the kernel itself)
#define SK_FLAGS_OFF ((int64_t)SPLITK_MAX_WG * 64 * 256 * 4)
#define SPLITK_CNT_OFF (SK_FLAGS_OFF + (int64_t)(SK_GRID + 1) * 4 + 12)
#define GEMM6_CTR_OFF ((SPLITK_CNT_OFF + (int64_t)SPLITK_MAX_TILES * 4 + 15) / 16 * 16)   // persistent GEMM: {tiles handed out, workgroups finished}
#define SK_WS_BYTES (GEMM6_CTR_OFF + 16)
extern "C" int64_t vl2_workspace_bytes(void) { return SK_WS_BYTES; }

__global__ void fill_zero_kernel(uint32_t* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0u;
}
extern "C" int32_t vl2_fill_zero(void* p, int64_t bytes, void* stream) {
    if (!p || bytes < 0 || (bytes & 3) || ((uintptr_t)p & 3)) return fail(VL2_E_BADARG, "vl2_fill_zero: null / unaligned pointer or size");
    if (bytes == 0) return 0;
    const int64_t n = bytes / 4;
    const int grid = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(fill_zero_kernel, dim3(grid), dim3(256), 0, ST(stream), (uint32_t*)p, n);
    return launched("vl2_fill_zero");
}

// ------------------------------------------------------------------------------------------------ GEMM
// Which kernel form a call gets is decided in gemm_plan.h (plain host C++, held by tests/test_gemm_plan_host.py); what follows turns a planned
// launch into its instantiation.  The plan's tile sizes are the kernels':
static_assert(GEMM_BM == 128 && GEMM_BN == 128 && GEMM_BK == 64 && GEMM3_BM == 128 && GEMM3_BN == 256 && GEMM4_BM == 256 && GEMM4_BN == 256 && GEMM4_BK == 32 &&
              GEMM7_BN == 128 && GEMMS_BM == 64 && GEMMS_BN == 64, "gemm_plan.h restates the tile sizes of k_gemm.h / k_gemm7.h");

static int cu_count() {
    static std::atomic<int> n{0};                                  // idempotent cache of a device constant (like lds_attr's bits)
    int v = n.load(std::memory_order_relaxed);
    if (v == 0) {
        int dev = 0;
        check(hipGetDevice(&dev));
        check(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
        if (v <= 0) v = 256;
        n.store(v, std::memory_order_relaxed);
    }
    return v;
}

// rows [m0, m0 + rows) of a call as a call of its own (A / C / residual / statistics rows shifted; the gather table keeps its
// row stride idx_ld)
static GemmArgs gemm_rows(const GemmArgs& a0, int m0, int rows, bool f32) {
    GemmArgs a = a0;
    a.M = rows;
    if (a0.a_idx) a.a_idx = a0.a_idx + m0; else a.A = a0.A + (size_t)m0 * a0.lda;
    a.C = f32 ? (void*)((float*)a0.C + (size_t)m0 * a0.ldc) : (void*)((bf16_t*)a0.C + (size_t)m0 * a0.ldc);
    if (a0.res) a.res = a0.res + (size_t)m0 * a0.ldres;
    if (a0.stats_out) a.stats_out = a0.stats_out + (size_t)m0 * a0.stats_out_np * 2;
    if (a0.stats_in) a.stats_in = a0.stats_in + (size_t)m0 * a0.stats_in_np * 2;
    if (a0.row_norm) a.row_norm = a0.row_norm + (size_t)m0 * 2;
    if (a0.row_norm_out) { a.row_norm_out = a0.row_norm_out + (size_t)m0 * 2; a.row_ticket = a0.row_ticket + m0 / 64; }   // 64 = the smallest tile height
    a.tiles_m = (rows + GEMM_BM - 1) / GEMM_BM;
    return a;
}

// One planned launch -> its instantiation.  ACT / SW / F32 / G are the call's epilogue and operand forms (gemm_dispatch); a `case` is compiled only
// for the combinations its kernel is built for, and the lab forms only with -DVL2_LAB -- the plan never hands a form to a combination without it.
template <int ACT, bool SW, bool F32, bool G>
static void launch_planned(const GemmArgs& a0, const GemmLaunch& l, void* ws, hipStream_t s) {
    GemmArgs a = gemm_rows(a0, l.m0, l.rows, F32);
    a.tiles_m = l.tiles_m;
    a.tiles_n = l.tiles_n;
    a.tile_group = l.tile_group;
    const dim3 grid(l.grid_x, l.grid_y), b128(128), b256(256), b512(512);
    constexpr bool kPlain = !G && !F32 && ACT == ACT_NONE;      // what the 16 x 16 x 32 kernels are built for
    switch (l.form) {
    case GF_128:
        launch<gemm_bf16_kernel<ACT, SW, F32, G>>(grid, b256, GEMM_LDS_BYTES, s, a);   // 64 KiB dynamic LDS needs the opt-in once per kernel instance
        return;
    case GF_128_SPLITK:
        a.sk_ws = (float*)ws;
        a.sk_flags = (int*)((char*)ws + SPLITK_CNT_OFF);
        launch<gemm_bf16_kernel<ACT, SW, F32, G, false, true>>(grid, b256, GEMM_LDS_BYTES, s, a);
        return;
    case GF_128_STREAMK:
        if constexpr (!G && kLab) {
            a.sk_ws = (float*)ws;
            a.sk_flags = (int*)((char*)ws + SK_FLAGS_OFF);
            a.sk_per = (a.tiles_m * a.tiles_n * (a.K / GEMM_BK) + SK_GRID - 1) / SK_GRID;
            lds_attr<gemm_sk_bf16_kernel<ACT, SW, F32>>(GEMM_LDS_BYTES);
            check(hipMemsetAsync(a.sk_flags, 0, (SK_GRID + 1) * 4, s));               // flags re-armed before EVERY launch (guide G16)
            hipLaunchKernelGGL((gemm_sk_bf16_kernel<ACT, SW, F32>), grid, b256, GEMM_LDS_BYTES, s, a);
        }
        return;
    case GF_64:
        if constexpr (!SW && !F32) launch<gemm_s_bf16_kernel<ACT, G>>(grid, b128, GEMMS_LDS_BYTES, s, a);
        return;
    case GF_L8:
        if constexpr (!G) launch<gemm_l8_bf16_kernel<ACT, SW, F32>>(grid, b512, GEMML_LDS_BYTES, s, a);
        return;
    case GF_128x256:
        if constexpr (!G) {
            if constexpr (kLab) {
                if (l.woven) {
                    if constexpr (!F32) {
                        if (l.tr) { launch<gemm3_bf16_kernel<ACT, SW, false, true, -1, true>>(grid, b512, GEMM3_LDS_BYTES, s, a); return; }
                    }
                    launch<gemm3_bf16_kernel<ACT, SW, F32, false, -1, true>>(grid, b512, GEMM3_LDS_BYTES, s, a);
                    return;
                }
            }
            if constexpr (!F32) {
                if (l.tr) { launch<gemm3_bf16_kernel<ACT, SW, false, true>>(grid, b512, GEMM3_LDS_BYTES, s, a); return; }
            }
            launch<gemm3_bf16_kernel<ACT, SW, F32>>(grid, b512, GEMM3_LDS_BYTES, s, a);
        }
        return;
    case GF_G4_256:           // the product builds the load-phase issue only (the woven one: lab)
        if constexpr (!G) {
            if constexpr (!F32) {
                if constexpr (kLab) {
                    if (l.woven) {
                        if (l.tr) launch<gemm4_bf16_kernel<ACT, SW, false, true, -1, 256, true>>(grid, b512, GEMM4_LDS_BYTES, s, a);
                        else launch<gemm4_bf16_kernel<ACT, SW, false, false, -1, 256, true>>(grid, b512, GEMM4_LDS_BYTES, s, a);
                        return;
                    }
                }
                if (l.tr) { launch<gemm4_bf16_kernel<ACT, SW, false, true, -1, 256>>(grid, b512, GEMM4_LDS_BYTES, s, a); return; }
            }
            launch<gemm4_bf16_kernel<ACT, SW, F32, false, -1, 256>>(grid, b512, GEMM4_LDS_BYTES, s, a);
        }
        return;
    case GF_G4_192:           // bf16 outputs only; the product builds the woven issue only (the load-phase one: lab)
        if constexpr (!G && !F32) {
            if constexpr (kLab) {
                if (!l.woven) {
                    if (l.tr) launch<gemm4_bf16_kernel<ACT, SW, false, true, -1, 192>>(grid, b512, GEMM4_LDS_BYTES, s, a);
                    else launch<gemm4_bf16_kernel<ACT, SW, false, false, -1, 192>>(grid, b512, GEMM4_LDS_BYTES, s, a);
                    return;
                }
            }
            if (l.tr) launch<gemm4_bf16_kernel<ACT, SW, false, true, -1, 192, true>>(grid, b512, GEMM4_LDS_BYTES, s, a);
            else launch<gemm4_bf16_kernel<ACT, SW, false, false, -1, 192, true>>(grid, b512, GEMM4_LDS_BYTES, s, a);
        }
        return;
    case GF_G4_160:
        if constexpr (!G && !F32 && !SW && kLab) launch<gemm4_bf16_kernel<ACT, SW, false, false, -1, 160>>(grid, b512, GEMM4_LDS_BYTES, s, a);
        return;
    case GF_GEMM6:
        if constexpr (!G && !F32) {
            a.tile_first_dyn = l.dyn == 2;
            if (l.dyn == 0) a.tile_ctr = nullptr;
            if (l.tile_h == 256) launch<gemm6_bf16_kernel<ACT, SW, 256, false>>(grid, b512, GEMM6_LDS_BYTES, s, a);
            else if (!l.acc2) launch<gemm6_bf16_kernel<ACT, SW, 192, false>>(grid, b512, GEMM6_LDS_BYTES, s, a);
            else if constexpr (kLab) launch<gemm6_bf16_kernel<ACT, SW, 192, true>>(grid, b512, GEMM6_LDS_BYTES, s, a);      // measured slower than one set
        }
        return;
    case GF_GEMM7:
        if constexpr (!SW) {
            if constexpr (kLab) {
                if (l.woven && l.tile_h == 224) { launch<gemm7_bf16_kernel<ACT, F32, G, 3, true>>(grid, b512, Gemm7Geo<3>::LDS_BYTES, s, a); return; }
                if (l.woven) { launch<gemm7_bf16_kernel<ACT, F32, G, 2, true>>(grid, b512, Gemm7Geo<2>::LDS_BYTES, s, a); return; }
            }
            if (l.tile_h == 224) launch<gemm7_bf16_kernel<ACT, F32, G, 3, false>>(grid, b512, Gemm7Geo<3>::LDS_BYTES, s, a);
            else launch<gemm7_bf16_kernel<ACT, F32, G, 2, false>>(grid, b512, Gemm7Geo<2>::LDS_BYTES, s, a);
        }
        return;
#ifdef VL2_LAB
    case GF_GEMM8:
        if constexpr (!G) {
            if constexpr (!F32) {
                if (l.tr) { launch<gemm8_bf16_kernel<ACT, SW, false, true>>(grid, b256, GEMM8_LDS_BYTES, s, a); return; }
            }
            launch<gemm8_bf16_kernel<ACT, SW, F32, false>>(grid, b256, GEMM8_LDS_BYTES, s, a);
        }
        return;
    case GF_GEMM7_16:
        if constexpr (kPlain && !SW) {
            if (l.tile_h == 224) launch<gemm7_16_bf16_kernel<3>>(grid, b512, Gemm7Geo<3>::LDS_BYTES, s, a);
            else launch<gemm7_16_bf16_kernel<2>>(grid, b512, Gemm7Geo<2>::LDS_BYTES, s, a);
        }
        return;
#endif
    case GF_GEMM9:            // MODE 9 (variant 26): 64-deep phases, 5-stage ring = the whole 160 KiB of LDS; MODE 1 ... 8: lab (variants 17 ... 23, 25; k_gemm9.h)
        if constexpr (kPlain) {
            if (l.mode == 7 || l.mode == 8) a.sk_ws = l.ws_wired ? (float*)ws : nullptr;      // the stamps' sums go into the workspace (scripts/gemm9_phase_stamps.py)
            if (l.mode == 9) { launch<gemm9_bf16_kernel<SW, 9>>(grid, b512, 5 * GEMM4_STAGE, s, a); return; }
            if constexpr (kLab) {
                switch (l.mode) {
                case 1: launch<gemm9_bf16_kernel<SW, 1>>(grid, b512, GEMM4_LDS_BYTES, s, a); return;
                case 2: launch<gemm9_bf16_kernel<SW, 2>>(grid, b512, GEMM4_LDS_BYTES, s, a); return;
                case 3: launch<gemm9_bf16_kernel<SW, 3>>(grid, b512, GEMM4_LDS_BYTES, s, a); return;
                case 4: launch<gemm9_bf16_kernel<SW, 4>>(grid, b512, GEMM4_LDS_BYTES, s, a); return;
                case 5: launch<gemm9_bf16_kernel<SW, 5>>(grid, b512, GEMM4_LDS_BYTES, s, a); return;
                case 6: launch<gemm9_bf16_kernel<SW, 6>>(grid, b512, GEMM4_LDS_BYTES, s, a); return;
                case 7: launch<gemm9_bf16_kernel<SW, 7>>(grid, b512, GEMM4_LDS_BYTES, s, a); return;
                case 8: launch<gemm9_bf16_kernel<SW, 8>>(grid, b512, GEMM4_LDS_BYTES, s, a); return;
                }
            }
            launch<gemm9_bf16_kernel<SW, 0>>(grid, b512, GEMM4_LDS_BYTES, s, a);
        }
        return;
    case GF_L8_16:
        if constexpr (kPlain && !SW) launch<gemm_l8_16_bf16_kernel<false>>(grid, b512, GEMML_LDS_BYTES, s, a);
        return;
    case GF_MIX:
    case GF_MIX16:
        if constexpr (!G && !F32) {
            GemmArgs tail = gemm_rows(a0, l.m0 + l.rows, l.tail_rows, F32);
            tail.tiles_m = l.tail_tiles_m;
            tail.tiles_n = l.tail_tiles_n;
            tail.tile_group = l.tail_tile_group;
            const int n_big = l.tiles_m * l.tiles_n;
            if (l.form == GF_MIX16) {
                if constexpr (kPlain) {
                    if constexpr (SW) {
                        if (l.mode == 9) { launch<gemm_mix16_bf16_kernel<SW, 9>>(grid, b512, 5 * GEMM4_STAGE, s, a, tail, n_big); return; }
                    }
                    launch<gemm_mix16_bf16_kernel<SW>>(grid, b512, GEMM4_LDS_BYTES, s, a, tail, n_big);
                }
                return;
            }
            if constexpr (kLab) {
                if (l.woven) {
                    if (l.tr) launch<gemm_mix_bf16_kernel<ACT, SW, true, true>>(grid, b512, GEMM4_LDS_BYTES, s, a, tail, n_big);
                    else launch<gemm_mix_bf16_kernel<ACT, SW, false, true>>(grid, b512, GEMM4_LDS_BYTES, s, a, tail, n_big);
                    return;
                }
            }
            if (l.tr) launch<gemm_mix_bf16_kernel<ACT, SW, true>>(grid, b512, GEMM4_LDS_BYTES, s, a, tail, n_big);
            else launch<gemm_mix_bf16_kernel<ACT, SW, false>>(grid, b512, GEMM4_LDS_BYTES, s, a, tail, n_big);
        }
        return;
    }
}

// the fp8 form's three kernels (`a` arrives with K, lda, ldw already halved: the kernels see a row of K bytes as K / 2 16-bit "elements")
template <int ACT, bool SW, bool F32>
static void launch_planned_fp8(const GemmArgs& a0, const GemmLaunch& l, hipStream_t s) {
    GemmArgs a = a0;
    a.tiles_m = l.tiles_m;
    a.tiles_n = l.tiles_n;
    const dim3 grid(l.grid_x), b512(512);
    if (l.form == GF_FP8_128x256) launch<gemm3_fp8_kernel<ACT, SW, F32>>(grid, b512, GEMM3_LDS_BYTES, s, a);
    else if (l.form == GF_FP8_256) launch<gemm4_fp8_kernel<ACT, SW, F32, 256>>(grid, b512, GEMM4_LDS_BYTES, s, a);
    else if constexpr (!F32) launch<gemm4_fp8_kernel<ACT, SW, false, 192>>(grid, b512, GEMM4_LDS_BYTES, s, a);
}

// one chunk (every operand within the kernels' 32-bit buffer offsets): its plan, launch by launch, on the right instantiation.  *need_fin is set
// when a planned kernel leaves `row_norm_out` to a row_norm_finalize launch.
static int32_t gemm_dispatch(const GemmArgs& a, GemmPlanIn in, int act, void* ws, bool* need_fin, hipStream_t s) {
    in.M = a.M; in.N = a.N;
    in.row_norm_out = a.row_norm_out != nullptr;
    const GemmPlan p = gemm_plan(in);
    for (int i = 0; i < p.n; ++i) {
        const GemmLaunch& l = p.l[i];
        if (l.needs_finalize) *need_fin = true;
        if (l.form == GF_REMAP) launch<gemm_bf16_kernel<ACT_NONE, false, false, false, true>>(dim3(l.grid_x), dim3(256), GEMM_LDS_BYTES, s, a);
        else if (in.swiglu) launch_planned<ACT_NONE, true, false, false>(a, l, ws, s);
        else if (in.gather) {
            if (act == VL2_ACT_SILU) launch_planned<ACT_SILU, false, false, true>(a, l, ws, s);
            else launch_planned<ACT_NONE, false, false, true>(a, l, ws, s);
        } else if (in.f32) launch_planned<ACT_NONE, false, true, false>(a, l, ws, s);
        else {
            switch (act) {
                case VL2_ACT_NONE: launch_planned<ACT_NONE, false, false, false>(a, l, ws, s); break;
                case VL2_ACT_QGELU: launch_planned<ACT_QGELU, false, false, false>(a, l, ws, s); break;
                case VL2_ACT_GELU: launch_planned<ACT_GELU, false, false, false>(a, l, ws, s); break;
                case VL2_ACT_SILU: launch_planned<ACT_SILU, false, false, false>(a, l, ws, s); break;
                case VL2_ACT_GELU_TANH: launch_planned<ACT_GELU_TANH, false, false, false>(a, l, ws, s); break;
                default: return fail(VL2_E_UNSUPP, "vl2_gemm: unknown act %d", act);
            }
        }
    }
    return 0;
}

extern "C" int32_t vl2_gemm(const vl2_gemm_desc* d, void* stream) {
    if (!d || d->size != sizeof(vl2_gemm_desc)) return fail(VL2_E_BADARG, "vl2_gemm: descriptor missing or of another ABI (size %u, expected %zu)", d ? d->size : 0u, sizeof(vl2_gemm_desc));
    const int M = d->M, N = d->N, K = d->K, act = d->act;
    if (!d->A || !d->W || !d->C || M <= 0 || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_gemm: null pointer or empty shape");
    if (N % 128 || K % 64) return fail(VL2_E_SHAPE, "vl2_gemm: need N%%128==0 and K%%64==0 (N=%d K=%d)", N, K);
    if ((d->lda % 8) || (d->ldw % 8) || (d->ldc % 8) || (d->res && (d->ldres % 8)) || !ALIGNED16(d->A) || !ALIGNED16(d->W) || !ALIGNED16(d->C) ||
        (d->res && !ALIGNED16(d->res)) || (d->bias && !ALIGNED16(d->bias)) || (d->w_colsum && !ALIGNED16(d->w_colsum)) ||
        (d->stats_in && !ALIGNED16(d->stats_in)))
        return fail(VL2_E_SHAPE, "vl2_gemm: pointers / leading dims must be 16-byte aligned");
    const bool sw = d->flags & VL2_GEMM_SWIGLU, f32 = d->flags & VL2_GEMM_OUT_F32, g = d->a_idx != nullptr;
    if (d->flags & VL2_GEMM_FP8) {
        // W8A8 on the fp8 matrix pipe: K counts e4m3fn elements = bytes; row scales through `row_norm` (vl2_quant_act_fp8), column scales `col_scale`
        if (g || d->out_grp > 0 || d->res_row_mod > 0 || d->stats_out || d->stats_in || d->w_colsum || (d->flags & (VL2_GEMM_SPLITK | VL2_GEMM_PERSISTENT)))
            return fail(VL2_E_UNSUPP, "vl2_gemm: the fp8 form supports plain rows with bias / activation / SwiGLU / residual only");
        if (!d->row_norm || !d->col_scale) return fail(VL2_E_BADARG, "vl2_gemm: the fp8 form needs row_norm (vl2_quant_act_fp8) and col_scale (vl2_pack_quant_fp8)");
        if (N % 256 || K % 128 || (d->lda % 16) || (d->ldw % 16)) return fail(VL2_E_SHAPE, "vl2_gemm: the fp8 form needs N%%256==0, K%%128==0, 16-byte rows (N=%d K=%d)", N, K);
        if (sw && (f32 || act != VL2_ACT_NONE || d->bias)) return fail(VL2_E_UNSUPP, "vl2_gemm: SWIGLU excludes bias/act/f32");
        if (f32 && act != VL2_ACT_NONE) return fail(VL2_E_UNSUPP, "vl2_gemm: f32 output supports act none");
        if (!ALIGNED16(d->col_scale) || (((uintptr_t)d->row_norm) & 7)) return fail(VL2_E_SHAPE, "vl2_gemm: col_scale must be 16-byte, row_norm 8-byte aligned");
        if ((int64_t)(M - 1) * d->lda + K >= ((int64_t)1 << 31) - 65536 || (int64_t)(N - 1) * d->ldw + K >= ((int64_t)1 << 31) - 65536)
            return fail(VL2_E_UNSUPP, "vl2_gemm: fp8 operands of 2 GiB or more are not chunked");
        const int v8 = d->variant;
        if (!(v8 == 0 || v8 == 4 || v8 == 8 || v8 == 12)) return fail(VL2_E_BADARG, "vl2_gemm: the fp8 form has variants 0 / 4 / 8 / 12 (got %d)", v8);
        GemmArgs a{};
        a.A = (const bf16_t*)d->A; a.W = (const bf16_t*)d->W; a.C = d->C; a.bias = d->bias; a.res = (const bf16_t*)d->res;
        a.M = M; a.N = N; a.K = K / 2; a.lda = d->lda / 2; a.ldw = d->ldw / 2; a.ldc = d->ldc; a.ldres = d->ldres;
        a.norm = VL2_NORM_RMS; a.row_norm = d->row_norm; a.col_scale = d->col_scale;
        a.stats_out_np = N / 64; a.stats_in_np = a.K / 64; a.idx_ld = M;
        hipStream_t s8 = ST(stream);
        GemmPlanIn in8{};
        in8.M = M; in8.N = N; in8.K = K; in8.f32 = f32; in8.fp8 = true; in8.variant = v8;
        const GemmLaunch l8 = gemm_plan(in8).l[0];
        if (sw) launch_planned_fp8<ACT_NONE, true, false>(a, l8, s8);
        else if (f32) launch_planned_fp8<ACT_NONE, false, true>(a, l8, s8);
        else if (act == VL2_ACT_NONE) launch_planned_fp8<ACT_NONE, false, false>(a, l8, s8);
        else if (act == VL2_ACT_SILU) launch_planned_fp8<ACT_SILU, false, false>(a, l8, s8);
        else return fail(VL2_E_UNSUPP, "vl2_gemm: the fp8 form supports act none / silu");
        return launched("vl2_gemm (fp8)");
    }
    if (d->col_scale) return fail(VL2_E_BADARG, "vl2_gemm: col_scale without VL2_GEMM_FP8");
    if (g && (d->seg_k <= 0 || d->seg_k % 64 || K % d->seg_k)) return fail(VL2_E_SHAPE, "vl2_gemm: bad gather segments");
    const bool remap = d->out_grp > 0 || d->res_row_mod > 0;
    if (remap && (sw || g || f32 || act != VL2_ACT_NONE || d->norm || d->stats_out)) return fail(VL2_E_UNSUPP, "vl2_gemm: row remap supports plain bf16 output only");
    if (sw && (f32 || g || act != VL2_ACT_NONE || d->bias)) return fail(VL2_E_UNSUPP, "vl2_gemm: SWIGLU excludes bias/act/f32/gather");
    if (g && f32) return fail(VL2_E_UNSUPP, "vl2_gemm: gather + f32 not built");
    if (g && act != VL2_ACT_NONE && act != VL2_ACT_SILU) return fail(VL2_E_UNSUPP, "vl2_gemm: gather supports act none/silu");
    if (f32 && act != VL2_ACT_NONE) return fail(VL2_E_UNSUPP, "vl2_gemm: f32 output supports act none");
    if (d->norm != VL2_NORM_NONE) {
        if (d->norm != VL2_NORM_RMS && d->norm != VL2_NORM_LN) return fail(VL2_E_BADARG, "vl2_gemm: unknown norm %d", d->norm);
        if ((!d->stats_in && !d->row_norm) || g || remap) return fail(VL2_E_BADARG, "vl2_gemm: a fused norm needs stats_in (or row_norm) and plain A rows");
        if (d->norm == VL2_NORM_LN && (!d->w_colsum || sw)) return fail(VL2_E_BADARG, "vl2_gemm: fused LayerNorm needs w_colsum (and excludes SWIGLU)");
        if (!d->row_norm && (K % 128)) return fail(VL2_E_SHAPE, "vl2_gemm: reducing stats_in in the GEMM needs K %% 128 == 0 (16-byte pairs of partials; K=%d): pass row_norm (vl2_row_norm_finalize)", K);
    }
    if (d->stats_out && (sw || f32)) return fail(VL2_E_UNSUPP, "vl2_gemm: stats_out needs a plain bf16 output");
    if (d->row_norm_out) {
        if (!d->stats_out || !d->row_ticket) return fail(VL2_E_BADARG, "vl2_gemm: row_norm_out needs stats_out and row_ticket");
        if (d->norm_out != VL2_NORM_RMS && d->norm_out != VL2_NORM_LN) return fail(VL2_E_BADARG, "vl2_gemm: unknown norm_out %d", d->norm_out);
        if ((((uintptr_t)d->row_norm_out) & 7) || (((uintptr_t)d->row_ticket) & 3)) return fail(VL2_E_SHAPE, "vl2_gemm: row_norm_out must be 8-byte, row_ticket 4-byte aligned");
    }
    if (d->ws && (d->ws_bytes < SK_WS_BYTES || !ALIGNED16(d->ws))) return fail(VL2_E_BADARG, "vl2_gemm: workspace needs >= %lld bytes, 16-byte aligned", (long long)SK_WS_BYTES);
    const int v = d->variant;
    if (!(v == 0 || v == 1 || v == 2 || v == 4 || v == 5 || v == 8 || v == 9 || v == 10 || v == 12 || (v >= 16 && v <= 23) || v == 25 || (v >= 26 && v <= 29) || v == 32 || v == 24 || v == 60 || v == 61 || v == 62 || v == 70 || v == 71 || v == 80 || v == 81 || v == 192 || v == 193 || v == 224 || v == 225 || v == 256)) return fail(VL2_E_BADARG, "vl2_gemm: unknown variant %d", v);
    if (!kLab && (v == 2 || v == 5 || v == 9 || v == 10 || (v >= 17 && v <= 23) || v == 25 || (v >= 27 && v <= 29) || v == 62 || v == 193 || v == 225))
        return fail(VL2_E_UNSUPP, "vl2_gemm: variant %d is a lab form: built into libvl2hip_lab.so only (scripts/build_lab_lib.sh)", v);
    // everything the plan reads (gemm_plan.h); M, N and row_norm_out are filled in per chunk
    GemmPlanIn in{};
    in.K = K; in.act = act != VL2_ACT_NONE; in.swiglu = sw; in.f32 = f32; in.gather = g; in.remap = remap;
    in.res = d->res != nullptr; in.stats_out = d->stats_out != nullptr; in.norm = d->norm != VL2_NORM_NONE; in.row_norm = d->row_norm != nullptr;
    in.tile_ctr = d->tile_ctr || d->ws; in.ws = d->ws != nullptr; in.ws_bytes = d->ws_bytes;
    in.variant = v; in.lab = kLab;
    in.splitk = (d->flags & VL2_GEMM_SPLITK) != 0;
    in.persist = (d->flags & VL2_GEMM_PERSISTENT) != 0;
    in.no_mix = (d->flags & VL2_GEMM_NO_MIX) != 0;
    in.no_fill = (d->flags & VL2_GEMM_NO_FILL) != 0;
    in.weave = (d->flags & VL2_GEMM_WEAVE) != 0;
    in.weave4 = (d->flags & VL2_GEMM_WEAVE4) != 0;
    in.no_weave4 = (d->flags & VL2_GEMM_NO_WEAVE4) != 0;
    in.N = N;
    // the 16 x 16 x 32 kernel: the flag is a wish (ignored where the kernel is not built), variant 16 a demand
    if (gemm_v16(v) && !gemm_ok16(in)) return fail(VL2_E_UNSUPP, "vl2_gemm: variant 16 (16x16x32 MFMA) is built for plain bf16 outputs without activation / gather / remap / stats_out, N %% 256 == 0");
    in.mfma16 = want_mfma16(in, (d->flags & VL2_GEMM_MFMA16) != 0);       // decided here, on the whole call; the plan of a chunk takes it as given
    bool need_fin = d->row_norm_out && (d->flags & VL2_GEMM_NO_TICKET);      // A/B: the separate launch as in rounds 3-4
    GemmArgs a{};
    a.A = (const bf16_t*)d->A; a.W = (const bf16_t*)d->W; a.C = d->C; a.bias = d->bias; a.res = (const bf16_t*)d->res;
    a.a_idx = d->a_idx; a.zero_row = nullptr;
    a.M = M; a.N = N; a.K = K; a.lda = d->lda; a.ldw = d->ldw; a.ldc = d->ldc; a.ldres = d->ldres; a.seg_k = d->seg_k;
    a.out_grp = d->out_grp; a.out_grp_pad = d->out_grp_pad; a.out_row_off = d->out_row_off;
    a.res_row_mod = d->res_row_mod; a.res_row_off = d->res_row_off;
    a.tiles_m = (M + GEMM_BM - 1) / GEMM_BM; a.tiles_n = N / GEMM_BN;
    a.idx_ld = M;
    a.stats_out = d->stats_out; a.stats_out_np = N / 64;
    a.stats_in = d->stats_in; a.stats_in_np = K / 64;
    a.norm = d->norm; a.norm_eps = d->norm_eps; a.w_colsum = d->w_colsum; a.row_norm = d->row_norm;
    if (d->row_norm_out && !need_fin) { a.row_norm_out = d->row_norm_out; a.row_ticket = (unsigned*)d->row_ticket; a.norm_out = d->norm_out; a.norm_out_eps = d->norm_out_eps; }
    a.tile_ctr = d->tile_ctr ? (unsigned*)d->tile_ctr : d->ws ? (unsigned*)((char*)d->ws + GEMM6_CTR_OFF) : nullptr;
    if (d->tile_ctr && ((uintptr_t)d->tile_ctr & 7)) return fail(VL2_E_BADARG, "vl2_gemm: tile_ctr must be 8-byte aligned");
    if (in.persist || (v >= 60 && v <= 81)) in.cus = cu_count();      // only the persistent form's plan reads it
    hipStream_t s = ST(stream);
    // The kernels address A and W through raw buffer resources: 32-bit byte offsets, NUM_RECORDS 2^31 - 1.  Operands beyond
    // that are covered in chunks of rows (A, C, residual, statistics) / columns (W, bias, w_colsum, C columns): e.g. the
    // [152064 x 8192] bf16 lm_head of VideoLLaMA2-72B (2.49 GB) runs as two column chunks.  Chunk sizes are multiples of
    // 256 (every tile shape, the 64-row SwiGLU blocks).  The gathered row pool cannot be chunked (its extent is unknown here).
    const int64_t LIM = ((int64_t)1 << 31) - 65536;
    int64_t rows_a = M, rows_w = N;
    if (!g && ((int64_t)(M - 1) * d->lda + K) * 2 >= LIM) rows_a = ((LIM / 2 - K) / d->lda + 1) / 256 * 256;
    if (((int64_t)(N - 1) * d->ldw + K) * 2 >= LIM) rows_w = ((LIM / 2 - K) / d->ldw + 1) / 256 * 256;
    if (rows_a <= 0 || rows_w <= 0) return fail(VL2_E_SHAPE, "vl2_gemm: a single 256-row block of A or W exceeds 2 GiB (lda %d, ldw %d)", d->lda, d->ldw);
    if ((rows_a < M || rows_w < N) && remap) return fail(VL2_E_UNSUPP, "vl2_gemm: row remap with >= 2 GiB operands not built");
    for (int64_t m0 = 0; m0 < M; m0 += rows_a) {
        const int mr = (int)(M - m0 < rows_a ? M - m0 : rows_a);
        for (int64_t n0 = 0; n0 < N; n0 += rows_w) {
            const int nr = (int)(N - n0 < rows_w ? N - n0 : rows_w);
            GemmArgs c = (mr == M) ? a : gemm_rows(a, (int)m0, mr, f32);
            if (nr != N) {
                c.N = nr;
                c.tiles_n = nr / GEMM_BN;
                c.W = a.W + (size_t)n0 * a.ldw;
                if (a.bias) c.bias = a.bias + n0;
                if (a.w_colsum) c.w_colsum = a.w_colsum + n0;
                const size_t ccol = sw ? (size_t)n0 / 2 : (size_t)n0;
                c.C = f32 ? (void*)((float*)c.C + ccol) : (void*)((bf16_t*)c.C + ccol);
                if (c.res) c.res = c.res + ccol;
                if (c.stats_out) c.stats_out = c.stats_out + (size_t)(n0 / 64) * 2;
                if (c.row_norm_out) { c.row_norm_out = nullptr; need_fin = true; }      // a column chunk sees a part of the row's partials only
            }
            const int32_t rc = gemm_dispatch(c, in, act, d->ws, &need_fin, s);
            if (rc) return rc;
        }
    }
    if (need_fin)      // a kernel without the producer-side finalize ran (64 x 64 tiles, split-K, column chunks), or VL2_GEMM_NO_TICKET asked for the launch
        hipLaunchKernelGGL(row_norm_finalize_kernel, dim3((M + 31) / 32), dim3(256), 0, s, (const float*)d->stats_out, d->row_norm_out, M, N / 64, N, d->norm_out, d->norm_out_eps);
    return launched("vl2_gemm");
}

extern "C" int32_t vl2_row_norm_finalize(const float* stats, float* row_norm, int32_t rows, int32_t np, int32_t K, int32_t norm, float eps,
                                         void* stream) {
    if (!stats || !row_norm || rows <= 0 || np <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_row_norm_finalize: null pointer or empty shape");
    if (norm != VL2_NORM_RMS && norm != VL2_NORM_LN) return fail(VL2_E_BADARG, "vl2_row_norm_finalize: unknown norm %d", norm);
    if (!ALIGNED16(stats) || (((uintptr_t)row_norm) & 7)) return fail(VL2_E_SHAPE, "vl2_row_norm_finalize: stats must be 16-byte, row_norm 8-byte aligned");
    hipLaunchKernelGGL(row_norm_finalize_kernel, dim3((rows + 31) / 32), dim3(256), 0, ST(stream), stats, row_norm, rows, np, K, norm, eps);
    return launched("vl2_row_norm_finalize");
}

extern "C" int32_t vl2_row_stats(const void* x, float* stats, int32_t rows, int32_t C, int32_t ldx, void* stream) {
    if (!x || !stats || rows <= 0 || C <= 0) return fail(VL2_E_BADARG, "vl2_row_stats: null pointer or empty shape");
    if (C % 64 || ldx % 8 || !ALIGNED16(x)) return fail(VL2_E_SHAPE, "vl2_row_stats: need C%%64==0 and 16-byte aligned rows (C=%d)", C);
    hipLaunchKernelGGL(row_stats_kernel, dim3((rows + 3) / 4), dim3(256), 0, ST(stream), (const bf16_t*)x, stats, rows, C, ldx);
    return launched("vl2_row_stats");
}

// ------------------------------------------------------------------------------------------------ skinny-M GEMM (batched decode)
// ONE host routine behind the three weight formats' entries (16-bit, fp8 k_skinny_fp8.h, MXFP4 k_mxfp4.h): the common checks, the plan
// (skinny_plan.h), the launch of the format's kernel (K1 / K2 / K4 = its MT = 1 / 2 / 4 instances) and the ordered reduce.  The entry checks
// its own format's operands first and hands in `a` with the operands, shape and strides set, whether its layout rule holds (`layout_ok`,
// reported as `rule` in its place in the order of checks), `row_scale` = the fp32 row scales the reduce applies (fp8) or null, and `shrink` =
// the K split may shrink to fit the workspace (the 16-bit entry alone: the quantised entries pick the split from N and K only, so a row's bits
// do not depend on M, and at the decode shapes and the default workspace it is the 16-bit kernel's split -- the output is
// vl2_gemm_skinny_bf16's on the dequantised weights).  Every check precedes every launch.
template <auto K1, auto K2, auto K4, class Args>
static int32_t skinny_rows(const char* who, Args a, bool layout_ok, const char* rule, const float* row_scale, bool shrink, void* C, const float* bias,
                           const void* res, int32_t ldc, int32_t ldres, int32_t flags, void* ws, int64_t ws_bytes, void* stream) {
    const int M = a.M, N = a.N, K = a.K;
    if (!a.A || !C || M <= 0 || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "%s: null pointer or empty shape", who);
    const bool sw = flags & VL2_GEMM_SWIGLU, f32 = flags & VL2_GEMM_OUT_F32;
    if (M > 64) return fail(VL2_E_SHAPE, "%s: M=%d rows, need M<=64 (split larger batches)", who, M);
    if (N % 64 || (sw && N % 128)) return fail(VL2_E_SHAPE, "%s: need N%%64==0 (N%%128==0 with SWIGLU; N=%d)", who, N);
    if (K % 32) return fail(VL2_E_SHAPE, "%s: need K%%32==0 (K=%d)", who, K);
    if (!layout_ok) return fail(VL2_E_SHAPE, "%s: need %s", who, rule);
    if (sw && (bias || f32)) return fail(VL2_E_UNSUPP, "%s: SWIGLU excludes bias / f32 output", who);
    if (!ws || !ALIGNED16(ws) || ws_bytes <= 0) return fail(VL2_E_BADARG, "%s: needs a 16-byte aligned workspace (fp32 partial sums)", who);
    SkinnyPlan pl;
    const int rc = skinny_plan(M, N, K, ws_bytes, shrink, pl);
    if (rc == SKINNY_PLAN_WS_SMALL) return fail(VL2_E_BADARG, "%s: workspace too small (%lld bytes, need %lld)", who, (long long)ws_bytes, (long long)pl.ws_need);
    if (rc != SKINNY_PLAN_OK) return fail(VL2_E_SHAPE, "%s: no K chunking for K=%d", who, K);
    a.part = (float*)ws;
    a.kslice = pl.kslice;
    a.kchunk = pl.kchunk;
    hipStream_t s = ST(stream);
    const dim3 gk(N / 64, pl.ks), b(256);
    if (pl.mt == 1) { lds_attr<K1>(65536); hipLaunchKernelGGL(K1, gk, b, pl.lds, s, a); }
    else if (pl.mt == 2) { lds_attr<K2>(65536); hipLaunchKernelGGL(K2, gk, b, pl.lds, s, a); }
    else { lds_attr<K4>(65536); hipLaunchKernelGGL(K4, gk, b, pl.lds, s, a); }
    SkinnyReduceArgs r{(const float*)ws, C, bias, (const bf16_t*)res, M, pl.Mp, N, pl.ks, ldc, ldres, row_scale};
    const int ncol = sw ? N / 2 : N;
    const dim3 g((M * (ncol / 4) + 255) / 256);
#define VL2_SKR(SW, F32) do { if (row_scale) hipLaunchKernelGGL((skinny_reduce_kernel<SW, F32, true>), g, b, 0, s, r); \
                              else hipLaunchKernelGGL((skinny_reduce_kernel<SW, F32, false>), g, b, 0, s, r); } while (0)
    if (sw) VL2_SKR(true, false); else if (f32) VL2_SKR(false, true); else VL2_SKR(false, false);
#undef VL2_SKR
    return launched(who);
}
#define VL2_SKINNY_ROWS(KERN, ARGS) skinny_rows<KERN<1>, KERN<2>, KERN<4>, ARGS>
extern "C" int32_t vl2_gemm_skinny_bf16(const void* A, const void* W, void* C, const float* bias, const void* res, int32_t M,
                                        int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldc, int32_t ldres, int32_t flags,
                                        void* ws, int64_t ws_bytes, void* stream) {
    if (!W) return fail(VL2_E_BADARG, "vl2_gemm_skinny_bf16: null pointer or empty shape");
    const bool ok = !(lda % 8 || ldw % 8 || ldc % 4 || (res && ldres % 4) || !ALIGNED16(A) || !ALIGNED16(W));
    return VL2_SKINNY_ROWS(gemm_skinny_kernel, SkinnyArgs)("vl2_gemm_skinny_bf16", SkinnyArgs{(const bf16_t*)A, (const bf16_t*)W, nullptr, M, N, K, lda, ldw, 0, 0},
                                                           ok, "16-byte aligned rows, lda%8==0, ldw%8==0, ldc%4==0, ldres%4==0", nullptr, true, C, bias, res,
                                                           ldc, ldres, flags, ws, ws_bytes, stream);
}
extern "C" int32_t vl2_gemm_skinny_fp8(const void* A, const void* q, const float* scale, void* C, const float* bias, const void* res, int32_t M,
                                       int32_t N, int32_t K, int32_t lda, int32_t ldq, int32_t ldc, int32_t ldres, int32_t flags, void* ws,
                                       int64_t ws_bytes, void* stream) {
    if (!q) return fail(VL2_E_BADARG, "vl2_gemm_skinny_fp8: null q (the e4m3fn weights)");
    if (!scale) return fail(VL2_E_BADARG, "vl2_gemm_skinny_fp8: null scale (the weights' row scales)");
    const bool ok = !(lda % 8 || lda < K || ldq % 16 || ldq < K || ldc % 4 || (res && ldres % 4) || !ALIGNED16(A) || !ALIGNED16(q));
    return VL2_SKINNY_ROWS(gemm_skinny_fp8_kernel, Skinny8Args)("vl2_gemm_skinny_fp8", Skinny8Args{(const bf16_t*)A, (const uint8_t*)q, nullptr, M, N, K, lda, ldq, 0, 0},
                                                                ok, "16-byte aligned rows, lda%8==0, ldq%16==0, ldc%4==0, ldres%4==0", scale, false, C, bias,
                                                                res, ldc, ldres, flags, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------------------------------------ norms
static int32_t launch_norm(const NormArgs& a, bool rms, hipStream_t s, const char* what) {
    if (!a.x || !a.y || !a.w || a.rows <= 0 || a.C <= 0) return fail(VL2_E_BADARG, "%s: null pointer or empty shape", what);
    if (a.C % 8 || a.C > 8192 || a.ldx % 8 || a.ldy % 8 || (a.res && a.ldres % 8))
        return fail(VL2_E_SHAPE, "%s: need C%%8==0, C<=8192, aligned strides (C=%d)", what, a.C);
    const int nv = (a.C + 511) / 512;
    dim3 g((a.rows + 3) / 4), b(256);
    if (rms && a.C > 2048) {     // long rows: the wide form (a workgroup per row), whatever the row count -- a row's result must
                                 // not depend on how many rows are normalised with it (batched prefill == one by one)
        if (a.C <= 4096) hipLaunchKernelGGL((norm_wide_kernel<true, 2>), dim3(a.rows), b, 0, s, a);
        else hipLaunchKernelGGL((norm_wide_kernel<true, 4>), dim3(a.rows), b, 0, s, a);
    } else if (rms) {
        if (nv <= 1) hipLaunchKernelGGL((norm_kernel<1, true>), g, b, 0, s, a);
        else if (nv <= 2) hipLaunchKernelGGL((norm_kernel<2, true>), g, b, 0, s, a);
        else hipLaunchKernelGGL((norm_kernel<8, true>), g, b, 0, s, a);
    } else {
        if (nv <= 1) hipLaunchKernelGGL((norm_kernel<1, false>), g, b, 0, s, a);
        else if (nv <= 2) hipLaunchKernelGGL((norm_kernel<2, false>), g, b, 0, s, a);
        else if (nv <= 3) hipLaunchKernelGGL((norm_kernel<3, false>), g, b, 0, s, a);      // SigLIP hidden 1152
        else if (nv <= 8) hipLaunchKernelGGL((norm_kernel<8, false>), g, b, 0, s, a);
        else hipLaunchKernelGGL((norm_kernel<16, false>), g, b, 0, s, a);                  // STC at the 72B decoder's width 8192
    }
    return launched(what);
}
extern "C" int32_t vl2_layernorm(const void* x, void* y, const float* w, const float* b, const void* res, int32_t rows,
                                 int32_t C, int32_t ldx, int32_t ldy, int32_t ldres, float eps, int32_t silu, void* stream) {
    NormArgs a{(const bf16_t*)x, (bf16_t*)y, w, b, (const bf16_t*)res, rows, C, ldx, ldy, ldres, eps, silu};
    return launch_norm(a, false, ST(stream), "vl2_layernorm");
}
extern "C" int32_t vl2_rmsnorm(const void* x, void* y, const float* w, int32_t rows, int32_t C, int32_t ldx, int32_t ldy,
                               float eps, void* stream) {
    NormArgs a{(const bf16_t*)x, (bf16_t*)y, w, nullptr, nullptr, rows, C, ldx, ldy, 0, eps, 0};
    return launch_norm(a, true, ST(stream), "vl2_rmsnorm");
}

// ------------------------------------------------------------------------------------------------ ViT front end
extern "C" int32_t vl2_patchify(const void* frames, int32_t dtype, void* out, int32_t T, int32_t H, int32_t W, int32_t P,
                                int32_t G, int32_t Kp, void* stream) {
    if (!frames || !out || T <= 0) return fail(VL2_E_BADARG, "vl2_patchify: null pointer or empty shape");
    if (G * P > H || G * P > W || Kp % 8 || Kp < 3 * P * P) return fail(VL2_E_SHAPE, "vl2_patchify: bad geometry");
    dim3 g(G, T), b(256);
    hipStream_t s = ST(stream);
    if (dtype == 0) hipLaunchKernelGGL((patchify_kernel<float>), g, b, 0, s, (const float*)frames, (bf16_t*)out, H, W, P, G, Kp);
    else if (dtype == 1) hipLaunchKernelGGL((patchify_kernel<_Float16>), g, b, 0, s, (const _Float16*)frames, (bf16_t*)out, H, W, P, G, Kp);
    else if (dtype == 2) hipLaunchKernelGGL((patchify_kernel<bf16_t>), g, b, 0, s, (const bf16_t*)frames, (bf16_t*)out, H, W, P, G, Kp);
    else return fail(VL2_E_UNSUPP, "vl2_patchify: dtype %d", dtype);
    return launched("vl2_patchify");
}
extern "C" int32_t vl2_patchify_u8(const void* frames_thwc, void* out, int32_t T, int32_t H, int32_t W, int32_t P, int32_t G, int32_t Kp,
                                   float rescale, float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b,
                                   void* stream) {
    if (!frames_thwc || !out || T <= 0 || std_r == 0.f || std_g == 0.f || std_b == 0.f) return fail(VL2_E_BADARG, "vl2_patchify_u8: null pointer, empty shape or zero std");
    if (G * P > H || G * P > W || Kp % 8 || Kp < 3 * P * P) return fail(VL2_E_SHAPE, "vl2_patchify_u8: bad geometry");
    U8Norm n{rescale, {mean_r, mean_g, mean_b}, {1.0f / std_r, 1.0f / std_g, 1.0f / std_b}};
    hipLaunchKernelGGL(patchify_u8_kernel, dim3(G, T), dim3(256), 0, ST(stream), (const unsigned char*)frames_thwc, (bf16_t*)out, H, W, P, G, Kp, n);
    return launched("vl2_patchify_u8");
}
extern "C" int32_t vl2_fill_cls(void* x, const void* cls_pos, int32_t T, int32_t D, int32_t rows_per_frame, void* stream) {
    if (!x || !cls_pos || T <= 0 || D % 8) return fail(VL2_E_BADARG, "vl2_fill_cls: bad args");
    hipLaunchKernelGGL(fill_cls_kernel, dim3(T), dim3(128), 0, ST(stream), (bf16_t*)x, (const bf16_t*)cls_pos, D, rows_per_frame);
    return launched("vl2_fill_cls");
}

// ------------------------------------------------------------------------------------------------ attention
extern "C" int32_t vl2_attn_fwd(const void* q, const void* k, const void* v, void* o, int64_t q_bs, int64_t q_hs, int32_t q_rs,
                                int64_t k_bs, int64_t k_hs, int32_t k_rs, int64_t v_bs, int64_t v_hs, int32_t v_rs,
                                int64_t o_bs, int64_t o_hs, int32_t o_rs, int32_t B, int32_t H, int32_t nq, int32_t nk,
                                int32_t group, float scale, int32_t causal, int32_t causal_off, int32_t D, int32_t variant,
                                void* stream) {
    if (!q || !k || !v || !o || B <= 0 || H <= 0 || nq <= 0 || nk <= 0 || group <= 0)
        return fail(VL2_E_BADARG, "vl2_attn_fwd: null pointer or empty shape");
    if ((q_rs | k_rs | v_rs | o_rs) % 8 || (q_bs | q_hs | k_bs | k_hs | v_bs | v_hs | o_bs | o_hs) % 4 || !ALIGNED16(q) ||
        !ALIGNED16(k) || !ALIGNED16(v) || ((uintptr_t)o & 7))
        return fail(VL2_E_SHAPE, "vl2_attn_fwd: strides must keep 16-byte row alignment");
    if (causal && causal_off < 0) return fail(VL2_E_SHAPE, "vl2_attn_fwd: causal_off must be >= 0");
    if (variant < 0 || variant > 5) return fail(VL2_E_BADARG, "vl2_attn_fwd: unknown variant %d", variant);
    const bool cls_shape = D == 64 && !causal && nq == nk && nk > 64 && (nk - 1) % 64 == 0 && group == 1;
    if (variant == 5 && (!kLab || !((D == 128 && causal) || cls_shape)))
        return fail(VL2_E_UNSUPP, "vl2_attn_fwd: variant 5 (the default kernels without round 6's scheduling changes) is a lab form of the causal head_dim 128 and class-token kernels: libvl2hip_lab.so only");
    // auto: the LDS-DMA / transpose-read structure wherever it is built (measured on MI355X, profiles/r02_attn_ab_*.jsonl:
    // causal D=128 S=945 / 1621 / 2973: 23.3 / 38.1 / 97.7 us vs 26.3 / 43.8 / 106.1 us; ViT D=64 T=8 / 16 / 32: 25.4 / 43.0 / 78.5 vs
    // 26.9 / 43.8 / 78.1 us); head_dim 96 (SigLIP's padded 72) stays on the register-staged kernel
    // full attention over [class token | 64 n patch tokens] (the CLIP tower: 577 = 1 + 576): the class token is peeled off the tiling
    // (k_attn2.h CLS = true: nine key tiles instead of ten, no dead query rows) -- automatic choice only, variant 3 keeps the plain tiling
    const bool cls_peel = variant == 0 && D == 64 && !causal && nq == nk && nk > 64 && (nk - 1) % 64 == 0 && group == 1;
    const bool cls_peel4 = variant == 4 && D == 64 && !causal && nq == nk && nk > 64 && (nk - 1) % 64 == 0 && group == 1;
    // causal head_dim 128 (the decoders' prefill): two key streams per query block (k_attn2.h NS = 2) while a SEQUENCE has at most 352 (query block, head)
    // pairs -- the longest query block's chain of dependent tiles is the launch's makespan there, and two streams halve it.  Decided per sequence (B is left
    // out) so that a prompt gets the same bits prefilled alone or in a batch.  Measured (profiles/r06_attn_ns2_ab*.jsonl, one / two streams, us): S = 512
    // 15.7 / 14.8, 945 23.5 / 21.2, 1152 28.7 / 25.2, 1408 33.1 / 30.6, 1452 x 28 heads 32.9 / 30.5, a 512-row chunk against 4096 keys 78.7 / 66.5;
    // beyond: S = 1621 (416 pairs) 37.4 / 41.1, 2973 92.2 / 102.5 -- one 128-KiB workgroup per CU balances worse than two of 64 KiB once the CUs hold
    // more than ~1.4 of them.  (The price of the per-sequence rule: a batch of short prompts, 2 x S = 945: 27.3 / 35.6.)  The ViT form stays on one stream
    // (T = 16: 40.8 / 42.8).
    if (variant == 0 && D == 128 && causal && (long)((nq + 127) / 128) * H <= 352) variant = 4;
    if (variant == 0 && (D == 64 || D == 128)) variant = 3;
    // K / V tiles are fetched through raw buffer resources whose byte offsets and NUM_RECORDS are 32-bit
    if (((int64_t)(nk - 1) * k_rs + D) * 2 >= (int64_t)1 << 31 || ((int64_t)(nk - 1) * v_rs + D) * 2 >= (int64_t)1 << 31)
        return fail(VL2_E_SHAPE, "vl2_attn_fwd: one head's K or V rows span >= 2 GiB (nk %d, row strides %d / %d elements)", nk, k_rs, v_rs);
    AttnArgs a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, q_bs, q_hs, q_rs, k_bs, k_hs, k_rs,
               v_bs, v_hs, v_rs, o_bs, o_hs, o_rs, nq, nk, group, H, B, scale * 1.4426950408889634f, causal_off};
    dim3 g((nq + 127) / 128, H, B), b(256);
    if (causal) g = dim3(((nq + 127) / 128) * H * B, 1, 1);
    hipStream_t s = ST(stream);
    if (variant == 4) {                                   // k_attn2.h with two key streams per query block (NS = 2): 512 threads, four LDS stages
        if (D != 64 && D != 128) return fail(VL2_E_SHAPE, "vl2_attn_fwd: variant 4 is built for head_dim 64 and 128 (got %d)", D);
        const dim3 b2(512);
        const int lds_bytes = 4 * (2 * 64 * D * 2);
#define VL2_ATTN_NS2(KERN, GRID) launch<KERN>(GRID, b2, lds_bytes, s, a)
        if (cls_peel4) VL2_ATTN_NS2((attn2_fwd_kernel<64, false, true, 2>), dim3((nq - 1 + 127) / 128 + ((((nq - 1) & 127) == 0 || ((nq - 1) & 127) > 96) ? 1 : 0), H, B));
        else if (D == 64 && !causal) VL2_ATTN_NS2((attn2_fwd_kernel<64, false, false, 2>), g);
        else if (D == 64 && causal) VL2_ATTN_NS2((attn2_fwd_kernel<64, true, false, 2>), g);
        else if (D == 128 && !causal) VL2_ATTN_NS2((attn2_fwd_kernel<128, false, false, 2>), g);
        else VL2_ATTN_NS2((attn2_fwd_kernel<128, true, false, 2>), g);
#undef VL2_ATTN_NS2
        return launched("vl2_attn_fwd");
    }
#ifdef VL2_LAB
    if (variant == 5) {
        if (cls_shape) hipLaunchKernelGGL((attn2_fwd_kernel<64, false, true, 1, false>), dim3((nq - 1 + 127) / 128 + ((((nq - 1) & 127) == 0 || ((nq - 1) & 127) > 96) ? 1 : 0), H, B), b, 0, s, a);
        else hipLaunchKernelGGL((attn2_fwd_kernel<128, true, false, 1, false>), g, b, 0, s, a);
        return launched("vl2_attn_fwd");
    }
#endif
    if (variant == 3) {                                   // second structure (k_attn2.h): LDS-DMA ring + transpose reads
        if (cls_peel) hipLaunchKernelGGL((attn2_fwd_kernel<64, false, true>), dim3(H, B, (nq - 1 + 127) / 128 + ((((nq - 1) & 127) == 0 || ((nq - 1) & 127) > 96) ? 1 : 0)), b, 0, s, a);      // (query block = the slowest index: k_attn2.h)
        else if (D == 64 && !causal) hipLaunchKernelGGL((attn2_fwd_kernel<64, false>), g, b, 0, s, a);
        else if (D == 64 && causal) hipLaunchKernelGGL((attn2_fwd_kernel<64, true>), g, b, 0, s, a);
        else if (D == 128 && !causal) hipLaunchKernelGGL((attn2_fwd_kernel<128, false>), g, b, 0, s, a);
        else if (D == 128 && causal) hipLaunchKernelGGL((attn2_fwd_kernel<128, true>), g, b, 0, s, a);
        else return fail(VL2_E_SHAPE, "vl2_attn_fwd: variant 3 is built for head_dim 64 and 128 (got %d)", D);
        return launched("vl2_attn_fwd");
    }
    if (D == 64 && !causal) hipLaunchKernelGGL((attn_fwd_kernel<64, false>), g, b, 0, s, a);
    else if (D == 64 && causal) hipLaunchKernelGGL((attn_fwd_kernel<64, true>), g, b, 0, s, a);
    else if (D == 128 && !causal) hipLaunchKernelGGL((attn_fwd_kernel<128, false>), g, b, 0, s, a);
    else if (D == 128 && causal) {
        // two KV groups per workgroup when a sequence has few (q block, head) pairs: decided per SEQUENCE (B is left out) so
        // that a prompt gets the same bits prefilled alone or in a batch.  Measured (scripts/attn_bench.py): 256 pairs (S = 945,
        // 32 heads) 28.5 -> 27.1 us, 336 (S = 1452, 28 heads) 38.9 -> 35.8; 416 (S = 1621, 32 heads) 47.4 -> 52.2: the SIMD's
        // per-tile throughput, not the length of the dependent tile chain, is the limit once every CU has > 1.4 workgroups.
        const long per_seq = (long)((nq + 127) / 128) * H;
        const bool two = variant == 2 || (variant == 0 && per_seq <= 352);
        if (two) hipLaunchKernelGGL((attn_fwd_kernel<128, true, 2>), g, dim3(512), 0, s, a);
        else hipLaunchKernelGGL((attn_fwd_kernel<128, true>), g, b, 0, s, a);
    }
    else if (D == 96 && !causal) hipLaunchKernelGGL((attn_fwd_kernel<96, false>), g, b, 0, s, a);
    else return fail(VL2_E_SHAPE, "vl2_attn_fwd: head_dim %d not built (64, 96 non-causal, 128)", D);
    return launched("vl2_attn_fwd");
}

// ------------------------------------------------------------------------------------------------ STC direct kernels
extern "C" int32_t vl2_dwconv3x3_ln_silu(const void* x, void* y, const float* w9c, const float* lnw, const float* lnb, int32_t F,
                                         int32_t H, int32_t W, int32_t C, float eps, void* stream) {
    if (!x || !y || !w9c || !lnw || !lnb || F <= 0 || H <= 0 || W <= 0) return fail(VL2_E_BADARG, "vl2_dwconv3x3_ln_silu: bad args");
    if (C % 8 || C > 8192) return fail(VL2_E_SHAPE, "vl2_dwconv3x3_ln_silu: need C%%8==0 and C<=8192");
    dim3 g(F * H * W), b(256);
    if (W >= 16) {         // wide rows: four positions per workgroup (k_stc.h); the choice depends on W alone
        dim3 g4(F * H * ((W + DW_P - 1) / DW_P));
        if (C <= 2048) hipLaunchKernelGGL((dwconv4_ln_silu_kernel<1>), g4, b, 0, ST(stream), (const bf16_t*)x, (bf16_t*)y, w9c, lnw, lnb, H, W, C, eps);
        else if (C <= 4096) hipLaunchKernelGGL((dwconv4_ln_silu_kernel<2>), g4, b, 0, ST(stream), (const bf16_t*)x, (bf16_t*)y, w9c, lnw, lnb, H, W, C, eps);
        else hipLaunchKernelGGL((dwconv4_ln_silu_kernel<4>), g4, b, 0, ST(stream), (const bf16_t*)x, (bf16_t*)y, w9c, lnw, lnb, H, W, C, eps);
        return launched("vl2_dwconv3x3_ln_silu");
    }
    if (C <= 2048) hipLaunchKernelGGL((dwconv_ln_silu_kernel<1>), g, b, 0, ST(stream), (const bf16_t*)x, (bf16_t*)y, w9c, lnw, lnb, H, W, C, eps);
    else if (C <= 4096) hipLaunchKernelGGL((dwconv_ln_silu_kernel<2>), g, b, 0, ST(stream), (const bf16_t*)x, (bf16_t*)y, w9c, lnw, lnb, H, W, C, eps);
    else hipLaunchKernelGGL((dwconv_ln_silu_kernel<4>), g, b, 0, ST(stream), (const bf16_t*)x, (bf16_t*)y, w9c, lnw, lnb, H, W, C, eps);
    return launched("vl2_dwconv3x3_ln_silu");
}
// strip form (k_stc.h): TPF teams per frame, a function of the grid (H, W) alone so that a frame's partial-sum grouping never depends on F
#define DWS_TPF_MAX 96
static inline int dws_tpf(int H, int W) {
    const int U = H * ((W + DWS_P - 1) / DWS_P);
    return U <= DWS_TPF_MAX ? U : (U + (U + 63) / 64 - 1) / ((U + 63) / 64);
}
template <int NVT>
static void launch_dwconv_strip(const void* x, void* y, const float* w9c, const float* lnw, const float* lnb, float* psum, int F, int H, int W, int C,
                                float eps, hipStream_t s) {
    const int U = H * ((W + DWS_P - 1) / DWS_P), tpf = dws_tpf(H, W), iters = (U + tpf - 1) / tpf;
    const size_t lds = (size_t)9 * C * 2;
    launch<dwconv_strip_ln_silu_kernel<NVT>>(dim3((F * tpf + 1) / 2), dim3(512), (int)lds, s, (const bf16_t*)x, (bf16_t*)y, w9c, lnw, lnb, psum,
                                             F, H, W, C, eps, tpf, iters);
}
extern "C" int64_t vl2_dwconv_mean_workspace_bytes(int32_t F, int32_t C) {
    if (F <= 0 || C <= 0) return -1;
    return (int64_t)F * DWS_TPF_MAX * C * 4;
}
extern "C" int32_t vl2_dwconv3x3_ln_silu_mean(const void* x, void* y, const float* w9c, const float* lnw, const float* lnb, int32_t F, int32_t H,
                                              int32_t W, int32_t C, float eps, float* mean, void* ws, int64_t ws_bytes, void* stream) {
    if (!x || !y || !w9c || !lnw || !lnb || F <= 0 || H <= 0 || W <= 0) return fail(VL2_E_BADARG, "vl2_dwconv3x3_ln_silu_mean: bad args");
    if (C % 8 || C > 8192) return fail(VL2_E_SHAPE, "vl2_dwconv3x3_ln_silu_mean: need C%%8==0 and C<=8192");
    const int tpf = dws_tpf(H, W);
    if (mean && (!ws || !ALIGNED16(ws) || ws_bytes < (int64_t)F * tpf * C * 4))
        return fail(VL2_E_BADARG, "vl2_dwconv3x3_ln_silu_mean: workspace missing, unaligned or < %lld bytes", (long long)F * tpf * C * 4);
    float* psum = mean ? (float*)ws : nullptr;
    if (C <= 2048) launch_dwconv_strip<1>(x, y, w9c, lnw, lnb, psum, F, H, W, C, eps, ST(stream));
    else if (C <= 4096) launch_dwconv_strip<2>(x, y, w9c, lnw, lnb, psum, F, H, W, C, eps, ST(stream));
    else launch_dwconv_strip<4>(x, y, w9c, lnw, lnb, psum, F, H, W, C, eps, ST(stream));
    if (mean)
        hipLaunchKernelGGL(chan_psum_finish_kernel, dim3((C + 255) / 256, F), dim3(256), 0, ST(stream), (const float*)psum, mean, tpf, C, 1.0f / (float)(H * W));
    return launched("vl2_dwconv3x3_ln_silu_mean");
}
extern "C" int32_t vl2_se_excite_scale(void* x, const float* g1, const void* W2, const float* b2, int32_t F, int32_t HW, int32_t C, int32_t rd,
                                       void* stream) {
    if (!x || !g1 || !W2 || F <= 0 || HW <= 0 || C <= 0 || rd <= 0) return fail(VL2_E_BADARG, "vl2_se_excite_scale: bad args");
    if (C % 8 || rd % 16) return fail(VL2_E_SHAPE, "vl2_se_excite_scale: need C%%8==0 and rd%%16==0 (C=%d rd=%d)", C, rd);
    hipLaunchKernelGGL(se_excite_scale_kernel, dim3((C + 127) / 128, F), dim3(256), 0, ST(stream), (bf16_t*)x, g1, (const bf16_t*)W2, b2, HW, C, rd);
    return launched("vl2_se_excite_scale");
}
extern "C" int32_t vl2_chan_mean(const void* x, float* mean, int32_t F, int32_t HW, int32_t C, void* stream) {
    if (!x || !mean || F <= 0 || HW <= 0) return fail(VL2_E_BADARG, "vl2_chan_mean: bad args");
    if (C % 64) return fail(VL2_E_SHAPE, "vl2_chan_mean: need C%%64==0");
    hipLaunchKernelGGL(chan_mean_kernel, dim3(C / 64, F), dim3(256), 0, ST(stream), (const bf16_t*)x, mean, HW, C);
    return launched("vl2_chan_mean");
}
extern "C" int32_t vl2_small_linear(const float* x, const void* W, const float* b, float* out, int32_t F, int32_t N, int32_t K,
                                    int32_t act, void* stream) {
    if (!x || !W || !out || F <= 0 || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_small_linear: bad args");
    if (K % 8) return fail(VL2_E_SHAPE, "vl2_small_linear: need K%%8==0");
    const int a = act == VL2_ACT_SILU ? 1 : act == VL2_ACT_SIGMOID ? 2 : act == VL2_ACT_NONE ? 0 : -1;
    if (a < 0) return fail(VL2_E_UNSUPP, "vl2_small_linear: act %d", act);
    hipLaunchKernelGGL(small_linear_kernel, dim3((N + SL_NB - 1) / SL_NB, (F + 7) / 8), dim3(256), 0, ST(stream), x, (const bf16_t*)W, b, out, F, N, K, a);
    return launched("vl2_small_linear");
}
extern "C" int32_t vl2_se_scale(void* x, const float* gate, int32_t F, int32_t HW, int32_t C, void* stream) {
    if (!x || !gate || F <= 0 || HW <= 0 || C % 8) return fail(VL2_E_BADARG, "vl2_se_scale: bad args");
    const size_t nvec = (size_t)F * HW * C / 8;
    size_t blocks = (nvec + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(se_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, ST(stream), (bf16_t*)x, gate, HW, C, nvec);
    return launched("vl2_se_scale");
}

// ------------------------------------------------------------------------------------------------ one-time weight re-layout
extern "C" int32_t vl2_pack_fold_norm(const void* W, const void* g, const void* beta, const void* bias, void* Wp, float* colsum, float* shift,
                                      int32_t N, int32_t K, int32_t ldw, void* stream) {
    if (!W || !g || !Wp || !colsum || N <= 0 || K <= 0 || ldw < K) return fail(VL2_E_BADARG, "vl2_pack_fold_norm: bad args");
    if ((beta != nullptr) != (shift != nullptr)) return fail(VL2_E_BADARG, "vl2_pack_fold_norm: beta and shift go together");
    if (bias && !beta) return fail(VL2_E_BADARG, "vl2_pack_fold_norm: a bias without a norm shift needs no folding");
    hipLaunchKernelGGL(pack_fold_norm_kernel, dim3((N + 3) / 4), dim3(256), 0, ST(stream), (const bf16_t*)W, (const bf16_t*)g, (const bf16_t*)beta,
                       (const bf16_t*)bias, (bf16_t*)Wp, colsum, shift, N, K, ldw);
    return launched("vl2_pack_fold_norm");
}
extern "C" int32_t vl2_pack_gate_up(const void* gate, const void* up, void* out, int32_t I, int32_t D, void* stream) {
    if (!gate || !up || !out || I <= 0 || D <= 0) return fail(VL2_E_BADARG, "vl2_pack_gate_up: bad args");
    if (I % 32 || D % 8) return fail(VL2_E_SHAPE, "vl2_pack_gate_up: need I%%32==0 and D%%8==0");
    hipLaunchKernelGGL(pack_gate_up_kernel, dim3(2 * I), dim3(128), 0, ST(stream), (const bf16_t*)gate, (const bf16_t*)up, (bf16_t*)out, D);
    return launched("vl2_pack_gate_up");
}
extern "C" int32_t vl2_pack_permute(const void* in, void* out, int32_t A, int32_t B, int32_t C, int32_t out_f32, void* stream) {
    if (!in || !out || A <= 0 || B <= 0 || C <= 0 || A > 65535) return fail(VL2_E_BADARG, "vl2_pack_permute: bad args");
    if ((int64_t)B * C > 0x7fffffffLL) return fail(VL2_E_SHAPE, "vl2_pack_permute: plane too large");
    const dim3 grid((unsigned)(((int64_t)B * C + 255) / 256), A);
    if (out_f32) hipLaunchKernelGGL((pack_permute_kernel<true>), grid, dim3(256), 0, ST(stream), (const bf16_t*)in, out, B, C);
    else hipLaunchKernelGGL((pack_permute_kernel<false>), grid, dim3(256), 0, ST(stream), (const bf16_t*)in, out, B, C);
    return launched("vl2_pack_permute");
}
extern "C" int32_t vl2_pack_pad_rows(const void* in, void* out, int64_t rows, int64_t cols_src, int64_t cols_dst, void* stream) {
    if (!in || !out || rows <= 0 || cols_src <= 0 || cols_dst < cols_src || rows > 0x7fffffffLL) return fail(VL2_E_BADARG, "vl2_pack_pad_rows: bad args");
    hipLaunchKernelGGL(pack_pad_rows_kernel, dim3((unsigned)rows), dim3(256), 0, ST(stream), (const bf16_t*)in, (bf16_t*)out, (long)cols_src, (long)cols_dst);
    return launched("vl2_pack_pad_rows");
}
extern "C" int32_t vl2_pack_cvt_f32(const void* in, float* out, int64_t n, void* stream) {
    if (!in || !out || n <= 0) return fail(VL2_E_BADARG, "vl2_pack_cvt_f32: bad args");
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_cvt_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, ST(stream), (const bf16_t*)in, out, (long)n);
    return launched("vl2_pack_cvt_f32");
}

// ------------------------------------------------------------------------------------------------ decoder glue / decode
extern "C" int32_t vl2_rope_kv(const void* qkv, void* q_out, void* kcache, void* vcache, const float* cos_t, const float* sin_t,
                               int32_t S, int32_t nh, int32_t nkv, int32_t smax, int32_t pos0, void* stream) {
    if (!qkv || !q_out || !kcache || !vcache || !cos_t || !sin_t || S <= 0) return fail(VL2_E_BADARG, "vl2_rope_kv: bad args");
    if (pos0 < 0 || pos0 + S > smax) return fail(VL2_E_SHAPE, "vl2_rope_kv: positions %d..%d exceed the cache (%d)", pos0, pos0 + S, smax);
    const size_t total = (size_t)S * (nh + 2 * nkv) * 8;
    size_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(rope_kv_kernel, dim3((unsigned)blocks), dim3(256), 0, ST(stream), (const bf16_t*)qkv, (bf16_t*)q_out,
                       (bf16_t*)kcache, (bf16_t*)vcache, cos_t, sin_t, S, nh, nkv, smax, pos0);
    return launched("vl2_rope_kv");
}

template <bool SW, bool F32>
static void launch_gemv(const GemvArgs& a, int n_out, hipStream_t s) {
    // one output row per wave: measured on MI355X 3.09 / 3.30 / 3.97 ms per 7B decode token at 1 / 2 / 4 rows per wave
    // norm-carrying single-pass rows (q/k/v, lm_head): x requested before the weight row (k_decode.h gemv_xfirst_bf16_kernel, same bits)
    if constexpr (!SW) {
        if ((a.norm_w || a.rms_plain) && a.K <= 4096) {
            hipLaunchKernelGGL((gemv_xfirst_bf16_kernel<false, F32, 2>), dim3((n_out + 3) / 4), dim3(256), (size_t)a.K * 2, s, a);
            return;
        }
    }
    hipLaunchKernelGGL((gemv_bf16_kernel<SW, F32, 1>), dim3((n_out + 3) / 4), dim3(256), (size_t)a.K * 2, s, a);
}
extern "C" int32_t vl2_gemv_bf16(const void* W, const void* x, const float* norm_w, const void* res, const float* bias, void* y,
                                 int32_t N, int32_t K, int32_t ldw, float eps, int32_t flags, void* stream) {
    if (!W || !x || !y || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_gemv_bf16: bad args");
    if (K % 8 || ldw % 8 || K > 32704) return fail(VL2_E_SHAPE, "vl2_gemv_bf16: need K%%8==0, K<=32704 (x lives in LDS; K=%d)", K);
    const bool sw = flags & VL2_GEMM_SWIGLU, f32 = flags & VL2_GEMM_OUT_F32;
    if (sw && (N % 64 || f32 || bias)) return fail(VL2_E_SHAPE, "vl2_gemv_bf16: SWIGLU needs N%%64==0, bf16 output, no bias");
    GemvArgs a{(const bf16_t*)W, (const bf16_t*)x, norm_w, (const bf16_t*)res, y, N, K, ldw, eps, bias, 0, 0, 0, 0};
    if (flags & VL2_GEMV_RMS_PLAIN) { a.norm_w = nullptr; a.rms_plain = 1; }
    if (sw) launch_gemv<true, false>(a, N / 2, ST(stream));
    else if (f32) launch_gemv<false, true>(a, N, ST(stream));
    else launch_gemv<false, false>(a, N, ST(stream));
    return launched("vl2_gemv_bf16");
}
extern "C" int32_t vl2_pack_quant_fp8(const void* w, int64_t N, int64_t K, int64_t ldw, void* q, float* scale, void* stream) {
    if (!w || !q || !scale || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_pack_quant_fp8: bad args");
    if (K % 16 || ldw % 8 || ldw < K || N > 0x7fffffff || K > 0x7fffffff) return fail(VL2_E_SHAPE, "vl2_pack_quant_fp8: need K%%16==0, ldw%%8==0, ldw>=K");
    hipLaunchKernelGGL(quant_fp8_rows_kernel, dim3((unsigned)N), dim3(256), 0, ST(stream), (const bf16_t*)w, (uint8_t*)q, scale, (int)K, (long)ldw);
    return launched("vl2_pack_quant_fp8");
}
extern "C" int32_t vl2_quant_act_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* row_tab, int32_t M, int32_t K, int32_t norm, float eps, void* stream) {
    if (!x || !q || !row_tab || M <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_quant_act_fp8: bad args");
    if (norm != VL2_NORM_NONE && norm != VL2_NORM_RMS) return fail(VL2_E_BADARG, "vl2_quant_act_fp8: norm must be none or RMS");
    if (K % 16 || ldx % 8 || ldq % 16 || ldx < K || ldq < K || !ALIGNED16(x) || !ALIGNED16(q) || (((uintptr_t)row_tab) & 7))
        return fail(VL2_E_SHAPE, "vl2_quant_act_fp8: need K%%16==0, 16-byte aligned rows");
    hipLaunchKernelGGL(quant_act_fp8_kernel, dim3((unsigned)M), dim3(256), 0, ST(stream), (const bf16_t*)x, (long)ldx, (uint8_t*)q, (long)ldq, row_tab, K,
                       norm == VL2_NORM_RMS ? 1 : 0, eps);
    return launched("vl2_quant_act_fp8");
}
template <bool SW, bool F32>
static void launch_gemv_mr(const GemvArgs& a, int mb, int n_out, hipStream_t s) {
    // two output rows per wave amortise staging the MB rows of x: measured at B = 4, 5.56 / 5.04 / 5.56 ms per step at 1 / 2 / 4
    constexpr int rpw = 2;
    const dim3 g((n_out + 4 * rpw - 1) / (4 * rpw)), b(256);
    const size_t lds = (size_t)mb * a.K * 2;
#define VL2_MR(MBV) hipLaunchKernelGGL((gemv_mr_bf16_kernel<SW, F32, MBV, 2>), g, b, lds, s, a)
    if (mb == 2) VL2_MR(2); else if (mb == 3) VL2_MR(3); else VL2_MR(4);
#undef VL2_MR
}
extern "C" int32_t vl2_gemv_batched_bf16(const void* W, const void* x, const float* norm_w, const void* res, const float* bias,
                                         void* y, int32_t MB, int32_t N, int32_t K, int32_t ldw, int32_t ldx, int32_t ldy,
                                         int32_t ldres, float eps, int32_t flags, void* stream) {
    if (!W || !x || !y || N <= 0 || K <= 0 || MB <= 0) return fail(VL2_E_BADARG, "vl2_gemv_batched_bf16: bad args");
    if (K % 8 || ldw % 8 || ldx % 8 || K > 32704) return fail(VL2_E_SHAPE, "vl2_gemv_batched_bf16: need K%%8==0, K<=32704 (K=%d)", K);
    const bool sw = flags & VL2_GEMM_SWIGLU, f32 = flags & VL2_GEMM_OUT_F32;
    if (sw && (N % 64 || f32 || bias)) return fail(VL2_E_SHAPE, "vl2_gemv_batched_bf16: SWIGLU needs N%%64==0, bf16 output, no bias");
    const int n_out = sw ? N / 2 : N;
    const int esz = f32 ? 4 : 2;
    const int cap = 65536 / (K * 2) < 4 ? 65536 / (K * 2) : 4;        // x rows that fit the 64 KiB of LDS, at most 4 per pass
    for (int b0 = 0; b0 < MB;) {
        const int mb = MB - b0 < cap ? MB - b0 : cap;
        GemvArgs a{(const bf16_t*)W, (const bf16_t*)x + (size_t)b0 * ldx, norm_w, res ? (const bf16_t*)res + (size_t)b0 * ldres : nullptr,
                   (char*)y + (size_t)b0 * ldy * esz, N, K, ldw, eps, bias, ldx, ldy, ldres};
        if (mb == 1) {
            if (sw) launch_gemv<true, false>(a, n_out, ST(stream));
            else if (f32) launch_gemv<false, true>(a, n_out, ST(stream));
            else launch_gemv<false, false>(a, n_out, ST(stream));
        } else {
            if (sw) launch_gemv_mr<true, false>(a, mb, n_out, ST(stream));
            else if (f32) launch_gemv_mr<false, true>(a, mb, n_out, ST(stream));
            else launch_gemv_mr<false, false>(a, mb, n_out, ST(stream));
        }
        b0 += mb;
    }
    return launched("vl2_gemv_batched_bf16");
}
// fp8 weights: rows of K <= 4096 are four 16-B vectors per lane: two pairs per wave and trip (NP = 2) keep the 16-bit kernel's bytes in flight
// (k_fp8.h); MB = 1 is gemv_fp8_kernel, MB = 2..4 gemv_mr_fp8_kernel -- one body
template <bool SW, bool F32>
static void launch_gemv_fp8_rows(const Gemv8Args& a, int mb, hipStream_t s) {
    const size_t lds = (size_t)mb * a.K * 2;
    const dim3 b(256);
#define VL2_G8(NP)                                                                                            \
    do {                                                                                                      \
        const dim3 g((unsigned)((a.N / 2 + 4 * NP - 1) / (4 * NP)));                                          \
        if (mb == 1) hipLaunchKernelGGL((gemv_fp8_kernel<SW, F32, NP>), g, b, lds, s, a);                     \
        else if (mb == 2) hipLaunchKernelGGL((gemv_mr_fp8_kernel<SW, F32, NP, 2>), g, b, lds, s, a);          \
        else if (mb == 3) hipLaunchKernelGGL((gemv_mr_fp8_kernel<SW, F32, NP, 3>), g, b, lds, s, a);          \
        else hipLaunchKernelGGL((gemv_mr_fp8_kernel<SW, F32, NP, 4>), g, b, lds, s, a);                       \
    } while (0)
    if (a.K <= 4096) VL2_G8(2); else VL2_G8(1);
#undef VL2_G8
}
// ONE host routine behind vl2_gemv_fp8 (MB = 1, the rows' strides their widths) and vl2_gemv_batched_fp8.  `mix` = the code of "SWIGLU with
// bias / f32 output", which the two entries have always reported differently.  Every check precedes every launch.
static int32_t gemv_fp8_rows(const char* who, int32_t mix, const void* q, const float* scale, const void* x, const float* norm_w, const void* res,
                             const float* bias, void* y, int32_t MB, int32_t N, int32_t K, int32_t ldq, int32_t ldx, int32_t ldy, int32_t ldres,
                             float eps, int32_t flags, void* stream) {
    if (!q) return fail(VL2_E_BADARG, "%s: null q (the e4m3fn weights)", who);
    if (!scale) return fail(VL2_E_BADARG, "%s: null scale (the weights' row scales)", who);
    if (!x || !y || N <= 0 || K <= 0 || MB <= 0) return fail(VL2_E_BADARG, "%s: null pointer or empty shape", who);
    if (K % 16 || K > 32704) return fail(VL2_E_SHAPE, "%s: need K%%16==0, K<=32704 (x lives in LDS as 16-bit elements; K=%d)", who, K);
    if (N % 2) return fail(VL2_E_SHAPE, "%s: need N even (N=%d)", who, N);
    const bool sw = flags & VL2_GEMM_SWIGLU, f32 = flags & VL2_GEMM_OUT_F32;
    const int n_out = sw ? N / 2 : N;
    if (ldq % 16 || ldq < K || ldx % 8 || ldx < K || ldy < n_out || (res && (ldres < n_out)) || !ALIGNED16(q) || !ALIGNED16(x))
        return fail(VL2_E_SHAPE, "%s: need 16-byte aligned rows, ldq%%16==0, ldq>=K, ldx%%8==0, ldx>=K, ldy / ldres >= the output width", who);
    if (sw && (bias || f32)) return fail(mix, "%s: SWIGLU excludes bias / f32 output", who);
    if (sw && N % 64) return fail(VL2_E_SHAPE, "%s: SWIGLU needs N%%64==0 (N=%d)", who, N);
    const int esz = f32 ? 4 : 2;
    const int cap = 65536 / (K * 2) < 4 ? 65536 / (K * 2) : 4;        // x rows that fit the 64 KiB of LDS, at most 4 per pass
    const bool plain = flags & VL2_GEMV_RMS_PLAIN;
    for (int b0 = 0; b0 < MB;) {
        const int mb = MB - b0 < cap ? MB - b0 : cap;
        Gemv8Args a{(const uint8_t*)q, scale, (const bf16_t*)x + (size_t)b0 * ldx, plain ? nullptr : norm_w,
                    res ? (const bf16_t*)res + (size_t)b0 * ldres : nullptr, (char*)y + (size_t)b0 * ldy * esz, N, K, ldq, eps, bias, plain ? 1 : 0,
                    ldx, ldy, ldres};
        if (sw) launch_gemv_fp8_rows<true, false>(a, mb, ST(stream));
        else if (f32) launch_gemv_fp8_rows<false, true>(a, mb, ST(stream));
        else launch_gemv_fp8_rows<false, false>(a, mb, ST(stream));
        b0 += mb;
    }
    return launched(who);
}
extern "C" int32_t vl2_gemv_fp8(const void* q, const float* scale, const void* x, const float* norm_w, const void* res, const float* bias, void* y,
                                int32_t N, int32_t K, int32_t ldq, float eps, int32_t flags, void* stream) {
    const int n_out = (flags & VL2_GEMM_SWIGLU) ? N / 2 : N;
    return gemv_fp8_rows("vl2_gemv_fp8", VL2_E_SHAPE, q, scale, x, norm_w, res, bias, y, 1, N, K, ldq, K, n_out, n_out, eps, flags, stream);
}
extern "C" int32_t vl2_gemv_batched_fp8(const void* q, const float* scale, const void* x, const float* norm_w, const void* res, const float* bias,
                                        void* y, int32_t MB, int32_t N, int32_t K, int32_t ldq, int32_t ldx, int32_t ldy, int32_t ldres, float eps,
                                        int32_t flags, void* stream) {
    return gemv_fp8_rows("vl2_gemv_batched_fp8", VL2_E_UNSUPP, q, scale, x, norm_w, res, bias, y, MB, N, K, ldq, ldx, ldy, ldres, eps, flags, stream);
}
// ---- MXFP4 weights (k_mxfp4.h): q [N, ldq] bytes of two E2M1 codes, s [N, lds] E8M0 bytes (one per 32 k).  Every check precedes every launch.
extern "C" int32_t vl2_pack_quant_mxfp4(const void* w, int64_t N, int64_t K, int64_t ldw, void* q, void* s, int64_t lds, void* stream) {
    if (!w) return fail(VL2_E_BADARG, "vl2_pack_quant_mxfp4: null w (the 16-bit weights)");
    if (!q) return fail(VL2_E_BADARG, "vl2_pack_quant_mxfp4: null q (the E2M1 codes)");
    if (!s) return fail(VL2_E_BADARG, "vl2_pack_quant_mxfp4: null scale (the E8M0 block scales)");
    if (N <= 0 || K <= 0 || N > 0x7fffffff || K > 0x7fffffff) return fail(VL2_E_BADARG, "vl2_pack_quant_mxfp4: empty or oversized shape");
    if (K % 32) return fail(VL2_E_SHAPE, "vl2_pack_quant_mxfp4: need K%%32==0 (one scale per block of 32; K=%lld)", (long long)K);
    if (ldw % 8 || ldw < K || lds < K / 32 || !ALIGNED16(w) || !ALIGNED16(q))
        return fail(VL2_E_SHAPE, "vl2_pack_quant_mxfp4: need 16-byte aligned rows, ldw%%8==0, ldw>=K, lds>=K/32");
    hipLaunchKernelGGL(quant_mxfp4_rows_kernel, dim3((unsigned)N), dim3(256), 0, ST(stream), (const bf16_t*)w, (uint8_t*)q, (uint8_t*)s, (int)K, (long)ldw,
                       (long)(K / 2), (long)lds);
    return launched("vl2_pack_quant_mxfp4");
}
// rows of K <= 4096 are two 16-B vectors per lane: four pairs per wave and trip keep 16 KiB per wave in flight (k_mxfp4.h); MB = 1 is
// gemv_mxfp4_kernel, MB = 2..4 gemv_mr_mxfp4_kernel -- one body
template <bool SW, bool F32>
static void launch_gemv_mxfp4_rows(const Gemv4Args& a, int mb, hipStream_t s) {
    const size_t lds = (size_t)mb * a.K * 2;
    const dim3 b(256);
#define VL2_G4(NP)                                                                                            \
    do {                                                                                                      \
        const dim3 g((unsigned)((a.N / 2 + 4 * NP - 1) / (4 * NP)));                                          \
        if (mb == 1) hipLaunchKernelGGL((gemv_mxfp4_kernel<SW, F32, NP>), g, b, lds, s, a);                   \
        else if (mb == 2) hipLaunchKernelGGL((gemv_mr_mxfp4_kernel<SW, F32, NP, 2>), g, b, lds, s, a);        \
        else if (mb == 3) hipLaunchKernelGGL((gemv_mr_mxfp4_kernel<SW, F32, NP, 3>), g, b, lds, s, a);        \
        else hipLaunchKernelGGL((gemv_mr_mxfp4_kernel<SW, F32, NP, 4>), g, b, lds, s, a);                     \
    } while (0)
    if (a.K <= 4096) VL2_G4(4); else VL2_G4(1);
#undef VL2_G4
}
static int32_t gemv_mxfp4_rows(const char* who, const void* q, const void* sc, int32_t lds, const void* x, const float* norm_w, const void* res,
                               const float* bias, void* y, int32_t MB, int32_t N, int32_t K, int32_t ldq, int32_t ldx, int32_t ldy, int32_t ldres,
                               float eps, int32_t flags, void* stream) {
    if (!q) return fail(VL2_E_BADARG, "%s: null q (the E2M1 codes)", who);
    if (!sc) return fail(VL2_E_BADARG, "%s: null scale (the E8M0 block scales)", who);
    if (!x || !y || N <= 0 || K <= 0 || MB <= 0) return fail(VL2_E_BADARG, "%s: null pointer or empty shape", who);
    if (K % 32) return fail(VL2_E_SHAPE, "%s: need K%%32==0 (one scale per block of 32; K=%d)", who, K);
    if (K > 32704) return fail(VL2_E_SHAPE, "%s: need K<=32704 (x lives in LDS as 16-bit elements; K=%d)", who, K);
    if (N % 2) return fail(VL2_E_SHAPE, "%s: need N even (N=%d)", who, N);
    const bool sw = flags & VL2_GEMM_SWIGLU, f32 = flags & VL2_GEMM_OUT_F32;
    const int n_out = sw ? N / 2 : N;
    if (ldq % 16 || ldq < K / 2 || lds < K / 32 || ldx % 8 || ldx < K || ldy < n_out || (res && (ldres < n_out)) || !ALIGNED16(q) || !ALIGNED16(x))
        return fail(VL2_E_SHAPE, "%s: need 16-byte aligned rows, ldq%%16==0, ldq>=K/2, lds>=K/32, ldx%%8==0, ldx>=K, ldy / ldres >= the output width", who);
    if (sw && (bias || f32)) return fail(VL2_E_UNSUPP, "%s: SWIGLU excludes bias / f32 output", who);
    if (sw && N % 64) return fail(VL2_E_SHAPE, "%s: SWIGLU needs N%%64==0 (N=%d)", who, N);
    const int esz = f32 ? 4 : 2;
    const int fit = (65536 - 64) / (K * 2), cap = fit < 4 ? fit : 4;  // x rows that fit the 64 KiB of LDS (beside the norm's 64 B), at most 4 per pass
    const bool plain = flags & VL2_GEMV_RMS_PLAIN;
    for (int b0 = 0; b0 < MB;) {
        const int mb = MB - b0 < cap ? MB - b0 : cap;
        Gemv4Args a{(const uint8_t*)q, (const uint8_t*)sc, (const bf16_t*)x + (size_t)b0 * ldx, plain ? nullptr : norm_w,
                    res ? (const bf16_t*)res + (size_t)b0 * ldres : nullptr, (char*)y + (size_t)b0 * ldy * esz, N, K, ldq, lds, eps, bias, plain ? 1 : 0,
                    ldx, ldy, ldres};
        if (sw) launch_gemv_mxfp4_rows<true, false>(a, mb, ST(stream));
        else if (f32) launch_gemv_mxfp4_rows<false, true>(a, mb, ST(stream));
        else launch_gemv_mxfp4_rows<false, false>(a, mb, ST(stream));
        b0 += mb;
    }
    return launched(who);
}
extern "C" int32_t vl2_gemv_mxfp4(const void* q, const void* scale, int32_t lds, const void* x, const float* norm_w, const void* res, const float* bias,
                                  void* y, int32_t N, int32_t K, int32_t ldq, float eps, int32_t flags, void* stream) {
    const int n_out = (flags & VL2_GEMM_SWIGLU) ? N / 2 : N;
    return gemv_mxfp4_rows("vl2_gemv_mxfp4", q, scale, lds, x, norm_w, res, bias, y, 1, N, K, ldq, K, n_out, n_out, eps, flags, stream);
}
extern "C" int32_t vl2_gemv_batched_mxfp4(const void* q, const void* scale, int32_t lds, const void* x, const float* norm_w, const void* res,
                                          const float* bias, void* y, int32_t MB, int32_t N, int32_t K, int32_t ldq, int32_t ldx, int32_t ldy,
                                          int32_t ldres, float eps, int32_t flags, void* stream) {
    return gemv_mxfp4_rows("vl2_gemv_batched_mxfp4", q, scale, lds, x, norm_w, res, bias, y, MB, N, K, ldq, ldx, ldy, ldres, eps, flags, stream);
}
// skinny-M on the MXFP4 weights (skinny_rows above): the block scales ride in the conversion, so the reduce is the unscaled one
extern "C" int32_t vl2_gemm_skinny_mxfp4(const void* A, const void* q, const void* scale, int32_t lds_, void* C, const float* bias, const void* res,
                                         int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldq, int32_t ldc, int32_t ldres, int32_t flags, void* ws,
                                         int64_t ws_bytes, void* stream) {
    if (!q) return fail(VL2_E_BADARG, "vl2_gemm_skinny_mxfp4: null q (the E2M1 codes)");
    if (!scale) return fail(VL2_E_BADARG, "vl2_gemm_skinny_mxfp4: null scale (the E8M0 block scales)");
    const bool ok = !(lda % 8 || lda < K || ldq % 16 || ldq < K / 2 || lds_ < K / 32 || ldc % 4 || (res && ldres % 4) || !ALIGNED16(A) || !ALIGNED16(q));
    return VL2_SKINNY_ROWS(gemm_skinny_mxfp4_kernel, Skinny4Args)(
        "vl2_gemm_skinny_mxfp4", Skinny4Args{(const bf16_t*)A, (const uint8_t*)q, (const uint8_t*)scale, nullptr, M, N, K, lda, ldq, lds_, 0, 0}, ok,
        "16-byte aligned rows, lda%8==0, ldq%16==0, ldq>=K/2, lds>=K/32, ldc%4==0, ldres%4==0", nullptr, false, C, bias, res, ldc, ldres, flags, ws, ws_bytes,
        stream);
}
extern "C" int32_t vl2_attn_decode(const void* qkv, void* kcache, void* vcache, const float* cos_t, const float* sin_t,
                                   float* partial, void* out, int32_t nh, int32_t nkv, int32_t smax, int32_t pos,
                                   const int32_t* pos_dev, int32_t ctx_cap, float scale, void* stream) {
    if (!qkv || !kcache || !vcache || !cos_t || !sin_t || !partial || !out || nh <= 0 || nkv <= 0)
        return fail(VL2_E_BADARG, "vl2_attn_decode: bad args");
    const int group = nh / nkv;
    if (group * nkv != nh) return fail(VL2_E_SHAPE, "vl2_attn_decode: need nh = nkv*group");
    const int cap = pos_dev ? ctx_cap : pos + 1;                 // positions the launch must be able to cover
    if (cap <= 0 || cap > smax || (!pos_dev && pos < 0)) return fail(VL2_E_SHAPE, "vl2_attn_decode: position %d outside the cache (%d)", cap - 1, smax);
    const int nsplit = (cap + 63) / 64;
    hipLaunchKernelGGL(attn_decode_kernel<false>, dim3(nsplit, nkv, (group + 3) / 4), dim3(256), 0, ST(stream), (const bf16_t*)qkv, (bf16_t*)kcache,
                       (bf16_t*)vcache, cos_t, sin_t, partial, nh, group, nkv, smax, pos, pos_dev, scale * 1.4426950408889634f, 0L, 0L, 0L,
                       (int*)nullptr, (bf16_t*)nullptr);
    hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(nh), dim3(128), 0, ST(stream), partial, (bf16_t*)out, nsplit, pos, pos_dev, 0L, 0L);
    return launched("vl2_attn_decode");
}
#ifdef VL2_LAB
// attention + combine of ONE decode token in one launch (k_decode.h attn_decode_kernel<true>): `cnt` = nkv int32 ticket counters,
// zero when the launch starts (vl2_llm_decode_step clears the counters of all layers in its argmax launch).  Same bits as
// vl2_attn_decode.  Measured 2.4 us per layer SLOWER than the two launches (profiles/r03_experiments.md section 5), so the stage-level
// decode step takes it only with VL2_STAGE_FUSED_DECODE_ATTN in the descriptor flags; exported as vl2_attn_decode_fused and kept under test.
static int32_t attn_decode_fused(const void* qkv, void* kcache, void* vcache, const float* cos_t, const float* sin_t, float* partial, void* out,
                                 int32_t nh, int32_t nkv, int32_t smax, const int32_t* pos_dev, float scale, int32_t* cnt, void* stream) {
    const int group = nh / nkv, nsplit = (smax + 63) / 64;
    hipLaunchKernelGGL(attn_decode_kernel<true>, dim3(nsplit, nkv, (group + 3) / 4), dim3(256), 0, ST(stream), (const bf16_t*)qkv, (bf16_t*)kcache,
                       (bf16_t*)vcache, cos_t, sin_t, partial, nh, group, nkv, smax, 0, pos_dev, scale * 1.4426950408889634f, 0L, 0L, 0L,
                       cnt, (bf16_t*)out);
    return launched("vl2_llm_decode_step (attention)");
}
extern "C" int32_t vl2_attn_decode_fused(const void* qkv, void* kcache, void* vcache, const float* cos_t, const float* sin_t, float* partial,
                                         void* out, int32_t nh, int32_t nkv, int32_t smax, const int32_t* pos_dev, float scale, int32_t* cnt,
                                         void* stream) {
    if (!qkv || !kcache || !vcache || !cos_t || !sin_t || !partial || !out || !pos_dev || !cnt || nh <= 0 || nkv <= 0 || smax <= 0 || nh % nkv)
        return fail(VL2_E_BADARG, "vl2_attn_decode_fused: bad args");
    return attn_decode_fused(qkv, kcache, vcache, cos_t, sin_t, partial, out, nh, nkv, smax, pos_dev, scale, cnt, stream);
}
#endif
extern "C" int32_t vl2_attn_decode_batched(const void* qkv, void* kcache, void* vcache, const float* cos_t, const float* sin_t,
                                           float* partial, void* out, int32_t B, int64_t qkv_bs, int64_t cache_bs, int64_t out_bs,
                                           int32_t nh, int32_t nkv, int32_t smax, const int32_t* pos_dev, int32_t ctx_cap, float scale,
                                           void* stream) {
    if (!qkv || !kcache || !vcache || !cos_t || !sin_t || !partial || !out || !pos_dev || nh <= 0 || nkv <= 0 || B <= 0)
        return fail(VL2_E_BADARG, "vl2_attn_decode_batched: bad args");
    const int group = nh / nkv;
    if (group * nkv != nh) return fail(VL2_E_SHAPE, "vl2_attn_decode_batched: need nh = nkv*group");
    if (ctx_cap <= 0 || ctx_cap > smax) return fail(VL2_E_SHAPE, "vl2_attn_decode_batched: ctx_cap %d outside the cache (%d)", ctx_cap, smax);
    const int nsplit = (ctx_cap + 63) / 64;
    const long partial_bs = (long)nh * nsplit * 130;
    hipLaunchKernelGGL(attn_decode_kernel<false>, dim3(nsplit, nkv * B, (group + 3) / 4), dim3(256), 0, ST(stream), (const bf16_t*)qkv,
                       (bf16_t*)kcache, (bf16_t*)vcache, cos_t, sin_t, partial, nh, group, nkv, smax, 0, pos_dev,
                       scale * 1.4426950408889634f, (long)qkv_bs, (long)cache_bs, partial_bs, (int*)nullptr, (bf16_t*)nullptr);
    hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(nh, B), dim3(128), 0, ST(stream), partial, (bf16_t*)out, nsplit, 0, pos_dev,
                       partial_bs, (long)out_bs);
    return launched("vl2_attn_decode_batched");
}
// ---- fp8 KV cache (k_kv8.h): the quantiser of cache rows and the decode attention on the quantised cache
extern "C" int32_t vl2_kv_quant(const void* k16, const void* v16, void* k8, void* v8, float* ks, float* vs, int32_t nkv, int32_t smax, int32_t p0,
                                int32_t p1, void* stream) {
    if (!k16 || !v16 || !k8 || !v8 || !ks || !vs || nkv <= 0 || smax <= 0) return fail(VL2_E_BADARG, "vl2_kv_quant: bad args");
    if (p0 < 0 || p1 <= p0 || p1 > smax) return fail(VL2_E_SHAPE, "vl2_kv_quant: rows [%d, %d) outside the cache (%d)", p0, p1, smax);
    if (!ALIGNED16(k16) || !ALIGNED16(v16) || !ALIGNED16(k8) || !ALIGNED16(v8)) return fail(VL2_E_SHAPE, "vl2_kv_quant: need 16-byte aligned caches");
    const long nrows = 2L * nkv * (p1 - p0);
    hipLaunchKernelGGL(kv_quant_rows_kernel, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, ST(stream), (const bf16_t*)k16, (const bf16_t*)v16,
                       (uint8_t*)k8, (uint8_t*)v8, ks, vs, nkv, smax, p0, p1);
    return launched("vl2_kv_quant");
}
static int32_t attn_decode_kv8(const char* who, const void* qkv, void* k8, void* v8, float* ks, float* vs, const float* cos_t, const float* sin_t,
                               float* partial, void* out, int B, long qkv_bs, long cache_bs, long scale_bs, long out_bs, int nh, int nkv, int smax,
                               int pos, const int32_t* pos_dev, int cap, float scale, void* stream) {
    if (!qkv || !k8 || !v8 || !ks || !vs || !cos_t || !sin_t || !partial || !out || nh <= 0 || nkv <= 0 || B <= 0)
        return fail(VL2_E_BADARG, "%s: bad args", who);
    const int group = nh / nkv;
    if (group * nkv != nh) return fail(VL2_E_SHAPE, "%s: need nh = nkv*group", who);
    if (cap <= 0 || cap > smax || (!pos_dev && pos < 0)) return fail(VL2_E_SHAPE, "%s: position %d outside the cache (%d)", who, cap - 1, smax);
    if (!ALIGNED16(k8) || !ALIGNED16(v8) || cache_bs % 16) return fail(VL2_E_SHAPE, "%s: need 16-byte aligned caches", who);
    const int nsplit = (cap + 63) / 64;
    const long partial_bs = (long)nh * nsplit * 130;
    hipLaunchKernelGGL(attn_decode_kv8_kernel, dim3(nsplit, nkv * B, (group + 3) / 4), dim3(256), 0, ST(stream), (const bf16_t*)qkv, (uint8_t*)k8,
                       (uint8_t*)v8, ks, vs, cos_t, sin_t, partial, nh, group, nkv, smax, pos, pos_dev, scale * 1.4426950408889634f, qkv_bs, cache_bs,
                       scale_bs, partial_bs);
    hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(nh, B), dim3(128), 0, ST(stream), partial, (bf16_t*)out, nsplit, pos, pos_dev, partial_bs, out_bs);
    return launched(who);
}
extern "C" int32_t vl2_attn_decode_kv8(const void* qkv, void* k8, void* v8, float* ks, float* vs, const float* cos_t, const float* sin_t, float* partial,
                                       void* out, int32_t nh, int32_t nkv, int32_t smax, int32_t pos, const int32_t* pos_dev, int32_t ctx_cap,
                                       float scale, void* stream) {
    return attn_decode_kv8("vl2_attn_decode_kv8", qkv, k8, v8, ks, vs, cos_t, sin_t, partial, out, 1, 0L, 0L, 0L, 0L, nh, nkv, smax, pos, pos_dev,
                           pos_dev ? ctx_cap : pos + 1, scale, stream);
}
extern "C" int32_t vl2_attn_decode_kv8_batched(const void* qkv, void* k8, void* v8, float* ks, float* vs, const float* cos_t, const float* sin_t,
                                               float* partial, void* out, int32_t B, int64_t qkv_bs, int64_t cache_bs, int64_t scale_bs, int64_t out_bs,
                                               int32_t nh, int32_t nkv, int32_t smax, const int32_t* pos_dev, int32_t ctx_cap, float scale,
                                               void* stream) {
    if (!pos_dev) return fail(VL2_E_BADARG, "vl2_attn_decode_kv8_batched: bad args (null pos_dev)");
    return attn_decode_kv8("vl2_attn_decode_kv8_batched", qkv, k8, v8, ks, vs, cos_t, sin_t, partial, out, B, (long)qkv_bs, (long)cache_bs,
                           (long)scale_bs, (long)out_bs, nh, nkv, smax, 0, pos_dev, ctx_cap, scale, stream);
}
// Split of the keys for vl2_attn_append: enough (kv head, row block, split) workgroups to fill the 256 CUs, at least two 64-key tiles per
// split (a split's fp32 partials cost about what one tile's loads do), at most APPEND_MAX_SPLITS.
static void attn_append_split(int P, int n, int group, int nkv, int& chunk, int& nsplit) {
    const int T = (P + n + 63) / 64, rb = (n * group + 127) / 128;
    int want = (256 + nkv * rb - 1) / (nkv * rb);
    want = want < (T + 1) / 2 ? want : (T + 1) / 2;
    want = want < APPEND_MAX_SPLITS ? want : APPEND_MAX_SPLITS;
    want = want > 1 ? want : 1;
    const int tps = (T + want - 1) / want;
    chunk = tps * 64;
    nsplit = (T + tps - 1) / tps;
}
extern "C" int64_t vl2_attn_append_ws_bytes(int32_t P, int32_t n, int32_t nh) {
    if (P < 0 || n <= 0 || nh <= 0) return 0;
    const int64_t T = (P + (int64_t)n + 63) / 64;
    return (int64_t)nh * n * (T < APPEND_MAX_SPLITS ? T : APPEND_MAX_SPLITS) * 130 * 4;
}
extern "C" int32_t vl2_attn_append(const void* q, int64_t q_rs, const void* kcache, const void* vcache, void* out, int64_t o_rs, int32_t P,
                                   int32_t n, int32_t nh, int32_t nkv, int32_t smax, float scale, float* ws, int64_t ws_bytes, void* stream) {
    if (!q || !kcache || !vcache || !out || !ws || n <= 0 || nh <= 0 || nkv <= 0 || smax <= 0 || P < 0)
        return fail(VL2_E_BADARG, "vl2_attn_append: null pointer or empty shape");
    if (nh % nkv) return fail(VL2_E_SHAPE, "vl2_attn_append: need nh = nkv*group");
    if ((int64_t)P + n > smax) return fail(VL2_E_SHAPE, "vl2_attn_append: rows %d..%d outside the cache (%d)", P, P + n - 1, smax);
    if (q_rs < (int64_t)nh * 128 || o_rs < (int64_t)nh * 128 || (q_rs & 7) || (o_rs & 7) || !ALIGNED16(q) || !ALIGNED16(kcache) || !ALIGNED16(vcache))
        return fail(VL2_E_SHAPE, "vl2_attn_append: rows must hold nh*128 elements at 16-byte alignment");
    if ((int64_t)smax * 128 * 2 >= (1ll << 31)) return fail(VL2_E_SHAPE, "vl2_attn_append: one head's cache spans >= 2 GiB");
    if (ws_bytes < vl2_attn_append_ws_bytes(P, n, nh))
        return fail(VL2_E_SHAPE, "vl2_attn_append: workspace of %lld bytes, need %lld", (long long)ws_bytes, (long long)vl2_attn_append_ws_bytes(P, n, nh));
    const int group = nh / nkv;
    int chunk, nsplit;
    attn_append_split(P, n, group, nkv, chunk, nsplit);
    AppendArgs a{(const bf16_t*)q, (long)q_rs, (const bf16_t*)kcache, (const bf16_t*)vcache, smax, P, n, nh, nkv, group, chunk, nsplit,
                 scale * 1.4426950408889634f, ws};
    hipLaunchKernelGGL(attn_append_kernel<false>, dim3(nsplit, nkv, (n * group + 127) / 128), dim3(256), 0, ST(stream), a);
    hipLaunchKernelGGL(attn_append_combine_kernel, dim3(nh, n), dim3(128), 0, ST(stream), (const float*)ws, (bf16_t*)out, (long)o_rs, n, P,
                       chunk, nsplit);
    return launched("vl2_attn_append");
}
// Split of the prefix keys for vl2_attn_decode_shared: a pure function of P (the partial layout and the order of a row's sums must not
// depend on the batch).  At least two 64-key tiles per split (as attn_append_split), at most 24 splits: with up to 8 own slices (512 own
// rows) the combine stays within COMBINE_EARLY = one memory round trip.
static void attn_shared_split(int P, int& chunk, int& nps) {
    const int T = (P + 63) / 64;
    int tps = (T + 23) / 24;
    tps = tps > 2 ? tps : 2;
    chunk = tps * 64;
    nps = (P + chunk - 1) / chunk;
}
extern "C" int64_t vl2_attn_decode_shared_partial_floats(int32_t P, int32_t own_cap, int32_t nh) {
    if (P <= 0 || own_cap <= 0 || own_cap % 64 || nh <= 0) return 0;
    int chunk, nps;
    attn_shared_split(P, chunk, nps);
    return (int64_t)nh * (nps + own_cap / 64) * 130;
}
extern "C" int32_t vl2_attn_decode_shared(const void* qkv, const void* kprefix, const void* vprefix, void* kown, void* vown, const float* cos_t,
                                          const float* sin_t, float* partial, int64_t partial_floats, void* out, int32_t B, int64_t qkv_bs,
                                          int64_t own_bs, int64_t out_bs, int32_t nh, int32_t nkv, int32_t P, int32_t prefix_smax, int32_t own_cap,
                                          int32_t rope_rows, const int32_t* pos_dev, float scale, void* stream) {
    if (!qkv || !kprefix || !vprefix || !kown || !vown || !cos_t || !sin_t || !partial || !out || !pos_dev || nh <= 0 || nkv <= 0 || B <= 0)
        return fail(VL2_E_BADARG, "vl2_attn_decode_shared: bad args");
    if (nh % nkv) return fail(VL2_E_SHAPE, "vl2_attn_decode_shared: need nh = nkv*group");
    if (P <= 0 || P > prefix_smax) return fail(VL2_E_SHAPE, "vl2_attn_decode_shared: prefix of %d rows outside the prefix cache (%d)", P, prefix_smax);
    if ((int64_t)prefix_smax * 128 * 2 >= (1ll << 31)) return fail(VL2_E_SHAPE, "vl2_attn_decode_shared: one head's prefix cache spans >= 2 GiB");
    if (own_cap <= 0 || own_cap % 64) return fail(VL2_E_SHAPE, "vl2_attn_decode_shared: own_cap %d must be a positive multiple of 64", own_cap);
    if ((int64_t)P + own_cap > rope_rows)
        return fail(VL2_E_SHAPE, "vl2_attn_decode_shared: positions up to %lld outside the cos/sin tables (%d rows)", (long long)P + own_cap - 1, rope_rows);
    if (qkv_bs < ((int64_t)nh + 2 * nkv) * 128 || (qkv_bs & 7) || out_bs < (int64_t)nh * 128 || own_bs < (int64_t)nkv * own_cap * 128 || (own_bs & 7) ||
        !ALIGNED16(qkv) || !ALIGNED16(kprefix) || !ALIGNED16(vprefix) || !ALIGNED16(kown) || !ALIGNED16(vown))
        return fail(VL2_E_SHAPE, "vl2_attn_decode_shared: rows must hold their heads' 128 elements at 16-byte alignment, a slot nkv*own_cap rows");
    const int64_t partial_bs = vl2_attn_decode_shared_partial_floats(P, own_cap, nh);
    if (partial_floats < partial_bs * B)
        return fail(VL2_E_SHAPE, "vl2_attn_decode_shared: partial of %lld floats, need %lld", (long long)partial_floats, (long long)(partial_bs * B));
    const int group = nh / nkv;
    if ((int64_t)nkv * B > 65535 || ((int64_t)B * group + 127) / 128 > 65535) return fail(VL2_E_SHAPE, "vl2_attn_decode_shared: too many requests (%d)", B);
    int chunk, nps;
    attn_shared_split(P, chunk, nps);
    const int nsplit_cap = nps + own_cap / 64;
    const float sl2 = scale * 1.4426950408889634f;
    SharedPrefixArgs a{};
    a.q = (const bf16_t*)qkv; a.q_rs = (long)qkv_bs; a.k = (const bf16_t*)kprefix; a.v = (const bf16_t*)vprefix;
    a.smax = prefix_smax; a.P = P; a.n = B; a.nh = nh; a.nkv = nkv; a.group = group; a.chunk = chunk; a.nsplit = nps;
    a.scale_log2e = sl2; a.ws = partial;
    a.pos_dev = pos_dev; a.cos_t = cos_t; a.sin_t = sin_t; a.own_cap = own_cap; a.nsplit_cap = nsplit_cap; a.partial_bs = (long)partial_bs;
    hipLaunchKernelGGL(attn_append_kernel<true>, dim3(nps, nkv, (B * group + 127) / 128), dim3(256), 0, ST(stream), a);
    hipLaunchKernelGGL(attn_decode_own_kernel, dim3(own_cap / 64, nkv * B, (group + 3) / 4), dim3(256), 0, ST(stream), (const bf16_t*)qkv,
                       (bf16_t*)kown, (bf16_t*)vown, cos_t, sin_t, partial, nh, group, nkv, own_cap, P, nps, nsplit_cap, pos_dev, sl2, (long)qkv_bs,
                       (long)own_bs, (long)partial_bs);
    hipLaunchKernelGGL(attn_shared_combine_kernel, dim3(nh, B), dim3(128), 0, ST(stream), (const float*)partial, (bf16_t*)out, P, nps, own_cap,
                       nsplit_cap, pos_dev, (long)partial_bs, (long)out_bs);
    return launched("vl2_attn_decode_shared");
}
// ---- paged KV cache (k_attn_paged.h): the batched decode attention on pages of 64 positions from one pool per layer, and the copy of a
// prefill's contiguous rows into a sequence's pages
extern "C" int32_t vl2_attn_decode_paged(const void* qkv, void* kpool, void* vpool, const int32_t* page_table, const float* cos_t, const float* sin_t,
                                         float* partial, void* out, int32_t B, int64_t qkv_bs, int32_t table_bs, int32_t n_pages, int64_t out_bs,
                                         int32_t nh, int32_t nkv, int32_t seq_cap, const int32_t* pos_dev, int32_t ctx_cap, float scale, void* stream) {
    if (!qkv || !kpool || !vpool || !page_table || !cos_t || !sin_t || !partial || !out || !pos_dev)
        return fail(VL2_E_BADARG, "vl2_attn_decode_paged: null pointer");
    if (nh <= 0 || nkv <= 0 || B <= 0) return fail(VL2_E_BADARG, "vl2_attn_decode_paged: need nh, nkv, B > 0 (got %d, %d, %d)", nh, nkv, B);
    if (nh % nkv) return fail(VL2_E_SHAPE, "vl2_attn_decode_paged: need nh = nkv*group");
    if (n_pages < 1) return fail(VL2_E_SHAPE, "vl2_attn_decode_paged: n_pages %d: the pool holds at least the parking page", n_pages);
    if (seq_cap <= 0 || seq_cap % 64) return fail(VL2_E_SHAPE, "vl2_attn_decode_paged: seq_cap %d must be a positive multiple of 64", seq_cap);
    if (table_bs <= 0 || seq_cap > 64 * (int64_t)table_bs)
        return fail(VL2_E_SHAPE, "vl2_attn_decode_paged: seq_cap %d outside a table row of %d pages", seq_cap, table_bs);
    if (ctx_cap <= 0 || ctx_cap > seq_cap) return fail(VL2_E_SHAPE, "vl2_attn_decode_paged: ctx_cap %d outside seq_cap (%d)", ctx_cap, seq_cap);
    if (!ALIGNED16(qkv) || !ALIGNED16(kpool) || !ALIGNED16(vpool) || (qkv_bs & 7))
        return fail(VL2_E_SHAPE, "vl2_attn_decode_paged: need 16-byte aligned qkv rows and pools");
    if ((int64_t)nkv * B > 65535) return fail(VL2_E_SHAPE, "vl2_attn_decode_paged: too many sequences (%d)", B);
    const int group = nh / nkv;
    const int nsplit = (ctx_cap + 63) / 64;
    const long partial_bs = (long)nh * nsplit * 130;
    hipLaunchKernelGGL(attn_decode_paged_kernel, dim3(nsplit, nkv * B, (group + 3) / 4), dim3(256), 0, ST(stream), (const bf16_t*)qkv,
                       (bf16_t*)kpool, (bf16_t*)vpool, (const int*)page_table, cos_t, sin_t, partial, nh, group, nkv, seq_cap, n_pages, table_bs,
                       pos_dev, scale * 1.4426950408889634f, (long)qkv_bs, partial_bs);
    hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(nh, B), dim3(128), 0, ST(stream), partial, (bf16_t*)out, nsplit, 0, pos_dev,
                       partial_bs, (long)out_bs);
    return launched("vl2_attn_decode_paged");
}
extern "C" int32_t vl2_kv_page_scatter(const void* k16, const void* v16, void* kpool, void* vpool, const int32_t* table_row, int32_t nkv, int32_t smax,
                                       int32_t n_pages, int32_t p0, int32_t p1, void* stream) {
    if (!k16 || !v16 || !kpool || !vpool || !table_row) return fail(VL2_E_BADARG, "vl2_kv_page_scatter: null pointer");
    if (nkv <= 0 || smax <= 0) return fail(VL2_E_BADARG, "vl2_kv_page_scatter: need nkv, smax > 0 (got %d, %d)", nkv, smax);
    if (n_pages < 1) return fail(VL2_E_SHAPE, "vl2_kv_page_scatter: n_pages %d: the pool holds at least the parking page", n_pages);
    if (p0 < 0 || p0 > p1 || p1 > smax) return fail(VL2_E_SHAPE, "vl2_kv_page_scatter: rows [%d, %d) outside the cache (%d)", p0, p1, smax);
    if (!ALIGNED16(k16) || !ALIGNED16(v16) || !ALIGNED16(kpool) || !ALIGNED16(vpool))
        return fail(VL2_E_SHAPE, "vl2_kv_page_scatter: need 16-byte aligned caches and pools");
    if (p0 == p1) return 0;
    const long nrows = 2L * nkv * (p1 - p0);
    hipLaunchKernelGGL(kv_page_scatter_kernel, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, ST(stream), (const bf16_t*)k16, (const bf16_t*)v16,
                       (bf16_t*)kpool, (bf16_t*)vpool, (const int*)table_row, nkv, smax, n_pages, p0, p1);
    return launched("vl2_kv_page_scatter");
}
// ---- shared prefix held once in the page pool (k_attn_paged_shared.h): vl2_attn_decode_shared's three launches through page lookups, and the
// copy of a sequence's pages back into contiguous caches
extern "C" int32_t vl2_attn_decode_shared_paged(const void* qkv, void* kpool, void* vpool, const int32_t* page_table, const int32_t* prefix_pages,
                                                const float* cos_t, const float* sin_t, float* partial, int64_t partial_floats, void* out, int32_t B,
                                                int64_t qkv_bs, int32_t table_bs, int32_t n_pages, int64_t out_bs, int32_t nh, int32_t nkv, int32_t P,
                                                int32_t own_cap, int32_t rope_rows, const int32_t* pos_dev, float scale, void* stream) {
    if (!qkv || !kpool || !vpool || !page_table || !prefix_pages || !cos_t || !sin_t || !partial || !out || !pos_dev)
        return fail(VL2_E_BADARG, "vl2_attn_decode_shared_paged: null pointer");
    if (nh <= 0 || nkv <= 0 || B <= 0) return fail(VL2_E_BADARG, "vl2_attn_decode_shared_paged: need nh, nkv, B > 0 (got %d, %d, %d)", nh, nkv, B);
    if (nh % nkv) return fail(VL2_E_SHAPE, "vl2_attn_decode_shared_paged: need nh = nkv*group");
    if (n_pages < 1) return fail(VL2_E_SHAPE, "vl2_attn_decode_shared_paged: n_pages %d: the pool holds at least the parking page", n_pages);
    if (P <= 0 || P % 64) return fail(VL2_E_SHAPE, "vl2_attn_decode_shared_paged: P %d must be a positive multiple of 64 (whole pages are shared)", P);
    if (own_cap <= 0 || own_cap % 64) return fail(VL2_E_SHAPE, "vl2_attn_decode_shared_paged: own_cap %d must be a positive multiple of 64", own_cap);
    if (table_bs <= 0 || (int64_t)P / 64 + own_cap / 64 > table_bs)
        return fail(VL2_E_SHAPE, "vl2_attn_decode_shared_paged: %d prefix pages + %d own pages outside a table row of %d pages", P / 64, own_cap / 64,
                    table_bs);
    if ((int64_t)P + own_cap > rope_rows)
        return fail(VL2_E_SHAPE, "vl2_attn_decode_shared_paged: positions up to %lld outside the cos/sin tables (%d rows)", (long long)P + own_cap - 1,
                    rope_rows);
    if (qkv_bs < ((int64_t)nh + 2 * nkv) * 128 || (qkv_bs & 7) || out_bs < (int64_t)nh * 128 || !ALIGNED16(qkv) || !ALIGNED16(kpool) || !ALIGNED16(vpool))
        return fail(VL2_E_SHAPE, "vl2_attn_decode_shared_paged: rows must hold their heads' 128 elements, qkv rows and pools at 16-byte alignment");
    const int64_t partial_bs = vl2_attn_decode_shared_partial_floats(P, own_cap, nh);
    if (partial_floats < partial_bs * B)
        return fail(VL2_E_SHAPE, "vl2_attn_decode_shared_paged: partial of %lld floats, need %lld", (long long)partial_floats, (long long)(partial_bs * B));
    const int group = nh / nkv;
    if ((int64_t)nkv * B > 65535 || ((int64_t)B * group + 127) / 128 > 65535)
        return fail(VL2_E_SHAPE, "vl2_attn_decode_shared_paged: too many requests (%d)", B);
    int chunk, nps;
    attn_shared_split(P, chunk, nps);
    const int nsplit_cap = nps + own_cap / 64;
    const float sl2 = scale * 1.4426950408889634f;
    SharedPrefixPagedArgs a{};
    a.q = (const bf16_t*)qkv; a.q_rs = (long)qkv_bs; a.k = (const bf16_t*)kpool; a.v = (const bf16_t*)vpool;
    a.smax = 0; a.P = P; a.n = B; a.nh = nh; a.nkv = nkv; a.group = group; a.chunk = chunk; a.nsplit = nps;
    a.scale_log2e = sl2; a.ws = partial;
    a.pos_dev = pos_dev; a.cos_t = cos_t; a.sin_t = sin_t; a.own_cap = own_cap; a.nsplit_cap = nsplit_cap; a.partial_bs = (long)partial_bs;
    a.prefix_pages = (const int*)prefix_pages; a.n_pages = n_pages;
    hipLaunchKernelGGL(attn_prefix_paged_kernel, dim3(nps, nkv, (B * group + 127) / 128), dim3(256), 0, ST(stream), a);
    hipLaunchKernelGGL(attn_decode_own_paged_kernel, dim3(own_cap / 64, nkv * B, (group + 3) / 4), dim3(256), 0, ST(stream), (const bf16_t*)qkv,
                       (bf16_t*)kpool, (bf16_t*)vpool, (const int*)page_table, cos_t, sin_t, partial, nh, group, nkv, own_cap, P, nps, nsplit_cap,
                       n_pages, table_bs, pos_dev, sl2, (long)qkv_bs, (long)partial_bs);
    hipLaunchKernelGGL(attn_shared_combine_kernel, dim3(nh, B), dim3(128), 0, ST(stream), (const float*)partial, (bf16_t*)out, P, nps, own_cap,
                       nsplit_cap, pos_dev, (long)partial_bs, (long)out_bs);
    return launched("vl2_attn_decode_shared_paged");
}
extern "C" int32_t vl2_kv_page_gather(const void* kpool, const void* vpool, void* k16, void* v16, const int32_t* table_row, int32_t nkv, int32_t smax,
                                      int32_t n_pages, int32_t p0, int32_t p1, void* stream) {
    if (!k16 || !v16 || !kpool || !vpool || !table_row) return fail(VL2_E_BADARG, "vl2_kv_page_gather: null pointer");
    if (nkv <= 0 || smax <= 0) return fail(VL2_E_BADARG, "vl2_kv_page_gather: need nkv, smax > 0 (got %d, %d)", nkv, smax);
    if (n_pages < 1) return fail(VL2_E_SHAPE, "vl2_kv_page_gather: n_pages %d: the pool holds at least the parking page", n_pages);
    if (p0 < 0 || p0 > p1 || p1 > smax) return fail(VL2_E_SHAPE, "vl2_kv_page_gather: rows [%d, %d) outside the cache (%d)", p0, p1, smax);
    if (!ALIGNED16(k16) || !ALIGNED16(v16) || !ALIGNED16(kpool) || !ALIGNED16(vpool))
        return fail(VL2_E_SHAPE, "vl2_kv_page_gather: need 16-byte aligned caches and pools");
    if (p0 == p1) return 0;
    const long nrows = 2L * nkv * (p1 - p0);
    hipLaunchKernelGGL(kv_page_gather_kernel, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, ST(stream), (const bf16_t*)kpool, (const bf16_t*)vpool,
                       (bf16_t*)k16, (bf16_t*)v16, (const int*)table_row, nkv, smax, n_pages, p0, p1);
    return launched("vl2_kv_page_gather");
}
// ---- paged KV cache in fp8 (k_attn_paged_kv8.h): vl2_attn_decode_paged and vl2_kv_page_scatter on pools of e4m3 codes and row scales
extern "C" int32_t vl2_attn_decode_kv8_paged(const void* qkv, void* k8pool, void* v8pool, float* kspool, float* vspool, const int32_t* page_table,
                                             const float* cos_t, const float* sin_t, float* partial, void* out, int32_t B, int64_t qkv_bs,
                                             int32_t table_bs, int32_t n_pages, int64_t out_bs, int32_t nh, int32_t nkv, int32_t seq_cap,
                                             const int32_t* pos_dev, int32_t ctx_cap, float scale, void* stream) {
    if (!qkv || !k8pool || !v8pool || !kspool || !vspool || !page_table || !cos_t || !sin_t || !partial || !out || !pos_dev)
        return fail(VL2_E_BADARG, "vl2_attn_decode_kv8_paged: null pointer");
    if (nh <= 0 || nkv <= 0 || B <= 0) return fail(VL2_E_BADARG, "vl2_attn_decode_kv8_paged: need nh, nkv, B > 0 (got %d, %d, %d)", nh, nkv, B);
    if (nh % nkv) return fail(VL2_E_SHAPE, "vl2_attn_decode_kv8_paged: need nh = nkv*group");
    if (n_pages < 1) return fail(VL2_E_SHAPE, "vl2_attn_decode_kv8_paged: n_pages %d: the pool holds at least the parking page", n_pages);
    if (seq_cap <= 0 || seq_cap % 64) return fail(VL2_E_SHAPE, "vl2_attn_decode_kv8_paged: seq_cap %d must be a positive multiple of 64", seq_cap);
    if (table_bs <= 0 || seq_cap > 64 * (int64_t)table_bs)
        return fail(VL2_E_SHAPE, "vl2_attn_decode_kv8_paged: seq_cap %d outside a table row of %d pages", seq_cap, table_bs);
    if (ctx_cap <= 0 || ctx_cap > seq_cap) return fail(VL2_E_SHAPE, "vl2_attn_decode_kv8_paged: ctx_cap %d outside seq_cap (%d)", ctx_cap, seq_cap);
    if (!ALIGNED16(qkv) || !ALIGNED16(k8pool) || !ALIGNED16(v8pool) || (qkv_bs & 7))
        return fail(VL2_E_SHAPE, "vl2_attn_decode_kv8_paged: need 16-byte aligned qkv rows and pools");
    if ((int64_t)nkv * B > 65535) return fail(VL2_E_SHAPE, "vl2_attn_decode_kv8_paged: too many sequences (%d)", B);
    const int group = nh / nkv;
    const int nsplit = (ctx_cap + 63) / 64;
    const long partial_bs = (long)nh * nsplit * 130;
    hipLaunchKernelGGL(attn_decode_kv8_paged_kernel, dim3(nsplit, nkv * B, (group + 3) / 4), dim3(256), 0, ST(stream), (const bf16_t*)qkv,
                       (uint8_t*)k8pool, (uint8_t*)v8pool, kspool, vspool, (const int*)page_table, cos_t, sin_t, partial, nh, group, nkv, seq_cap,
                       n_pages, table_bs, pos_dev, scale * 1.4426950408889634f, (long)qkv_bs, partial_bs);
    hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(nh, B), dim3(128), 0, ST(stream), partial, (bf16_t*)out, nsplit, 0, pos_dev,
                       partial_bs, (long)out_bs);
    return launched("vl2_attn_decode_kv8_paged");
}
extern "C" int32_t vl2_kv_page_quant(const void* k16, const void* v16, void* k8pool, void* v8pool, float* kspool, float* vspool,
                                     const int32_t* table_row, int32_t nkv, int32_t smax, int32_t n_pages, int32_t p0, int32_t p1, void* stream) {
    if (!k16 || !v16 || !k8pool || !v8pool || !kspool || !vspool || !table_row) return fail(VL2_E_BADARG, "vl2_kv_page_quant: null pointer");
    if (nkv <= 0 || smax <= 0) return fail(VL2_E_BADARG, "vl2_kv_page_quant: need nkv, smax > 0 (got %d, %d)", nkv, smax);
    if (n_pages < 1) return fail(VL2_E_SHAPE, "vl2_kv_page_quant: n_pages %d: the pool holds at least the parking page", n_pages);
    if (p0 < 0 || p0 > p1 || p1 > smax) return fail(VL2_E_SHAPE, "vl2_kv_page_quant: rows [%d, %d) outside the cache (%d)", p0, p1, smax);
    if (!ALIGNED16(k16) || !ALIGNED16(v16) || !ALIGNED16(k8pool) || !ALIGNED16(v8pool))
        return fail(VL2_E_SHAPE, "vl2_kv_page_quant: need 16-byte aligned caches and pools");
    if (p0 == p1) return 0;
    const long nrows = 2L * nkv * (p1 - p0);
    hipLaunchKernelGGL(kv_page_quant_kernel, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, ST(stream), (const bf16_t*)k16, (const bf16_t*)v16,
                       (uint8_t*)k8pool, (uint8_t*)v8pool, kspool, vspool, (const int*)table_row, nkv, smax, n_pages, p0, p1);
    return launched("vl2_kv_page_quant");
}
// ---- swapping pages of the paged KV cache (k_kv_swap.h): n whole pages of ONE pool tensor to or from a packed device arena
extern "C" int32_t vl2_kv_pages_move(void* pool, void* arena, const int32_t* page_ids, int32_t n, int32_t n_pages, int64_t page_bytes,
                                     int32_t to_arena, void* stream) {
    if (!pool || !arena || !page_ids) return fail(VL2_E_BADARG, "vl2_kv_pages_move: null pointer");
    if (n < 0 || n > 65535) return fail(VL2_E_BADARG, "vl2_kv_pages_move: n %d outside [0, 65535]", n);
    if (n_pages < 1) return fail(VL2_E_SHAPE, "vl2_kv_pages_move: n_pages %d: the pool holds at least the parking page", n_pages);
    if (page_bytes <= 0 || (page_bytes & 15))
        return fail(VL2_E_SHAPE, "vl2_kv_pages_move: page_bytes %lld must be a positive multiple of 16", (long long)page_bytes);
    if (!ALIGNED16(pool) || !ALIGNED16(arena)) return fail(VL2_E_SHAPE, "vl2_kv_pages_move: need a 16-byte aligned pool and arena");
    if (n == 0) return 0;
    // memory bound: about 2048 workgroups in all, each lane KV_MOVE_UNROLL 16-byte vectors per trip
    const long vpp = (long)(page_bytes / 16);
    const long per_wg = (long)KV_MOVE_UNROLL * 256;
    long gx = (vpp + per_wg - 1) / per_wg;
    const long cap = 2048 / n > 0 ? 2048 / n : 1;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(kv_pages_move_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, ST(stream), (u32x4*)pool, (u32x4*)arena,
                       (const int*)page_ids, n_pages, vpp, to_arena);
    return launched("vl2_kv_pages_move");
}
extern "C" int32_t vl2_argmax(const float* logits, int32_t V, int32_t* tok, int32_t* hist, int32_t step, int32_t* state,
                              void* stream) {
    if (!logits || !tok || V <= 0) return fail(VL2_E_BADARG, "vl2_argmax: bad args");
    hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, ST(stream), logits, V, tok, hist, step, state, (int*)nullptr, 0, (const bf16_t*)nullptr, (bf16_t*)nullptr, 0);
    return launched("vl2_argmax");
}
// do_sample=True: temperature -> top-k -> top-p -> one draw at the host's uniform number (k_sample.h; HF:generation/logits_process.py warpers +
// GenerationMixin._sample).  Same token / history / state protocol as vl2_argmax, so it takes the argmax launch's place in a decode loop or graph.
extern "C" int32_t vl2_sample_token(const float* logits, int32_t V, float temperature, int32_t top_k, float top_p, const float* u, int32_t* tok,
                                    int32_t* hist, int32_t step, int32_t* state, float* dbg, void* stream) {
    if (!logits || !tok || !u || V <= 0) return fail(VL2_E_BADARG, "vl2_sample_token: null pointer or empty vocabulary");
    if (!(temperature > 0.f) || top_k < 0 || !(top_p > 0.f)) return fail(VL2_E_BADARG, "vl2_sample_token: need temperature > 0, top_k >= 0, top_p > 0 (got %g, %d, %g)", (double)temperature, top_k, (double)top_p);
    if (!state && step < 0) return fail(VL2_E_BADARG, "vl2_sample_token: negative step");
    SampleArgs a{logits, V, temperature, top_k, top_p, u, tok, hist, step, state, dbg};
    if (V <= 32768) {                  // the scaled scores fit into LDS beside the kernel's 10 KB of static LDS
        lds_attr<sample_token_kernel<true>>(32768 * 4);
        hipLaunchKernelGGL(sample_token_kernel<true>, dim3(1), dim3(1024), (size_t)V * 4, ST(stream), a);
    } else {
        hipLaunchKernelGGL(sample_token_kernel<false>, dim3(1), dim3(1024), 0, ST(stream), a);
    }
    return launched("vl2_sample_token");
}
// The draws of a batched decode step in ONE launch: row b of the logits is greedy (temperature[b] <= 0: vl2_argmax's token) or sampled (vl2_sample_token's
// token at u[b * ld_u + step[b]], then step[b] += 1); every setting lives on the device, so one captured graph serves any mix (k_sample.h sample_rows_kernel).
extern "C" int32_t vl2_sample_tokens(const float* logits, int64_t ld_logits, int32_t V, int32_t nb, const float* temperature, const int32_t* top_k,
                                     const float* top_p, const float* u, int64_t ld_u, int32_t* step, int32_t* tok, void* stream) {
    if (!logits || !temperature || !top_k || !top_p || !u || !step || !tok) return fail(VL2_E_BADARG, "vl2_sample_tokens: null pointer");
    if (V <= 0 || nb <= 0) return fail(VL2_E_BADARG, "vl2_sample_tokens: need V > 0 and nb > 0 (got %d, %d)", V, nb);
    if (ld_logits < V || ld_u < 1)
        return fail(VL2_E_BADARG, "vl2_sample_tokens: need ld_logits >= V and ld_u >= 1 (got %lld, %lld)", (long long)ld_logits, (long long)ld_u);
    SampleRowsArgs a{logits, ld_logits, V, temperature, top_k, top_p, u, ld_u, step, tok};
    if (V <= 32768) {                  // as vl2_sample_token: the scaled scores of a row in LDS, one row per CU
        lds_attr<sample_rows_kernel<true>>(32768 * 4);
        hipLaunchKernelGGL(sample_rows_kernel<true>, dim3(nb), dim3(1024), (size_t)V * 4, ST(stream), a);
    } else {
        hipLaunchKernelGGL(sample_rows_kernel<false>, dim3(nb), dim3(1024), 0, ST(stream), a);
    }
    return launched("vl2_sample_tokens");
}
// the decode step's argmax, which also clears `nzero` int32 words (the fused attention launches' ticket counters)
static int32_t argmax_and_clear(const float* logits, int32_t V, int32_t* tok, int32_t* hist, int32_t* state, int32_t* zero, int32_t nzero,
                                const void* embed, void* x0, int32_t D, void* stream) {
    hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, ST(stream), logits, V, tok, hist, 0, state, (int*)zero, nzero,
                       (const bf16_t*)embed, (bf16_t*)x0, D);
    return launched("vl2_llm_decode_step: argmax");
}
#ifdef VL2_LAB
extern "C" int32_t vl2_decode_tail(const void* Wo, const void* Wgu, const void* Wd, int32_t ldwo, int32_t ldwgu, int32_t ldwd, const void* o,
                                   const void* x0, void* x1, void* act, void* xout, int32_t D, int32_t QD, int32_t I, float eps, int32_t* bar,
                                   void* stream) {
    if (!Wo || !Wgu || !Wd || !o || !x0 || !x1 || !act || !xout || !bar) return fail(VL2_E_BADARG, "vl2_decode_tail: null pointer");
    if (D <= 0 || QD <= 0 || I <= 0 || D % 8 || QD % 8 || I % 32 || ldwo % 8 || ldwgu % 8 || ldwd % 8 || D > 32512 || QD > 32512 || I > 32512)
        return fail(VL2_E_SHAPE, "vl2_decode_tail: need D, QD %% 8 == 0, I %% 32 == 0, all <= 32512 (D %d QD %d I %d)", D, QD, I);
    if ((uintptr_t)bar & 3) return fail(VL2_E_BADARG, "vl2_decode_tail: bar must be 4-byte aligned");
    TailArgs a{(const bf16_t*)Wo, (const bf16_t*)Wgu, (const bf16_t*)Wd, ldwo, ldwgu, ldwd, (const bf16_t*)o, (const bf16_t*)x0, (bf16_t*)x1,
               (bf16_t*)act, (bf16_t*)xout, D, QD, I, eps, (unsigned*)bar};
    const int kmax = QD > D ? (QD > I ? QD : I) : (D > I ? D : I);
    const int g = cu_count() & ~7;                                 // one workgroup per CU (the grid barrier needs all of them resident), 8 groups
    if (g <= 0 || (long)I > (long)TAIL_MAX_ROWS * TAIL_WAVES * g || (long)D > (long)TAIL_MAX_ROWS * TAIL_WAVES * g)
        return fail(VL2_E_SHAPE, "vl2_decode_tail: %d rows per phase exceed %d per wave on %d workgroups", I > D ? I : D, TAIL_MAX_ROWS, g);
    hipLaunchKernelGGL((decode_tail_kernel<7>), dim3(g), dim3(1024), (size_t)kmax * 2, ST(stream), a);
    return launched("vl2_decode_tail");
}
#endif
extern "C" int32_t vl2_embed_rows(const int32_t* ids, const void* table, void* out, int32_t n, int32_t D, int32_t ldo, void* stream) {
    if (!ids || !table || !out || n <= 0 || D % 8 || ldo % 8) return fail(VL2_E_BADARG, "vl2_embed_rows: bad args");
    hipLaunchKernelGGL(embed_rows_kernel, dim3(n), dim3(128), 0, ST(stream), ids, (const bf16_t*)table, (bf16_t*)out, D, ldo);
    return launched("vl2_embed_rows");
}

// ------------------------------------------------------------------------------------------------ sparse MoE (Mixtral), k_moe.h
static bool moe_rows_ok(int S, int k, int E, int P) {
    return P % MOE_BM == 0 && (int64_t)P >= (int64_t)S * k + (int64_t)E * (MOE_BM - 1);
}
extern "C" int32_t vl2_moe_route(const void* x, int32_t ldx, const float* wr, int32_t S, int32_t D, int32_t E, int32_t k, float eps,
                                 int32_t* ids, float* wts, float* rstd, float* logits, int32_t* counts, int32_t* offs, int32_t* gather,
                                 int32_t* inv, int32_t P, void* xg, float* rn_g, void* stream) {
    if (!x || !wr || !ids || !wts || !rstd || !counts || !offs || !gather || !inv || S <= 0 || D <= 0 || E <= 0 || k <= 0)
        return fail(VL2_E_BADARG, "vl2_moe_route: null pointer or empty shape");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "vl2_moe_route: need E <= %d and 1 <= k <= min(E, %d) (E=%d k=%d)", MOE_MAX_E, MOE_MAX_K, E, k);
    if ((int64_t)S * k > MOE_SCAN_MAX) return fail(VL2_E_UNSUPP, "vl2_moe_route: S * k <= %d (S=%d k=%d)", MOE_SCAN_MAX, S, k);
    if (D % 8 || ldx % 8 || ldx < D || !ALIGNED16(x) || !ALIGNED16(wr) || (xg && !ALIGNED16(xg)))
        return fail(VL2_E_SHAPE, "vl2_moe_route: need D%%8==0, ldx>=D and 16-byte aligned rows (D=%d ldx=%d)", D, ldx);
    if (!moe_rows_ok(S, k, E, P)) return fail(VL2_E_SHAPE, "vl2_moe_route: P=%d must be a multiple of %d and >= S*k + E*%d", P, MOE_BM, MOE_BM - 1);
    if (xg && !rn_g) return fail(VL2_E_BADARG, "vl2_moe_route: the gathered rows need their row-norm table rn_g");
    hipStream_t s = ST(stream);
    hipLaunchKernelGGL(moe_router_kernel, dim3((S + 3) / 4), dim3(256), 0, s, (const bf16_t*)x, ldx, wr, S, D, E, k, eps, ids, wts, rstd, logits);
    hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)ids, S, E, k, MOE_BM, P, counts, offs, gather, inv);
    if (xg) hipLaunchKernelGGL(moe_gather_kernel, dim3(P), dim3(256), 0, s, (const bf16_t*)x, ldx, (const int*)gather, (const float*)rstd, D, (bf16_t*)xg, rn_g);
    return launched("vl2_moe_route");
}
extern "C" int32_t vl2_moe_gemm(const void* A, int32_t lda, const void* W, int64_t w_stride, int32_t ldw, void* C, int32_t ldc, const float* row_norm,
                                float eps, const int32_t* counts, const int32_t* offs, int32_t S, int32_t k, int32_t E, int32_t P, int32_t N, int32_t K,
                                int32_t flags, void* stream) {
    if (!A || !W || !C || !counts || !offs || S <= 0 || k <= 0 || E <= 0 || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_moe_gemm: null pointer or empty shape");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "vl2_moe_gemm: need E <= %d and 1 <= k <= min(E, %d)", MOE_MAX_E, MOE_MAX_K);
    if (N % GEMM_BN || K % 64 || lda % 8 || ldw % 8 || ldc % 8 || w_stride % 8 || lda < K || ldw < K || w_stride < (int64_t)N * ldw ||
        !ALIGNED16(A) || !ALIGNED16(W) || !ALIGNED16(C) || (row_norm && (((uintptr_t)row_norm) & 7)))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm: need N%%%d==0, K%%64==0, 16-byte aligned rows, w_stride >= N*ldw (N=%d K=%d)", GEMM_BN, N, K);
    if (!moe_rows_ok(S, k, E, P)) return fail(VL2_E_SHAPE, "vl2_moe_gemm: P=%d must be a multiple of %d and >= S*k + E*%d", P, MOE_BM, MOE_BM - 1);
    if ((int64_t)(GEMM_BM - 1) * lda + K >= ((int64_t)1 << 30) || (int64_t)(GEMM_BN - 1) * ldw + K >= ((int64_t)1 << 30))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm: a tile's rows exceed the kernels' 32-bit buffer offsets");
    const bool sw = flags & VL2_GEMM_SWIGLU;
    if (flags & ~VL2_GEMM_SWIGLU) return fail(VL2_E_UNSUPP, "vl2_moe_gemm: flags other than VL2_GEMM_SWIGLU not built");
    if (sw && N % 64) return fail(VL2_E_SHAPE, "vl2_moe_gemm: SWIGLU needs N%%64==0");
    MoeGemmArgs q{};
    GemmArgs& a = q.g;
    a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = C;
    a.M = P; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldc = ldc;
    a.stats_out_np = N / 64; a.stats_in_np = K / 64; a.idx_ld = P;
    if (row_norm) { a.norm = VL2_NORM_RMS; a.norm_eps = eps; a.row_norm = row_norm; }
    q.offs = offs; q.counts = counts; q.w_stride = w_stride; q.E = E; q.rt_cap = P / MOE_BM;
    const dim3 grid((unsigned)(q.rt_cap * (N / GEMM_BN)));
    hipStream_t s = ST(stream);
    if (sw) launch<moe_gemm_kernel<true>>(grid, dim3(512), GEMML_LDS_BYTES, s, q);
    else launch<moe_gemm_kernel<false>>(grid, dim3(512), GEMML_LDS_BYTES, s, q);
    return launched("vl2_moe_gemm");
}
extern "C" int32_t vl2_moe_combine(const void* x1, int32_t ldx1, const void* y, int32_t ldy, const int32_t* inv, const float* wts, int32_t S, int32_t k,
                                   int32_t D, float eps, void* out, int32_t ldo, float* row_norm, void* stream) {
    if (!x1 || !y || !inv || !wts || !out || S <= 0 || k <= 0 || D <= 0) return fail(VL2_E_BADARG, "vl2_moe_combine: null pointer or empty shape");
    if (k > MOE_MAX_K) return fail(VL2_E_UNSUPP, "vl2_moe_combine: k <= %d", MOE_MAX_K);
    if (D % 8 || ldx1 % 8 || ldy % 8 || ldo % 8 || ldx1 < D || ldy < D || ldo < D || !ALIGNED16(x1) || !ALIGNED16(y) || !ALIGNED16(out) ||
        (row_norm && (((uintptr_t)row_norm) & 7)))
        return fail(VL2_E_SHAPE, "vl2_moe_combine: need D%%8==0, ldx1 / ldy / ldo >= D and 16-byte aligned rows (D=%d)", D);
    hipLaunchKernelGGL(moe_combine_kernel, dim3(S), dim3(256), 0, ST(stream), (const bf16_t*)x1, ldx1, (const bf16_t*)y, ldy, (const int*)inv, wts, k, D, eps,
                       (bf16_t*)out, ldo, row_norm);
    return launched("vl2_moe_combine");
}
extern "C" int32_t vl2_moe_route_gemv(const void* x, const float* wr, int32_t D, int32_t E, int32_t k, float eps, int32_t* ids, float* wts, float* logits,
                                      void* stream) {
    if (!x || !wr || !ids || !wts || D <= 0 || E <= 0 || k <= 0) return fail(VL2_E_BADARG, "vl2_moe_route_gemv: null pointer or empty shape");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "vl2_moe_route_gemv: need E <= %d and 1 <= k <= min(E, %d)", MOE_MAX_E, MOE_MAX_K);
    if (D % 8 || !ALIGNED16(x) || !ALIGNED16(wr)) return fail(VL2_E_SHAPE, "vl2_moe_route_gemv: need D%%8==0 and 16-byte aligned rows");
    hipLaunchKernelGGL(moe_router_kernel, dim3(1), dim3(256), 0, ST(stream), (const bf16_t*)x, D, wr, 1, D, E, k, eps, ids, wts,
                       (float*)nullptr, logits);
    return launched("vl2_moe_route_gemv");
}
extern "C" int32_t vl2_moe_gemv(const void* W, int64_t w_stride, int32_t ldw, const void* x, const int32_t* ids, const float* wts, const void* res,
                                void* y, int32_t E, int32_t k, int32_t N, int32_t K, float eps, int32_t flags, void* stream) {
    if (!W || !x || !ids || !y || E <= 0 || k <= 0 || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_moe_gemv: null pointer or empty shape");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "vl2_moe_gemv: need E <= %d and 1 <= k <= min(E, %d)", MOE_MAX_E, MOE_MAX_K);
    if (K % 8 || ldw % 8 || ldw < K || w_stride < (int64_t)N * ldw || !ALIGNED16(W) || !ALIGNED16(x) || !ALIGNED16(y))
        return fail(VL2_E_SHAPE, "vl2_moe_gemv: need K%%8==0, 16-byte aligned rows, w_stride >= N*ldw");
    if (flags & ~VL2_GEMM_SWIGLU) return fail(VL2_E_UNSUPP, "vl2_moe_gemv: flags other than VL2_GEMM_SWIGLU not built");
    hipStream_t s = ST(stream);
    if (flags & VL2_GEMM_SWIGLU) {
        if (N % 64 || K > 32704 || wts || res) return fail(VL2_E_SHAPE, "vl2_moe_gemv: SWIGLU needs N%%64==0, K<=32704 and no wts / res");
        GemvArgs a{(const bf16_t*)W, (const bf16_t*)x, nullptr, nullptr, y, N, K, ldw, eps, nullptr, 0, 0, 0, 1};
        hipLaunchKernelGGL(moe_gemv_gu_kernel, dim3((N / 2 + 3) / 4, k), dim3(256), (size_t)K * 2, s, a, (const int*)ids, (long long)w_stride, N / 2);
        return launched("vl2_moe_gemv");
    }
    if (!wts) return fail(VL2_E_BADARG, "vl2_moe_gemv: the down form needs the routing weights");
    const size_t lds = (size_t)k * K * 2;
    if (lds > 160 * 1024) return fail(VL2_E_SHAPE, "vl2_moe_gemv: k * K * 2 bytes of activations must fit the LDS (k=%d K=%d)", k, K);
    const dim3 g((N + 3) / 4), b(256);
#define VL2_MOE_DOWN(KS) do { lds_attr<moe_gemv_down_kernel<KS>>(160 * 1024); \
        hipLaunchKernelGGL((moe_gemv_down_kernel<KS>), g, b, lds, s, (const bf16_t*)W, (long long)w_stride, ldw, (const bf16_t*)x, (const int*)ids, wts, \
                           (const bf16_t*)res, (bf16_t*)y, N, K); } while (0)
    if (k == 1) VL2_MOE_DOWN(1); else if (k == 2) VL2_MOE_DOWN(2); else if (k == 3) VL2_MOE_DOWN(3); else VL2_MOE_DOWN(4);
#undef VL2_MOE_DOWN
    return launched("vl2_moe_gemv");
}

// ------------------------------------------------------------------------------------------------ batched MoE decode, k_moe_skinny.h
extern "C" int32_t vl2_moe_route_rows(const void* x, int32_t ldx, const float* wr, int32_t S, int32_t D, int32_t E, int32_t k, float eps, int32_t* ids,
                                      float* wts, float* logits, int32_t* counts, int32_t* offs, int32_t* gather, int32_t* inv, void* stream) {
    if (!x || !wr || !ids || !wts || S <= 0 || D <= 0 || E <= 0 || k <= 0) return fail(VL2_E_BADARG, "vl2_moe_route_rows: null pointer or empty shape");
    const bool tables = counts || offs || gather || inv;
    if (tables && (!counts || !offs || !gather || !inv)) return fail(VL2_E_BADARG, "vl2_moe_route_rows: counts / offs / gather / inv come together or not at all");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E)
        return fail(VL2_E_UNSUPP, "vl2_moe_route_rows: need E <= %d and 1 <= k <= min(E, %d) (E=%d k=%d)", MOE_MAX_E, MOE_MAX_K, E, k);
    if ((int64_t)S * k > MOE_SCAN_MAX) return fail(VL2_E_UNSUPP, "vl2_moe_route_rows: S * k <= %d (S=%d k=%d)", MOE_SCAN_MAX, S, k);
    if (D % 8 || ldx % 8 || ldx < D || !ALIGNED16(x) || !ALIGNED16(wr))
        return fail(VL2_E_SHAPE, "vl2_moe_route_rows: need D%%8==0, ldx>=D and 16-byte aligned rows (D=%d ldx=%d)", D, ldx);
    hipStream_t s = ST(stream);
    hipLaunchKernelGGL(moe_router_kernel, dim3((S + 3) / 4), dim3(256), 0, s, (const bf16_t*)x, ldx, wr, S, D, E, k, eps, ids, wts, (float*)nullptr, logits);
    if (tables) hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)ids, S, E, k, 1, S * k, counts, offs, gather, inv);
    return launched("vl2_moe_route_rows");
}
// the K split of the grouped skinny GEMM: skinny_plan's for (N, K), never shrunk; the staged rows (mt) from S
static int moe_skinny_plan(int S, int N, int K, SkinnyPlan& pl) { return skinny_plan(S, N, K, INT64_MAX, false, pl); }
extern "C" int64_t vl2_moe_gemm_skinny_part_bytes(int32_t S, int32_t k, int32_t N, int32_t K) {
    SkinnyPlan pl;
    if (S <= 0 || S > 64 || k <= 0 || k > MOE_MAX_K || N <= 0 || K <= 0 || N % 64 || K % 32 || moe_skinny_plan(S, N, K, pl) != SKINNY_PLAN_OK) return -1;
    return (int64_t)pl.ks * S * k * N * 4;
}
extern "C" int32_t vl2_moe_gemm_skinny(const void* A, int32_t lda, int32_t a_rows, const int32_t* rowmap, const void* W, int64_t w_stride, int32_t ldw,
                                       void* C, int32_t ldc, const int32_t* counts, const int32_t* offs, int32_t S, int32_t k, int32_t E, int32_t N,
                                       int32_t K, int32_t flags, void* part, int64_t part_bytes, void* stream) {
    if (!A || !W || !C || !counts || !offs || S <= 0 || k <= 0 || E <= 0 || N <= 0 || K <= 0 || a_rows <= 0)
        return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny: null pointer or empty shape");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "vl2_moe_gemm_skinny: need E <= %d and 1 <= k <= min(E, %d)", MOE_MAX_E, MOE_MAX_K);
    if (S > 64) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny: S=%d tokens, need S<=64 (vl2_moe_gemm beyond)", S);
    const bool sw = flags & VL2_GEMM_SWIGLU;
    if (flags & ~VL2_GEMM_SWIGLU) return fail(VL2_E_UNSUPP, "vl2_moe_gemm_skinny: flags other than VL2_GEMM_SWIGLU not built");
    if (N % 64 || (sw && N % 128)) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny: need N%%64==0 (N%%128==0 with SWIGLU; N=%d)", N);
    if (K % 32) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny: need K%%32==0 (K=%d)", K);
    const int R = S * k;
    if (lda % 8 || ldw % 8 || ldc % 4 || lda < K || ldw < K || w_stride % 8 || w_stride < (int64_t)N * ldw || ldc < (sw ? N / 2 : N) ||
        !ALIGNED16(A) || !ALIGNED16(W) || (((uintptr_t)C) & 7))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny: need 16-byte aligned rows, lda%%8==0, ldw%%8==0, ldc%%4==0, lda / ldw >= K, w_stride >= N*ldw");
    if (a_rows < (rowmap ? S : R)) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny: A has %d rows, need %d", a_rows, rowmap ? S : R);
    if (!part || !ALIGNED16(part) || part_bytes <= 0) return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny: needs a 16-byte aligned buffer of fp32 partial sums");
    SkinnyPlan pl;
    if (moe_skinny_plan(S, N, K, pl) != SKINNY_PLAN_OK) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny: no K chunking for K=%d", K);
    const int64_t need = (int64_t)pl.ks * R * N * 4;
    if (need > part_bytes)
        return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny: partial buffer too small (%lld bytes, need %lld: the K split is never shrunk)", (long long)part_bytes, (long long)need);
    MoeSkinnyArgs q{};
    q.g = SkinnyArgs{(const bf16_t*)A, (const bf16_t*)W, (float*)part, S, N, K, lda, ldw, pl.kslice, pl.kchunk};
    q.counts = counts; q.offs = offs; q.rowmap = rowmap; q.w_stride = w_stride; q.R = R; q.a_rows = a_rows;
    hipStream_t s = ST(stream);
    const dim3 gk(N / 64, pl.ks, E), b(256);
    if (pl.mt == 1) { lds_attr<moe_skinny_kernel<1>>(65536); hipLaunchKernelGGL(moe_skinny_kernel<1>, gk, b, pl.lds, s, q); }
    else if (pl.mt == 2) { lds_attr<moe_skinny_kernel<2>>(65536); hipLaunchKernelGGL(moe_skinny_kernel<2>, gk, b, pl.lds, s, q); }
    else { lds_attr<moe_skinny_kernel<4>>(65536); hipLaunchKernelGGL(moe_skinny_kernel<4>, gk, b, pl.lds, s, q); }
    SkinnyReduceArgs r{(const float*)part, C, nullptr, nullptr, R, R, N, pl.ks, ldc, 0, nullptr};
    const dim3 g((R * ((sw ? N / 2 : N) / 4) + 255) / 256);
    if (sw) hipLaunchKernelGGL((skinny_reduce_kernel<true, false, false>), g, b, 0, s, r);
    else hipLaunchKernelGGL((skinny_reduce_kernel<false, false, false>), g, b, 0, s, r);
    return launched("vl2_moe_gemm_skinny");
}
extern "C" int32_t vl2_moe_gemv_batched(const void* W, int64_t w_stride, int32_t ldw, const void* x, int32_t ldx, const int32_t* ids, const float* wts,
                                        const void* res, int32_t ldres, void* y, int32_t ldy, int32_t S, int32_t E, int32_t k, int32_t N, int32_t K,
                                        float eps, int32_t flags, void* stream) {
    if (!W || !x || !ids || !y || S <= 0 || E <= 0 || k <= 0 || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_moe_gemv_batched: null pointer or empty shape");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "vl2_moe_gemv_batched: need E <= %d and 1 <= k <= min(E, %d)", MOE_MAX_E, MOE_MAX_K);
    if (S > 65535) return fail(VL2_E_SHAPE, "vl2_moe_gemv_batched: S=%d tokens exceed the grid", S);
    if (K % 8 || ldw % 8 || ldw < K || w_stride < (int64_t)N * ldw || ldx % 8 || ldx < K || !ALIGNED16(W) || !ALIGNED16(x) || !ALIGNED16(y))
        return fail(VL2_E_SHAPE, "vl2_moe_gemv_batched: need K%%8==0, 16-byte aligned rows, ldw / ldx >= K, w_stride >= N*ldw");
    if (flags & ~VL2_GEMM_SWIGLU) return fail(VL2_E_UNSUPP, "vl2_moe_gemv_batched: flags other than VL2_GEMM_SWIGLU not built");
    hipStream_t s = ST(stream);
    if (flags & VL2_GEMM_SWIGLU) {       // x [S, ldx] -> y [S * k, ldy]
        if (N % 64 || K > 32704 || wts || res || ldy < N / 2) return fail(VL2_E_SHAPE, "vl2_moe_gemv_batched: SWIGLU needs N%%64==0, K<=32704, ldy >= N/2 and no wts / res");
        GemvArgs a{(const bf16_t*)W, (const bf16_t*)x, nullptr, nullptr, y, N, K, ldw, eps, nullptr, 0, 0, 0, 1};
        hipLaunchKernelGGL(moe_gemv_gu_rows_kernel, dim3((N / 2 + 3) / 4, k, S), dim3(256), (size_t)K * 2, s, a, (const int*)ids, (long long)w_stride, ldy, ldx);
        return launched("vl2_moe_gemv_batched");
    }
    if (!wts) return fail(VL2_E_BADARG, "vl2_moe_gemv_batched: the down form needs the routing weights");
    if (ldx != K) return fail(VL2_E_SHAPE, "vl2_moe_gemv_batched: the down form reads the SwiGLU rows [S * k, K] without a gap (ldx=%d K=%d)", ldx, K);
    if (ldy < N || (res && ldres < N)) return fail(VL2_E_SHAPE, "vl2_moe_gemv_batched: need ldy / ldres >= N (N=%d)", N);
    const size_t lds = (size_t)k * K * 2;
    if (lds > 160 * 1024) return fail(VL2_E_SHAPE, "vl2_moe_gemv_batched: k * K * 2 bytes of activations must fit the LDS (k=%d K=%d)", k, K);
    const dim3 g((N + 3) / 4, S), b(256);
#define VL2_MOE_DOWN(KS) do { lds_attr<moe_gemv_down_rows_kernel<KS>>(160 * 1024); \
        hipLaunchKernelGGL((moe_gemv_down_rows_kernel<KS>), g, b, lds, s, (const bf16_t*)W, (long long)w_stride, ldw, (const bf16_t*)x, (const int*)ids, wts, \
                           (const bf16_t*)res, ldres, (bf16_t*)y, ldy, N, K); } while (0)
    if (k == 1) VL2_MOE_DOWN(1); else if (k == 2) VL2_MOE_DOWN(2); else if (k == 3) VL2_MOE_DOWN(3); else VL2_MOE_DOWN(4);
#undef VL2_MOE_DOWN
    return launched("vl2_moe_gemv_batched");
}

// ------------------------------------------------------------------------------------------------ fp8 expert weights of the MoE decode, k_moe_fp8.h
// ONE host routine behind vl2_moe_gemv_fp8 (S = 1, the rows' strides their widths) and vl2_moe_gemv_batched_fp8.  Every check precedes every launch.
static int32_t moe_gemv_fp8_rows(const char* who, const void* q, int64_t q_stride, int32_t ldq, const float* scale, int64_t s_stride, const void* x,
                                 int32_t ldx, const int32_t* ids, const float* wts, const void* res, int32_t ldres, void* y, int32_t ldy, int32_t S,
                                 int32_t E, int32_t k, int32_t N, int32_t K, float eps, int32_t flags, void* stream) {
    if (!q) return fail(VL2_E_BADARG, "%s: null q (the e4m3fn expert weights)", who);
    if (!scale) return fail(VL2_E_BADARG, "%s: null scale (the experts' row scales)", who);
    if (!x || !ids || !y || S <= 0 || E <= 0 || k <= 0 || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "%s: null pointer or empty shape", who);
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "%s: need E <= %d and 1 <= k <= min(E, %d)", who, MOE_MAX_E, MOE_MAX_K);
    if (S > 65535) return fail(VL2_E_SHAPE, "%s: S=%d tokens exceed the grid", who, S);
    if (flags & ~VL2_GEMM_SWIGLU) return fail(VL2_E_UNSUPP, "%s: flags other than VL2_GEMM_SWIGLU not built", who);
    if (K % 16 || K > 32704) return fail(VL2_E_SHAPE, "%s: need K%%16==0, K<=32704 (K=%d)", who, K);
    if (ldq % 16 || ldq < K || q_stride % 16 || q_stride < (int64_t)N * ldq || s_stride < N || ldx % 8 || ldx < K || !ALIGNED16(q) || !ALIGNED16(x))
        return fail(VL2_E_SHAPE, "%s: need 16-byte aligned rows, ldq%%16==0, ldq / ldx >= K, q_stride >= N*ldq, s_stride >= N", who);
    hipStream_t s = ST(stream);
    if (flags & VL2_GEMM_SWIGLU) {       // x [S, ldx] -> y [S * k, ldy]
        if (N % 2) return fail(VL2_E_SHAPE, "%s: need N even (N=%d)", who, N);
        if (N % 64 || wts || res || ldy < N / 2) return fail(VL2_E_SHAPE, "%s: SWIGLU needs N%%64==0, ldy >= N/2 and no wts / res", who);
        Gemv8Args a{(const uint8_t*)q, scale, (const bf16_t*)x, nullptr, nullptr, y, N, K, ldq, eps, nullptr, 1, 0, 0, 0};
        const dim3 b(256);
        // vl2_gemv_fp8's rule: rows of K <= 4096 run two pairs per wave and trip
        if (K <= 4096)
            hipLaunchKernelGGL(moe_gemv_gu_fp8_kernel<2>, dim3((N / 2 + 7) / 8, k, S), b, (size_t)K * 2, s, a, (const int*)ids, (long long)q_stride,
                               (long long)s_stride, E, ldy, ldx);
        else
            hipLaunchKernelGGL(moe_gemv_gu_fp8_kernel<1>, dim3((N / 2 + 3) / 4, k, S), b, (size_t)K * 2, s, a, (const int*)ids, (long long)q_stride,
                               (long long)s_stride, E, ldy, ldx);
        return launched(who);
    }
    if (!wts) return fail(VL2_E_BADARG, "%s: the down form needs the routing weights", who);
    if (ldx != K) return fail(VL2_E_SHAPE, "%s: the down form reads the SwiGLU rows [S * k, K] without a gap (ldx=%d K=%d)", who, ldx, K);
    if (ldy < N || (res && ldres < N)) return fail(VL2_E_SHAPE, "%s: need ldy / ldres >= N (N=%d)", who, N);
    const size_t lds = (size_t)k * K * 2;
    if (lds > 160 * 1024) return fail(VL2_E_SHAPE, "%s: k * K * 2 bytes of activations must fit the LDS (k=%d K=%d)", who, k, K);
    const dim3 g((N + 3) / 4, S), b(256);
#define VL2_MOE_DOWN8(KS) do { lds_attr<moe_gemv_down_fp8_kernel<KS>>(160 * 1024); \
        hipLaunchKernelGGL((moe_gemv_down_fp8_kernel<KS>), g, b, lds, s, (const uint8_t*)q, (long long)q_stride, ldq, scale, (long long)s_stride, \
                           (const bf16_t*)x, (const int*)ids, wts, (const bf16_t*)res, ldres, (bf16_t*)y, ldy, N, K, E); } while (0)
    if (k == 1) VL2_MOE_DOWN8(1); else if (k == 2) VL2_MOE_DOWN8(2); else if (k == 3) VL2_MOE_DOWN8(3); else VL2_MOE_DOWN8(4);
#undef VL2_MOE_DOWN8
    return launched(who);
}
extern "C" int32_t vl2_moe_gemv_fp8(const void* q, int64_t q_stride, int32_t ldq, const float* scale, int64_t s_stride, const void* x, const int32_t* ids,
                                    const float* wts, const void* res, void* y, int32_t E, int32_t k, int32_t N, int32_t K, float eps, int32_t flags,
                                    void* stream) {
    const int n_out = (flags & VL2_GEMM_SWIGLU) ? N / 2 : N;
    return moe_gemv_fp8_rows("vl2_moe_gemv_fp8", q, q_stride, ldq, scale, s_stride, x, K, ids, wts, res, n_out, y, n_out, 1, E, k, N, K, eps, flags, stream);
}
extern "C" int32_t vl2_moe_gemv_batched_fp8(const void* q, int64_t q_stride, int32_t ldq, const float* scale, int64_t s_stride, const void* x, int32_t ldx,
                                            const int32_t* ids, const float* wts, const void* res, int32_t ldres, void* y, int32_t ldy, int32_t S,
                                            int32_t E, int32_t k, int32_t N, int32_t K, float eps, int32_t flags, void* stream) {
    return moe_gemv_fp8_rows("vl2_moe_gemv_batched_fp8", q, q_stride, ldq, scale, s_stride, x, ldx, ids, wts, res, ldres, y, ldy, S, E, k, N, K, eps, flags,
                             stream);
}
extern "C" int32_t vl2_moe_gemm_skinny_fp8(const void* A, int32_t lda, int32_t a_rows, const int32_t* rowmap, const void* q, int64_t q_stride, int32_t ldq,
                                           const float* scale, int64_t s_stride, void* C, int32_t ldc, const int32_t* counts, const int32_t* offs,
                                           int32_t S, int32_t k, int32_t E, int32_t N, int32_t K, int32_t flags, void* part, int64_t part_bytes,
                                           void* stream) {
    if (!q) return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny_fp8: null q (the e4m3fn expert weights)");
    if (!scale) return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny_fp8: null scale (the experts' row scales)");
    if (!A || !C || !counts || !offs || S <= 0 || k <= 0 || E <= 0 || N <= 0 || K <= 0 || a_rows <= 0)
        return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny_fp8: null pointer or empty shape");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "vl2_moe_gemm_skinny_fp8: need E <= %d and 1 <= k <= min(E, %d)", MOE_MAX_E, MOE_MAX_K);
    if (S > 64) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_fp8: S=%d tokens, need S<=64 (no tiled W8A16 grouped GEMM is built)", S);
    const bool sw = flags & VL2_GEMM_SWIGLU;
    if (flags & ~VL2_GEMM_SWIGLU) return fail(VL2_E_UNSUPP, "vl2_moe_gemm_skinny_fp8: flags other than VL2_GEMM_SWIGLU not built");
    if (N % 64 || (sw && N % 128)) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_fp8: need N%%64==0 (N%%128==0 with SWIGLU; N=%d)", N);
    if (K % 32 || K > 32704) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_fp8: need K%%32==0, K<=32704 (K=%d)", K);
    const int R = S * k;
    if (lda % 8 || ldq % 16 || ldc % 4 || lda < K || ldq < K || q_stride % 16 || q_stride < (int64_t)N * ldq || s_stride < N || ldc < (sw ? N / 2 : N) ||
        !ALIGNED16(A) || !ALIGNED16(q) || (((uintptr_t)C) & 7) || (((uintptr_t)scale) & 3))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_fp8: need 16-byte aligned rows, lda%%8==0, ldq%%16==0, ldc%%4==0, lda / ldq >= K, q_stride >= N*ldq, s_stride >= N");
    if (a_rows < (rowmap ? S : R)) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_fp8: A has %d rows, need %d", a_rows, rowmap ? S : R);
    if (!part || !ALIGNED16(part) || part_bytes <= 0) return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny_fp8: needs a 16-byte aligned buffer of fp32 partial sums");
    SkinnyPlan pl;
    if (moe_skinny_plan(S, N, K, pl) != SKINNY_PLAN_OK) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_fp8: no K chunking for K=%d", K);
    const int64_t need = (int64_t)pl.ks * R * N * 4;
    if (need > part_bytes)
        return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny_fp8: partial buffer too small (%lld bytes, need %lld: the K split is never shrunk)", (long long)part_bytes, (long long)need);
    MoeSkinnyArgsT<Skinny8Args> a{};
    a.g = Skinny8Args{(const bf16_t*)A, (const uint8_t*)q, (float*)part, S, N, K, lda, ldq, pl.kslice, pl.kchunk};
    a.counts = counts; a.offs = offs; a.rowmap = rowmap; a.w_stride = q_stride; a.R = R; a.a_rows = a_rows;
    hipStream_t s = ST(stream);
    const dim3 gk(N / 64, pl.ks, E), b(256);
    if (pl.mt == 1) { lds_attr<moe_skinny_kernel<1, SkinnyWFp8>>(65536); hipLaunchKernelGGL((moe_skinny_kernel<1, SkinnyWFp8>), gk, b, pl.lds, s, a); }
    else if (pl.mt == 2) { lds_attr<moe_skinny_kernel<2, SkinnyWFp8>>(65536); hipLaunchKernelGGL((moe_skinny_kernel<2, SkinnyWFp8>), gk, b, pl.lds, s, a); }
    else { lds_attr<moe_skinny_kernel<4, SkinnyWFp8>>(65536); hipLaunchKernelGGL((moe_skinny_kernel<4, SkinnyWFp8>), gk, b, pl.lds, s, a); }
    SkinnyReduceArgs r{(const float*)part, C, nullptr, nullptr, R, R, N, pl.ks, ldc, 0, scale};
    const dim3 g((R * ((sw ? N / 2 : N) / 4) + 255) / 256);
    if (sw) hipLaunchKernelGGL(moe_skinny_reduce_fp8_kernel<true>, g, b, 0, s, r, (const int*)counts, (const int*)offs, E, (long long)s_stride);
    else hipLaunchKernelGGL(moe_skinny_reduce_fp8_kernel<false>, g, b, 0, s, r, (const int*)counts, (const int*)offs, E, (long long)s_stride);
    return launched("vl2_moe_gemm_skinny_fp8");
}

// ------------------------------------------------------------------------------------------------ tiled W8A16 grouped GEMM, k_moe_gemm8.h
// vl2_moe_gemm on the fp8 expert stacks: every check of vl2_moe_gemm, restated for bytes, precedes the launch.
extern "C" int32_t vl2_moe_gemm_fp8(const void* A, int32_t lda, const void* q, int64_t q_stride, int32_t ldq, const float* scale, int64_t s_stride, void* C,
                                    int32_t ldc, const float* row_norm, float eps, const int32_t* counts, const int32_t* offs, int32_t S, int32_t k, int32_t E,
                                    int32_t P, int32_t N, int32_t K, int32_t flags, void* stream) {
    if (!q) return fail(VL2_E_BADARG, "vl2_moe_gemm_fp8: null q (the e4m3fn expert weights)");
    if (!scale) return fail(VL2_E_BADARG, "vl2_moe_gemm_fp8: null scale (the experts' row scales)");
    if (!A || !C || !counts || !offs || S <= 0 || k <= 0 || E <= 0 || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_moe_gemm_fp8: null pointer or empty shape");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "vl2_moe_gemm_fp8: need E <= %d and 1 <= k <= min(E, %d)", MOE_MAX_E, MOE_MAX_K);
    if (N % GEMM_BN || K % 64 || lda % 8 || ldc % 8 || lda < K || !ALIGNED16(A) || !ALIGNED16(C) || (row_norm && (((uintptr_t)row_norm) & 7)))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm_fp8: need N%%%d==0, K%%64==0, 16-byte aligned rows (N=%d K=%d)", GEMM_BN, N, K);
    if (ldq % 16 || ldq < K || q_stride % 16 || q_stride < (int64_t)N * ldq || !ALIGNED16(q))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm_fp8: need 16-byte aligned weight rows, ldq%%16==0, ldq >= K, q_stride%%16==0, q_stride >= N*ldq (ldq=%d)", ldq);
    if (!ALIGNED16(scale) || s_stride % 4 || s_stride < N)
        return fail(VL2_E_SHAPE, "vl2_moe_gemm_fp8: need 16-byte aligned scale rows, s_stride%%4==0, s_stride >= N (N=%d)", N);
    if (!moe_rows_ok(S, k, E, P)) return fail(VL2_E_SHAPE, "vl2_moe_gemm_fp8: P=%d must be a multiple of %d and >= S*k + E*%d", P, MOE_BM, MOE_BM - 1);
    if ((int64_t)(GEMM_BM - 1) * lda + K >= ((int64_t)1 << 30) || (int64_t)(GEMM_BN - 1) * ldq + K >= ((int64_t)1 << 30))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm_fp8: a tile's rows exceed the kernels' 32-bit buffer offsets");
    const bool sw = flags & VL2_GEMM_SWIGLU;
    if (flags & ~VL2_GEMM_SWIGLU) return fail(VL2_E_UNSUPP, "vl2_moe_gemm_fp8: flags other than VL2_GEMM_SWIGLU not built");
    MoeGemm8Args m{};
    GemmArgs& a = m.g;
    a.A = (const bf16_t*)A; a.C = C;
    a.M = P; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc;
    a.stats_out_np = N / 64; a.stats_in_np = K / 64; a.idx_ld = P;
    if (row_norm) { a.norm = VL2_NORM_RMS; a.norm_eps = eps; a.row_norm = row_norm; }
    m.offs = offs; m.counts = counts; m.q = (const uint8_t*)q; m.scale = scale; m.q_stride = q_stride; m.s_stride = s_stride; m.ldq = ldq; m.E = E;
    m.rt_cap = P / MOE_BM;
    const dim3 grid((unsigned)(m.rt_cap * (N / GEMM_BN)));
    hipStream_t s = ST(stream);
    if (sw) launch<moe_gemm8_kernel<true>>(grid, dim3(512), MOE8_LDS_BYTES, s, m);
    else launch<moe_gemm8_kernel<false>>(grid, dim3(512), MOE8_LDS_BYTES, s, m);
    return launched("vl2_moe_gemm_fp8");
}

// ------------------------------------------------------------------------------------------------ MXFP4 expert weights of the MoE decode, k_moe_mxfp4.h
// ONE host routine behind vl2_moe_gemv_mxfp4 (S = 1, the rows' strides their widths) and vl2_moe_gemv_batched_mxfp4.  Every check precedes every
// launch.  vl2_moe_gemm_skinny_mxfp4 (S <= 64) is the grouped form of these three; the tiled W4A16 grouped GEMM is vl2_moe_gemm_mxfp4 below.
static int32_t moe_gemv_mxfp4_rows(const char* who, const void* q, int64_t q_stride, int32_t ldq, const void* scale, int64_t s_stride, int32_t lds_,
                                   const void* x, int32_t ldx, const int32_t* ids, const float* wts, const void* res, int32_t ldres, void* y, int32_t ldy,
                                   int32_t S, int32_t E, int32_t k, int32_t N, int32_t K, float eps, int32_t flags, void* stream) {
    if (!q) return fail(VL2_E_BADARG, "%s: null q (the experts' E2M1 codes)", who);
    if (!scale) return fail(VL2_E_BADARG, "%s: null scale (the experts' E8M0 block scales)", who);
    if (!x || !ids || !y || S <= 0 || E <= 0 || k <= 0 || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "%s: null pointer or empty shape", who);
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "%s: need E <= %d and 1 <= k <= min(E, %d)", who, MOE_MAX_E, MOE_MAX_K);
    if (S > 65535) return fail(VL2_E_SHAPE, "%s: S=%d tokens exceed the grid", who, S);
    if (flags & ~VL2_GEMM_SWIGLU) return fail(VL2_E_UNSUPP, "%s: flags other than VL2_GEMM_SWIGLU not built", who);
    if (K % 32) return fail(VL2_E_SHAPE, "%s: need K%%32==0 (one scale per block of 32; K=%d)", who, K);
    if (K > 32704) return fail(VL2_E_SHAPE, "%s: need K<=32704 (x lives in LDS as 16-bit elements; K=%d)", who, K);
    if (ldq % 16 || ldq < K / 2 || lds_ < K / 32 || q_stride % 16 || q_stride < (int64_t)N * ldq || s_stride < (int64_t)N * lds_ || ldx % 8 || ldx < K ||
        !ALIGNED16(q) || !ALIGNED16(x))
        return fail(VL2_E_SHAPE, "%s: need 16-byte aligned rows, ldq%%16==0, ldq >= K/2, lds >= K/32, ldx >= K, q_stride%%16==0, q_stride >= N*ldq, s_stride >= N*lds", who);
    hipStream_t s = ST(stream);
    if (flags & VL2_GEMM_SWIGLU) {       // x [S, ldx] -> y [S * k, ldy]
        if (N % 64 || wts || res || ldy < N / 2) return fail(VL2_E_SHAPE, "%s: SWIGLU needs N%%64==0, ldy >= N/2 and no wts / res (N=%d)", who, N);
        Gemv4Args a{(const uint8_t*)q, (const uint8_t*)scale, (const bf16_t*)x, nullptr, nullptr, y, N, K, ldq, lds_, eps, nullptr, 1, 0, 0, 0};
        const dim3 b(256);
        // launch_gemv_mxfp4_rows' rule: rows of K <= 4096 run four pairs per wave and trip
        if (K <= 4096)
            hipLaunchKernelGGL(moe_gemv_gu_mxfp4_kernel<4>, dim3((N / 2 + 15) / 16, k, S), b, (size_t)K * 2, s, a, (const int*)ids, (long long)q_stride,
                               (long long)s_stride, E, ldy, ldx);
        else
            hipLaunchKernelGGL(moe_gemv_gu_mxfp4_kernel<1>, dim3((N / 2 + 3) / 4, k, S), b, (size_t)K * 2, s, a, (const int*)ids, (long long)q_stride,
                               (long long)s_stride, E, ldy, ldx);
        return launched(who);
    }
    if (!wts) return fail(VL2_E_BADARG, "%s: the down form needs the routing weights", who);
    if (ldx != K) return fail(VL2_E_SHAPE, "%s: the down form reads the SwiGLU rows [S * k, K] without a gap (ldx=%d K=%d)", who, ldx, K);
    if (ldy < N || (res && ldres < N)) return fail(VL2_E_SHAPE, "%s: need ldy / ldres >= N (N=%d)", who, N);
    const size_t lds = (size_t)k * K * 2;
    if (lds > 160 * 1024) return fail(VL2_E_SHAPE, "%s: k * K * 2 bytes of activations must fit the LDS (k=%d K=%d)", who, k, K);
    const dim3 g((N + 3) / 4, S), b(256);
#define VL2_MOE_DOWN4(KS) do { lds_attr<moe_gemv_down_mxfp4_kernel<KS>>(160 * 1024); \
        hipLaunchKernelGGL((moe_gemv_down_mxfp4_kernel<KS>), g, b, lds, s, (const uint8_t*)q, (long long)q_stride, ldq, (const uint8_t*)scale, \
                           (long long)s_stride, lds_, (const bf16_t*)x, (const int*)ids, wts, (const bf16_t*)res, ldres, (bf16_t*)y, ldy, N, K, E); } while (0)
    if (k == 1) VL2_MOE_DOWN4(1); else if (k == 2) VL2_MOE_DOWN4(2); else if (k == 3) VL2_MOE_DOWN4(3); else VL2_MOE_DOWN4(4);
#undef VL2_MOE_DOWN4
    return launched(who);
}
extern "C" int32_t vl2_moe_gemv_mxfp4(const void* q, int64_t q_stride, int32_t ldq, const void* scale, int64_t s_stride, int32_t lds, const void* x,
                                      const int32_t* ids, const float* wts, const void* res, void* y, int32_t E, int32_t k, int32_t N, int32_t K, float eps,
                                      int32_t flags, void* stream) {
    const int n_out = (flags & VL2_GEMM_SWIGLU) ? N / 2 : N;
    return moe_gemv_mxfp4_rows("vl2_moe_gemv_mxfp4", q, q_stride, ldq, scale, s_stride, lds, x, K, ids, wts, res, n_out, y, n_out, 1, E, k, N, K, eps, flags,
                               stream);
}
extern "C" int32_t vl2_moe_gemv_batched_mxfp4(const void* q, int64_t q_stride, int32_t ldq, const void* scale, int64_t s_stride, int32_t lds, const void* x,
                                              int32_t ldx, const int32_t* ids, const float* wts, const void* res, int32_t ldres, void* y, int32_t ldy,
                                              int32_t S, int32_t E, int32_t k, int32_t N, int32_t K, float eps, int32_t flags, void* stream) {
    return moe_gemv_mxfp4_rows("vl2_moe_gemv_batched_mxfp4", q, q_stride, ldq, scale, s_stride, lds, x, ldx, ids, wts, res, ldres, y, ldy, S, E, k, N, K, eps,
                               flags, stream);
}
extern "C" int32_t vl2_moe_gemm_skinny_mxfp4(const void* A, int32_t lda, int32_t a_rows, const int32_t* rowmap, const void* q, int64_t q_stride, int32_t ldq,
                                             const void* scale, int64_t s_stride, int32_t lds_, void* C, int32_t ldc, const int32_t* counts,
                                             const int32_t* offs, int32_t S, int32_t k, int32_t E, int32_t N, int32_t K, int32_t flags, void* part,
                                             int64_t part_bytes, void* stream) {
    if (!q) return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny_mxfp4: null q (the experts' E2M1 codes)");
    if (!scale) return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny_mxfp4: null scale (the experts' E8M0 block scales)");
    if (!A || !C || !counts || !offs || S <= 0 || k <= 0 || E <= 0 || N <= 0 || K <= 0 || a_rows <= 0)
        return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny_mxfp4: null pointer or empty shape");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "vl2_moe_gemm_skinny_mxfp4: need E <= %d and 1 <= k <= min(E, %d)", MOE_MAX_E, MOE_MAX_K);
    if (S > 64) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_mxfp4: S=%d tokens, need S<=64 (no tiled W4A16 grouped GEMM is built)", S);
    const bool sw = flags & VL2_GEMM_SWIGLU;
    if (flags & ~VL2_GEMM_SWIGLU) return fail(VL2_E_UNSUPP, "vl2_moe_gemm_skinny_mxfp4: flags other than VL2_GEMM_SWIGLU not built");
    if (N % 64 || (sw && N % 128)) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_mxfp4: need N%%64==0 (N%%128==0 with SWIGLU; N=%d)", N);
    if (K % 32 || K > 32704) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_mxfp4: need K%%32==0, K<=32704 (K=%d)", K);
    const int R = S * k;
    if (lda % 8 || ldq % 16 || ldc % 4 || lda < K || ldq < K / 2 || lds_ < K / 32 || q_stride % 16 || q_stride < (int64_t)N * ldq ||
        s_stride < (int64_t)N * lds_ || ldc < (sw ? N / 2 : N) || !ALIGNED16(A) || !ALIGNED16(q) || (((uintptr_t)C) & 7))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_mxfp4: need 16-byte aligned rows, lda%%8==0, ldq%%16==0, ldc%%4==0, lda >= K, ldq >= K/2, lds >= K/32, q_stride%%16==0, q_stride >= N*ldq, s_stride >= N*lds");
    if (a_rows < (rowmap ? S : R)) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_mxfp4: A has %d rows, need %d", a_rows, rowmap ? S : R);
    if (!part || !ALIGNED16(part) || part_bytes <= 0) return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny_mxfp4: needs a 16-byte aligned buffer of fp32 partial sums");
    SkinnyPlan pl;
    if (moe_skinny_plan(S, N, K, pl) != SKINNY_PLAN_OK) return fail(VL2_E_SHAPE, "vl2_moe_gemm_skinny_mxfp4: no K chunking for K=%d", K);
    const int64_t need = (int64_t)pl.ks * R * N * 4;
    if (need > part_bytes)
        return fail(VL2_E_BADARG, "vl2_moe_gemm_skinny_mxfp4: partial buffer too small (%lld bytes, need %lld: the K split is never shrunk)", (long long)part_bytes, (long long)need);
    MoeSkinnyArgsT<Skinny4Args> a{};
    a.g = Skinny4Args{(const bf16_t*)A, (const uint8_t*)q, (const uint8_t*)scale, (float*)part, S, N, K, lda, ldq, lds_, pl.kslice, pl.kchunk};
    a.counts = counts; a.offs = offs; a.rowmap = rowmap; a.w_stride = q_stride; a.s_stride = s_stride; a.R = R; a.a_rows = a_rows;
    hipStream_t s = ST(stream);
    const dim3 gk(N / 64, pl.ks, E), b(256);
    if (pl.mt == 1) { lds_attr<moe_skinny_kernel<1, SkinnyWMx4>>(65536); hipLaunchKernelGGL((moe_skinny_kernel<1, SkinnyWMx4>), gk, b, pl.lds, s, a); }
    else if (pl.mt == 2) { lds_attr<moe_skinny_kernel<2, SkinnyWMx4>>(65536); hipLaunchKernelGGL((moe_skinny_kernel<2, SkinnyWMx4>), gk, b, pl.lds, s, a); }
    else { lds_attr<moe_skinny_kernel<4, SkinnyWMx4>>(65536); hipLaunchKernelGGL((moe_skinny_kernel<4, SkinnyWMx4>), gk, b, pl.lds, s, a); }
    SkinnyReduceArgs r{(const float*)part, C, nullptr, nullptr, R, R, N, pl.ks, ldc, 0, nullptr};
    const dim3 g((R * ((sw ? N / 2 : N) / 4) + 255) / 256);
    if (sw) hipLaunchKernelGGL(moe_skinny_reduce_mxfp4_kernel<true>, g, b, 0, s, r, (const int*)counts, (const int*)offs, E);
    else hipLaunchKernelGGL(moe_skinny_reduce_mxfp4_kernel<false>, g, b, 0, s, r, (const int*)counts, (const int*)offs, E);
    return launched("vl2_moe_gemm_skinny_mxfp4");
}

// ------------------------------------------------------------------------------------------------ tiled W4A16 grouped GEMM, k_moe_gemm4.h
// vl2_moe_gemm on the MXFP4 expert stacks: every check of vl2_moe_gemm, restated for codes and scale bytes, precedes the launch.  The scales
// travel as 1-byte LDS-DMA pieces: lds and s_stride carry no alignment rule.
extern "C" int32_t vl2_moe_gemm_mxfp4(const void* A, int32_t lda, const void* q, int64_t q_stride, int32_t ldq, const void* scale, int64_t s_stride,
                                      int32_t lds_, void* C, int32_t ldc, const float* row_norm, float eps, const int32_t* counts, const int32_t* offs,
                                      int32_t S, int32_t k, int32_t E, int32_t P, int32_t N, int32_t K, int32_t flags, void* stream) {
    if (!q) return fail(VL2_E_BADARG, "vl2_moe_gemm_mxfp4: null q (the experts' E2M1 codes)");
    if (!scale) return fail(VL2_E_BADARG, "vl2_moe_gemm_mxfp4: null scale (the experts' E8M0 block scales)");
    if (!A || !C || !counts || !offs || S <= 0 || k <= 0 || E <= 0 || N <= 0 || K <= 0) return fail(VL2_E_BADARG, "vl2_moe_gemm_mxfp4: null pointer or empty shape");
    if (E > MOE_MAX_E || k > MOE_MAX_K || k > E) return fail(VL2_E_UNSUPP, "vl2_moe_gemm_mxfp4: need E <= %d and 1 <= k <= min(E, %d)", MOE_MAX_E, MOE_MAX_K);
    if (N % GEMM_BN || K % 64 || lda % 8 || ldc % 8 || lda < K || !ALIGNED16(A) || !ALIGNED16(C) || (row_norm && (((uintptr_t)row_norm) & 7)))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm_mxfp4: need N%%%d==0, K%%64==0, 16-byte aligned rows (N=%d K=%d)", GEMM_BN, N, K);
    if (ldq % 16 || ldq < K / 2 || lds_ < K / 32 || q_stride % 16 || q_stride < (int64_t)N * ldq || s_stride < (int64_t)N * lds_ || !ALIGNED16(q))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm_mxfp4: need 16-byte aligned code rows, ldq%%16==0, ldq >= K/2, lds >= K/32, q_stride%%16==0, q_stride >= N*ldq, "
                                 "s_stride >= N*lds (ldq=%d lds=%d)", ldq, lds_);
    if (!moe_rows_ok(S, k, E, P)) return fail(VL2_E_SHAPE, "vl2_moe_gemm_mxfp4: P=%d must be a multiple of %d and >= S*k + E*%d", P, MOE_BM, MOE_BM - 1);
    if ((int64_t)(GEMM_BM - 1) * lda + K >= ((int64_t)1 << 30) || (int64_t)(GEMM_BN - 1) * ldq + K / 2 >= ((int64_t)1 << 30) ||
        (int64_t)(GEMM_BN - 1) * lds_ + K / 32 >= ((int64_t)1 << 30))
        return fail(VL2_E_SHAPE, "vl2_moe_gemm_mxfp4: a tile's rows exceed the kernels' 32-bit buffer offsets");
    const bool sw = flags & VL2_GEMM_SWIGLU;
    if (flags & ~VL2_GEMM_SWIGLU) return fail(VL2_E_UNSUPP, "vl2_moe_gemm_mxfp4: flags other than VL2_GEMM_SWIGLU not built");
    MoeGemm4Args m{};
    GemmArgs& a = m.g;
    a.A = (const bf16_t*)A; a.C = C;
    a.M = P; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc;
    a.stats_out_np = N / 64; a.stats_in_np = K / 64; a.idx_ld = P;
    if (row_norm) { a.norm = VL2_NORM_RMS; a.norm_eps = eps; a.row_norm = row_norm; }
    m.offs = offs; m.counts = counts; m.q = (const uint8_t*)q; m.scale = (const uint8_t*)scale; m.q_stride = q_stride; m.s_stride = s_stride;
    m.ldq = ldq; m.lds = lds_; m.E = E;
    m.rt_cap = P / MOE_BM;
    const dim3 grid((unsigned)(m.rt_cap * (N / GEMM_BN)));
    hipStream_t s = ST(stream);
    if (sw) launch<moe_gemm4_kernel<true>>(grid, dim3(512), MOE4_LDS_BYTES, s, m);
    else launch<moe_gemm4_kernel<false>>(grid, dim3(512), MOE4_LDS_BYTES, s, m);
    return launched("vl2_moe_gemm_mxfp4");
}

#include "vl2_stage.inc"
