"""The decode projections (GEMV, multi-row GEMV, skinny-M GEMM; 16-bit, fp8 and MXFP4 weights) on exact inputs at the edges of their launch
plans, on the MI355X: tests/decode_exact.py's case tables through the C ABI.  fp32 accumulation is exact in any order on these inputs, so every
projection output equals the fp64 reference bit for bit -- `torch.equal`, no tolerance; the only approximate pieces are silu in the SwiGLU
epilogue and the statistic of the RMSNorm prologue, held to one bf16 step with the caps `swiglu_cap` / `probe_cap`.  Every operand is a strided
view of a poisoned allocation and every output sits inside a sentinel frame.  DESIGN.md section 15; measured figures: profiles/r13_decode_edges.md."""
import pytest
import torch

from tests import decode_exact as E
from tests import mxfp4_oracle as M4

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from videollama2_amd import _lib, ops as o
    _lib.load()
    o.attach_workspace(DEV)
    return o


def _run(ops, cases, make):
    errs, n, sw_diff, sw_tot, worst = [], 0, 0, 0, (0.0, "")
    for cs in cases:
        c = make(*cs)
        out = E.run_case(ops, c, DEV)
        err, nd = E.check_case(c, out)
        n += 1
        if c.swiglu:
            print(f"\n  {c.coords()}: {nd} of {c.n_out * c.R} outputs one bf16 step from RNE(silu(g) u + res) ({nd / (c.n_out * c.R):.2e})", end="")
            sw_diff, sw_tot = sw_diff + nd, sw_tot + c.n_out * c.R
            if nd / (c.n_out * c.R) > worst[0]:
                worst = (nd / (c.n_out * c.R), c.coords())
        if err:
            errs.append(err)
    if sw_tot:
        print(f"\nSwiGLU outputs one bf16 step from RNE(silu(g) u + res): {sw_diff} of {sw_tot} ({sw_diff / sw_tot:.2e}); largest share of a case "
              f"{worst[0]:.2e} {worst[1]}")
    assert not errs, f"{len(errs)} of {n} cases failed:\n" + "\n".join(errs[:16])


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_gemv_edges(ops, fmt):
    _run(ops, E.gemv_cases(fmt), lambda K, N, e: E.Case(fmt, "gemv", 1, N, K, e))


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_batched_gemv_edges(ops, fmt):
    _run(ops, E.batched_cases(fmt), lambda MB, K, N, e: E.Case(fmt, "batched", MB, N, K, e))


def test_workspace_never_shrinks_the_16bit_skinny_split_of_the_table(ops):
    """vl2_gemm_skinny_bf16 alone may shrink the K split to its workspace; with the library's workspace it must not on any row of the table, or
    test_skinny_edges[b16] would not reach the regimes tests/test_decode_edges_emu.py asserts for the table."""
    ws = ops.attach_workspace(DEV).numel()
    for M, N, K, _ in E.skinny_cases():
        free = E.skinny_plan(M, N, K)
        assert free["ws_need"] <= ws and E.skinny_plan(M, N, K, ws, True) == free, (M, N, K, ws, free)


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_skinny_edges(ops, fmt):
    _run(ops, E.skinny_cases(), lambda M, N, K, e: E.Case(fmt, "skinny", M, N, K, e))


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_staged_x_probe(ops, fmt):
    """Identity weights and fp32 output return the staged x of every kernel that stages one: bit-identical across the kernels of the format and
    across the formats (the x-first kernel is the one restatement of gemv_stage_x), and one bf16 step at most from the fp64 RMSNorm."""
    errs, nd, tot = [], 0, 0
    for K in E.PROBE_K[fmt]:
        x, nw = E.probe_inputs(K)
        for w in (nw, None):
            probes = E.probe_collect(ops, fmt, K, x, w, DEV)
            err, d, t = E.probe_check(fmt, K, probes, x, w)
            nd, tot = nd + d, tot + t
            if err:
                errs.append(err)
            if fmt != "b16" and K % 32 == 0 and K in E.PROBE_K["b16"]:      # the same x through the 16-bit kernels: the same staged bits
                other = E.probe_collect(ops, "b16", K, x, w, DEV, batched=(2,))["single"]
                if not torch.equal(other.view(torch.int16), probes["single"].view(torch.int16)):
                    errs.append(f"{fmt} K={K}: staged x differs from the 16-bit kernels'")
        torch.cuda.empty_cache()
    print(f"\nstaged-x probe {fmt}: {nd} of {tot} elements one bf16 step from the fp64 RMSNorm ({nd / max(tot, 1):.2e})")
    assert not errs, "\n".join(errs)


def test_device_quantisers_reproduce_the_hand_built_weights(ops):
    from oracle import fp8_oracle as F8
    W = E.Weights("fp8", 34, 1040, torch.Generator().manual_seed(1))
    q, sc = ops.quant_fp8(W.w64.bfloat16().to(DEV))
    assert torch.equal(F8.dequant(q.cpu(), sc.cpu()).double(), W.w64)
    W = E.Weights("mx4", 34, 2080, torch.Generator().manual_seed(1))
    q, s = ops.quant_mxfp4(W.w64.bfloat16().to(DEV))
    assert torch.equal(M4.dequant(q, s).double(), W.w64)


def test_rejections_at_the_edges_leave_the_output_untouched(ops):
    """Host checks only (vl2_abi.hip: every check precedes every launch): each call raises Vl2HipError and writes nothing."""
    from videollama2_amd import _lib
    p, st = ops._p, ops._stream
    ws = ops.attach_workspace(DEV)
    SW, MB = E.GEMM_SWIGLU, 2
    calls = []

    def bufs(N, K, rows):
        ld = (K + 15) // 16 * 16
        return dict(w=torch.zeros(N * ld * 2 + 64, dtype=torch.uint8, device=DEV), sc=torch.ones(N, dtype=torch.float32, device=DEV),
                    s8=torch.full((N * (K // 32 + 1),), 127, dtype=torch.uint8, device=DEV), x=torch.zeros(rows * ld + 64, dtype=torch.bfloat16, device=DEV),
                    y=torch.full((rows * (N + 8),), E.SENTINEL, dtype=torch.float32, device=DEV), ld=ld)

    def gemv(fmt, N, K, flags, why):
        for batched in (False, True):
            b = bufs(N, K, MB)
            ld, lds = b["ld"], K // 32 + 1
            tail = (MB, N, K, ld, ld, N + 8, N + 8, E.EPS, flags, st()) if batched else (N, K, ld, E.EPS, flags, st())
            name = {"b16": "vl2_gemv_bf16", "fp8": "vl2_gemv_fp8", "mx4": "vl2_gemv_mxfp4"}[fmt]
            name = name.replace("gemv_", "gemv_batched_") if batched else name
            head = {"b16": (p(b["w"]),), "fp8": (p(b["w"]), p(b["sc"])), "mx4": (p(b["w"]), p(b["s8"]), lds)}[fmt]
            calls.append((f"{name} N={N} K={K} flags={flags}: {why}", name, head + (p(b["x"]), None, None, None, p(b["y"])) + tail, b))

    def skinny(fmt, M, N, K, flags, why):
        b = bufs(N, K, M)
        ld, lds = b["ld"], K // 32 + 1
        name = {"b16": "vl2_gemm_skinny_bf16", "fp8": "vl2_gemm_skinny_fp8", "mx4": "vl2_gemm_skinny_mxfp4"}[fmt]
        head = {"b16": (p(b["x"]), p(b["w"])), "fp8": (p(b["x"]), p(b["w"]), p(b["sc"])), "mx4": (p(b["x"]), p(b["w"]), p(b["s8"]), lds)}[fmt]
        calls.append((f"{name} M={M} N={N} K={K} flags={flags}: {why}", name,
                      head + (p(b["y"]), None, None, M, N, K, ld, ld, N + 8, N + 8, flags, p(ws), ws.numel(), st()), b))

    for fmt in E.FORMATS:
        gemv(fmt, 2, 32712, 0, "K above 32704")       # (fp8 and MXFP4 refuse this one for its alignment: their limit itself is the next two)
        gemv(fmt, 96, 64, SW, "SwiGLU needs N % 64 == 0")
        skinny(fmt, 65, 64, 32, 0, "M above 64")
        skinny(fmt, 1, 96, 32, 0, "N % 64")
        skinny(fmt, 1, 64, 48, 0, "K % 32")
        skinny(fmt, 1, 192, 32, SW, "SwiGLU needs N % 128 == 0")
    gemv("fp8", 2, 32720, 0, "K above 32704, K % 16 == 0")
    gemv("mx4", 2, 32736, 0, "K above 32704, K % 32 == 0")
    gemv("fp8", 3, 16, 0, "odd N")
    gemv("fp8", 2, 24, 0, "K % 16")
    gemv("mx4", 2, 48, 0, "K % 32")
    for what, name, args, b in calls:
        with pytest.raises(_lib.Vl2HipError):
            _lib.call(name, *args)
            pytest.fail(f"accepted: {what}")
        torch.cuda.synchronize()
        assert bool((b["y"] == E.SENTINEL).all()), f"output written: {what}"
