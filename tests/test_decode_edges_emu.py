"""The exact-input edge cases of tests/decode_exact.py on the CPU: the helper proven (guard, three summation orders, quantisers, the references
alone), the skinny case table held against skinny_plan.h, and the same case tables as tests/test_gpu_decode_edges.py through the host emulator
build of the kernel sources (tests/emu) for the entry points it has: 16-bit and fp8 weights, single-row, batched and skinny.  DESIGN.md section 15."""
import ctypes
import os
import subprocess

import pytest
import torch

from tests import decode_exact as E
from tests import mxfp4_oracle as M4
from tests.emu.backend import emulated_backend

EMU_FORMATS = ("b16", "fp8")            # the emulator has no MXFP4 entry points
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Cases the emulator is too slow for (every one of them runs in tests/test_gpu_decode_edges.py): nothing else is dropped.
EMU_DROPPED_GEMV = lambda K, N, epi: K > 8208 and N > 64                                # the K = 32704 rows of the widest SwiGLU blocks
# the emulator's batched launchers take 3 (16-bit) / 4 (fp8) rows per launch whatever K is -- they do not restate the product's LDS split, which
# therefore runs on the GPU only -- and 3 rows of K = 32704 do not fit the emulator's own 160 KiB LDS array
EMU_DROPPED_BATCHED = lambda MB, K, N, epi: K > 16384
EMU_DROPPED_SKINNY = lambda M, N, K, epi: N == 8192 and M not in (1, 17, 64)            # the wide-N row at three of its seven M
EMU_PROBE_K = {"b16": (8, 72, 2056), "fp8": (16, 1040)}                                 # a K x K identity per probe: the larger K run on the GPU only


def _run(cases, make):
    errs, n = [], 0
    with emulated_backend():
        from videollama2_amd import ops
        for cs in cases:
            c = make(*cs)
            err, _ = E.check_case(c, E.run_case(ops, c, "cpu"))
            n += 1
            if err:
                errs.append(err)
    assert not errs, f"{len(errs)} of {n} cases failed:\n" + "\n".join(errs[:12])


# ------------------------------------------------------------------------------------------------------------ the helper itself
def test_guard_fires_when_a_range_is_widened():
    E.Case("fp8", "gemv", 1, 34, 32704, "plain")                        # the narrowed ranges hold at the largest K
    with pytest.raises(AssertionError, match="exactness guard"):
        E.Case("fp8", "gemv", 1, 34, 32704, "plain", wide=True)         # x in [-8, 8] and row scales 2^-3 .. 2^2 do not
    with pytest.raises(AssertionError, match="not a multiple"):
        E.guard(torch.tensor([[1.5]], dtype=torch.float64), torch.ones(1, 1, dtype=torch.float64), None, None, 1.0, 1.0)


@pytest.mark.parametrize("fmt", E.FORMATS)
def test_every_case_of_the_tables_passes_the_guard_and_three_fp32_orders_give_the_reference(fmt):
    ks = E.GEMV_K[fmt]
    for K, N in ((ks[0], E.GEMV_N[fmt][-1]), (ks[1], E.GEMV_N[fmt][2]), (ks[3], E.GEMV_N[fmt][-1]), (ks[-1], E.GEMV_N[fmt][1])):
        for epi in ("plain", "norm_w"):
            c = E.Case(fmt, "gemv", 1, N, K, epi)
            assert c.bound < 2 ** 24 and c.quantum >= 2.0 ** -20
            assert E.three_orders_exact(c), c.coords()
    c = E.Case(fmt, "gemv", 1, 64, ks[2], "swiglu")                     # the gate and up sums of a SwiGLU case are exact too
    assert E.three_orders_exact(c) and c.quantum >= 2.0 ** -20
    assert float(c.g.abs().max()) <= 16.0 and float(c.g.abs().max()) > 2.0, "gate sums should spread over about +-8"


def test_fp8_quantiser_reproduces_the_integer_weights():
    """The hand-built codes and row scales against the product's own quantiser (k_fp8.h, here through the emulator): dequant(quant(W)) == W."""
    from oracle import fp8_oracle as F8
    W = E.Weights("fp8", 34, 1040, torch.Generator().manual_seed(1))
    with emulated_backend():
        from videollama2_amd import ops
        q, sc = ops.quant_fp8(W.w64.bfloat16().contiguous())
    assert torch.equal(F8.dequant(q, sc).double(), W.w64)
    assert torch.equal(F8.dequant(W.store["q"][:34, :1040], W.store["scale"][:34]).double(), W.w64)


def test_mxfp4_quantiser_reproduces_the_hand_built_weights():
    """The hand-built codes and block scales against the quantiser's definition (tests/mxfp4_oracle.py, which the device quantiser is held to bit
    for bit; the device itself: tests/test_gpu_decode_edges.py)."""
    W = E.Weights("mx4", 34, 2080, torch.Generator().manual_seed(1))
    q, s = M4.quant_blocks(W.w64.bfloat16())
    assert torch.equal(M4.dequant(q, s).double(), W.w64)
    sb = W.store["s"][:34, :65].to(torch.int64)
    assert bool((sb[:, 1:] != sb[:, :-1]).all()), "neighbouring blocks must carry different scales"


def test_fp8_pair_rows_carry_different_scales():
    for sw in (False, True):
        sc = E.Weights("fp8", 192, 16, torch.Generator().manual_seed(2), swiglu=sw).scale
        n = torch.arange(192)
        first = n[(n % 64) < 32] if sw else n[n % 2 == 0]
        assert bool((sc[first] != sc[first + (32 if sw else 1)]).all())


def test_references_alone_stay_inside_the_one_ulp_rules(capsys):
    """torch fp32 against fp64 on the same inputs: the share of outputs off by one bf16 step (never more), for the SwiGLU epilogue and the probe."""
    nd = tot = 0
    for fmt in E.FORMATS:
        for K, N, epi in E.gemv_cases(fmt):
            if E.EPILOGUES[epi][1] and K <= 8208:
                c = E.Case(fmt, "gemv", 1, N, K, epi)
                d, mx = E.swiglu_reference_share(c)
                assert mx <= 1 and d <= E.swiglu_cap(c), (c.coords(), d, mx)
                nd, tot = nd + d, tot + c.n_out
    with capsys.disabled():
        print(f"\nSwiGLU, torch fp32 against fp64: {nd} of {tot} outputs differ by one bf16 step ({nd / tot:.2e})")
    nd = tot = 0
    for K in (8, 72, 2056, 4096, 4104, 8192):
        for seed in range(4):
            x, nw = E.probe_inputs(K, rows=4, seed=seed)
            for w in (nw, None):
                d = E.ulp_distance(E.probe_reference_fp32(x, w), E.probe_reference(x, w))
                assert int(d.max()) <= 1 and int((d > 0).sum(dim=1).max()) <= E.probe_cap(K)
                nd, tot = nd + int((d > 0).sum()), tot + d.numel()
    with capsys.disabled():
        print(f"staged-x probe, torch fp32 against fp64: {nd} of {tot} elements differ by one bf16 step ({nd / tot:.2e})")


# ------------------------------------------------------------------------------------------------------------ the skinny table
def test_skinny_plan_transcription_matches_the_header(tmp_path):
    src = tmp_path / "plan.cpp"
    src.write_text('#include "skinny_plan.h"\nextern "C" int plan(int M, int N, int K, long long ws, int shrink, int* o) { SkinnyPlan p;\n'
                   "int rc = skinny_plan(M, N, K, ws, shrink != 0, p); o[0] = p.mt; o[1] = p.ks; o[2] = p.kslice; o[3] = p.kchunk; return rc; }\n")
    so = tmp_path / "plan.so"
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.run([cxx if os.path.exists(cxx) else "c++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "videollama2_amd", "csrc"),
                    str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    o = (ctypes.c_int * 4)()
    for N, K, _ in E.SKINNY_NK:
        for M in E.SKINNY_M:
            # the quantised entries' call (no shrink), and the 16-bit entry's (shrink) with an ample and with a tight workspace (2 MiB: the
            # widest rows must give up part of their split)
            for ws, shrink in ((1 << 40, False), (1 << 40, True), (1 << 21, True)):
                assert lib.plan(M, N, K, ws, int(shrink), o) == 0
                p = E.skinny_plan(M, N, K, ws, shrink)
                assert list(o) == [p["mt"], p["ks"], p["kslice"], p["kchunk"]], (M, N, K, ws, shrink, list(o), p)
    assert E.skinny_plan(64, 8192, 64, 1 << 21, True)["ks"] < E.skinny_plan(64, 8192, 64)["ks"]      # the tight workspace does bite


def test_skinny_table_reaches_every_regime_of_the_plan():
    """A later change to skinny_plan() cannot silently hollow the table out.  (The plan of the quantised entries; the 16-bit entry may shrink the
    split to its workspace, and tests/test_gpu_decode_edges.py asserts that the library's workspace is large enough for it never to do so here.)"""
    plans = [E.skinny_plan(M, N, K) for M, N, K, _ in E.skinny_cases()]
    assert {p["mt"] for p in plans} == {1, 2, 4}
    assert {p["ks"] for p in plans} >= {1, 2, 3, 32}
    chunks = {p["kslice"] // p["kchunk"] for p in plans}
    assert 1 in chunks and any(c > 1 for c in chunks)
    steps = {p["kchunk"] // 32 for p in plans}
    for nl in (8, 16):
        assert 1 in steps and nl in steps, (nl, sorted(steps))
        assert any(1 < s < nl for s in steps), (nl, sorted(steps))
        assert any(s > nl and s % nl for s in steps), (nl, sorted(steps))
    assert set(E.NL.values()) == {8, 16}


# ------------------------------------------------------------------------------------------------------------ the case tables on the emulator
@pytest.mark.parametrize("fmt", EMU_FORMATS)
def test_gemv_edges_on_the_emulator(fmt):
    _run([c for c in E.gemv_cases(fmt) if not EMU_DROPPED_GEMV(*c)], lambda K, N, e: E.Case(fmt, "gemv", 1, N, K, e))


@pytest.mark.parametrize("fmt", EMU_FORMATS)
def test_batched_gemv_edges_on_the_emulator(fmt):
    _run([c for c in E.batched_cases(fmt) if not EMU_DROPPED_BATCHED(*c)], lambda MB, K, N, e: E.Case(fmt, "batched", MB, N, K, e))


@pytest.mark.parametrize("fmt", EMU_FORMATS)
def test_skinny_edges_on_the_emulator(fmt):
    _run([c for c in E.skinny_cases() if not EMU_DROPPED_SKINNY(*c)], lambda M, N, K, e: E.Case(fmt, "skinny", M, N, K, e))


@pytest.mark.parametrize("fmt", EMU_FORMATS)
def test_staged_x_probe_on_the_emulator(fmt):
    errs = []
    with emulated_backend():
        from videollama2_amd import ops
        for K in EMU_PROBE_K[fmt]:
            x, nw = E.probe_inputs(K)
            for w in (nw, None):
                err, _, _ = E.probe_check(fmt, K, E.probe_collect(ops, fmt, K, x, w, "cpu"), x, w)
                if err:
                    errs.append(err)
    assert not errs, "\n".join(errs)
