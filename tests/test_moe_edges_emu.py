"""The exact-input edge cases of tests/moe_exact.py through the host emulator build of the kernel sources (tests/emu: csrc/k_moe.h and
csrc/k_moe_skinny.h behind launchers that restate vl2_abi.hip's argument checks): the same tables as tests/test_gpu_moe_edges.py, on the CPU.
Cases the emulator is too slow for are dropped by the named predicates below, with the reason, and by nothing else; every dropped case runs in
tests/test_gpu_moe_edges.py.  DESIGN.md section 22b."""
import pytest

from tests import moe_exact as X
from tests.emu.backend import emulated_backend

DEV = "cpu"

# the router runs one fiber per lane and a rendezvous per shuffle: S (1 + E) wave sums.  Dropped: the two S k = 16384 rows of each entry (the
# gather launch alone is 17408 workgroups) and the E >= 63 rows of more than 1024 tokens
EMU_DROPPED_ROUTE = lambda r: r.S * r.k == X.MOE_SCAN_MAX or (r.E >= 63 and r.S > 1024)
# the grouped GEMM: an emulated 128 x 128 x 64 step of the 16 x 16 x 32 MFMA costs milliseconds.  Dropped: the E = 64 rotations but three (one
# per epilogue) and K = 1088 at more than one column tile
EMU_DROPPED_GEMM = lambda i, r: (r.E == 64 and i % 9 >= 3) or (r.K == 1088 and r.N > 128)
# the grouped skinny GEMM at N = 1024 launches 16 x 16 x E workgroups: kept at S = 5 and 64 only
EMU_DROPPED_SKINNY = lambda r: r.N == 1024 and r.S not in (5, 64)
# the decode GEMVs: the K = 20480 rows stage 160 KiB per workgroup through one fiber per lane; the single-token one is kept, the batched one dropped
EMU_DROPPED_DOWN = lambda r: r.K == X.DOWN_K_LDS and r.batched


def _report(errs, n):
    assert not errs, f"{len(errs)} of {n} cases failed:\n" + "\n".join(errs[:12])


@pytest.mark.parametrize("entry", ("route", "rows", "gemv"))
def test_router_edges_on_the_emulator(entry):
    errs, n = [], 0
    with emulated_backend():
        from videollama2_amd import ops
        for row in X.route_table():
            if row.entry != entry or EMU_DROPPED_ROUTE(row):
                continue
            c = X.RouteCase(row)
            e, _ = X.check_route(c, X.run_route(ops, c, DEV))
            errs += e
            n += 1
    _report(errs, n)


def test_router_refusals_on_the_emulator():
    with emulated_backend():
        from videollama2_amd import ops
        errs = [e for e in (X.run_route_refusal(ops, r, DEV) for r in X.ROUTE_REFUSALS) if e]
    _report(errs, len(X.ROUTE_REFUSALS))


def test_grouped_gemm_edges_on_the_emulator():
    errs, n = [], 0
    with emulated_backend():
        from videollama2_amd import ops
        for i, row in enumerate(X.gemm_table()):
            if EMU_DROPPED_GEMM(i, row):
                continue
            c = X.GemmCase(row)
            e, _ = X.check_gemm(c, X.run_gemm(ops, c, DEV))
            n += 1
            if e:
                errs.append(e)
    _report(errs, n)


def test_grouped_skinny_gemm_edges_on_the_emulator():
    errs, n = [], 0
    with emulated_backend():
        from videollama2_amd import ops
        for row in X.skinny_table():
            if EMU_DROPPED_SKINNY(row):
                continue
            c = X.SkinnyCase(row)
            e, _ = X.check_skinny(c, *X.run_skinny(ops, c, DEV))
            n += 1
            if e:
                errs.append(e)
    _report(errs, n)


def test_decode_gate_up_edges_on_the_emulator():
    errs, n = [], 0
    with emulated_backend():
        from videollama2_amd import ops
        cases = [X.GateUpCase(1, *a, False) for a in X.GU_CASES] + [X.GateUpCase(*a, True) for a in X.GU_BATCHED]
        for c in cases:
            e, _ = X.check_gate_up(c, X.run_gate_up(ops, c, DEV))
            n += 1
            if e:
                errs.append(e)
    _report(errs, n)


def test_decode_down_edges_on_the_emulator():
    errs, n = [], 0
    with emulated_backend():
        from videollama2_amd import ops
        cases = [X.DownCase(r) for r in X.down_table() if not EMU_DROPPED_DOWN(r)] + [X.DownCase.order_case()]
        for c in cases:
            e = X.check_down(c, X.run_down(ops, c, DEV))
            n += 1
            if e:
                errs.append(e)
        errs += [e for e in (X.run_down_refusal(ops, r, DEV) for r in X.DOWN_REFUSALS) if e]
    _report(errs, n)


def test_combine_edges_on_the_emulator():
    errs, n = [], 0
    with emulated_backend():
        from videollama2_amd import ops
        for row in X.combine_table():
            c = X.CombineCase(row)
            e, _ = X.check_combine(c, *X.run_combine(ops, c, DEV))
            n += 1
            if e:
                errs.append(e)
    _report(errs, n)
