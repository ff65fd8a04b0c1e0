"""The sparse-MoE kernels (csrc/k_moe.h, csrc/k_moe_skinny.h: router, scan, gather, grouped GEMM, grouped skinny GEMM, decode gate/up and down
GEMVs, combine) on exact inputs at their edges, on the MI355X: tests/moe_exact.py's case tables through the vl2_moe_* entry points.  The router's
ids are fully determined by integer scores and compared on every row -- exact ties included, no margin mask; the tables against references built
from the reference ids; every fp32 accumulation is exact in any order, so plain outputs, the down projection and the combine equal RNE(fp64) bit
for bit; silu of the SwiGLU forms is held to one step with decode_exact's cap.  Every operand is a strided view of a poisoned allocation and
every output sits in a sentinel frame.  The CPU twins: tests/test_moe_edges_host.py, tests/test_moe_edges_emu.py.  DESIGN.md section 22b."""
import pytest
import torch

from tests import moe_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from videollama2_amd import _lib, ops as o
    _lib.load()
    o.attach_workspace(DEV)
    return o


def _report(errs, n):
    assert not errs, f"{len(errs)} of {n} cases failed:\n" + "\n".join(errs[:12])


def _route(ops, rows):
    errs, n, fig = [], 0, dict(wts=0.0, rstd_ulps=0, logit_ulps=0)
    for row in rows:
        c = X.RouteCase(row)
        e, f = X.check_route(c, X.run_route(ops, c, DEV))
        errs += e
        n += 1
        fig = {k: max(v, f[k]) for k, v in fig.items()}
    print(f"\n  router, {n} cases: largest |wts - fp64| {fig['wts']:.2e} (bound {X.WTS_TOL}), rstd {fig['rstd_ulps']} fp32 steps (bound {X.RSTD_ULPS}), "
          f"logits {fig['logit_ulps']} fp32 steps (bound {X.LOGIT_ULPS})", end="")
    return errs, n


@pytest.mark.parametrize("entry", ("route", "rows", "gemv"))
def test_router_edges(ops, entry):
    _report(*_route(ops, [r for r in X.route_table() if r.entry == entry]))


def test_router_refusals_leave_every_sentinel_alone(ops):
    """The refusals go through the ABI's argument checks only: nothing is launched."""
    errs = [e for e in (X.run_route_refusal(ops, r, DEV) for r in X.ROUTE_REFUSALS) if e]
    _report(errs, len(X.ROUTE_REFUSALS))


def _approx(tag, cases, run, check):
    errs, n, nd, tot, worst = [], 0, 0, 0, 0.0
    for c in cases:
        res = run(c)
        e, d = check(c, *res) if isinstance(res, tuple) else check(c, res)
        n += 1
        if e:
            errs.append(e)
        elif getattr(c, "swiglu", True):
            nd, tot, worst = nd + d, tot + c.R * c.n_out, max(worst, d / max(1, c.R * c.n_out))
    if tot:
        print(f"\n  {tag} SwiGLU: {nd} of {tot} outputs one step from RNE of the fp64 value ({nd / tot:.2e}); largest share of a case {worst:.2e}, cap 1.00e-02", end="")
    return errs, n


def test_grouped_gemm_edges(ops):
    cases = [X.GemmCase(r) for r in X.gemm_table()]
    _report(*_approx("grouped GEMM", cases, lambda c: X.run_gemm(ops, c, DEV), X.check_gemm))
    sh = [c.rounding_share() for c in cases if not c.swiglu]
    print(f"\n  grouped GEMM plain: {sum(s for s, _ in sh) / len(sh):.2f} of the outputs need the rounding, {sum(t for _, t in sh)} exact ties", end="")


def test_grouped_skinny_gemm_edges(ops):
    _report(*_approx("grouped skinny GEMM", [X.SkinnyCase(r) for r in X.skinny_table()], lambda c: X.run_skinny(ops, c, DEV), X.check_skinny))


def test_decode_gate_up_edges(ops):
    cases = [X.GateUpCase(1, *a, False) for a in X.GU_CASES] + [X.GateUpCase(*a, True) for a in X.GU_BATCHED]
    _report(*_approx("decode gate/up", cases, lambda c: X.run_gate_up(ops, c, DEV), X.check_gate_up))


def test_decode_down_edges(ops):
    cases = [X.DownCase(r) for r in X.down_table()] + [X.DownCase.order_case()]
    errs = [e for e in (X.check_down(c, X.run_down(ops, c, DEV)) for c in cases) if e]
    errs += [e for e in (X.run_down_refusal(ops, r, DEV) for r in X.DOWN_REFUSALS) if e]
    sh = [c.rounding_share() for c in cases[:-1]]
    print(f"\n  decode down: {sum(s for s, _ in sh) / len(sh):.2f} of the outputs need the rounding, {sum(t for _, t in sh)} exact ties", end="")
    _report(errs, len(cases) + len(X.DOWN_REFUSALS))


def test_combine_edges(ops):
    errs, worst, cases = [], 0, [X.CombineCase(r) for r in X.combine_table()]
    for c in cases:
        e, d = X.check_combine(c, *X.run_combine(ops, c, DEV))
        worst = max(worst, d)
        if e:
            errs.append(e)
    print(f"\n  combine: {sum(c.rounding_count() for c in cases)} outputs need the rounding; rstd of the stored row {worst} fp32 steps (bound {X.RSTD_ULPS})", end="")
    _report(errs, len(cases))


def test_reduced_tables_on_the_fp16_build(ops):
    """+-4 and the small integers are exact in fp16 too: one pass of a reduced table on the fp16 library (the order case is bf16's own)."""
    from videollama2_amd import _lib
    errs, n = [], 0
    _lib.set_elem("fp16")
    try:
        _lib.load()
        rt = X.route_table()
        pick = [r for r in rt if (r.S, r.mode) in ((65, "ties"), (37, "free"))][::4] + [r for r in rt if r.mode == "counts" and r.arg == "tile_edges"] + \
               [r for r in rt if r.entry == "gemv"][:3]
        e, m = _route(ops, pick)
        errs, n = errs + e, n + m
        for c in [X.GemmCase(r) for r in X.gemm_table()[9:12]]:
            errs.append(X.check_gemm(c, X.run_gemm(ops, c, DEV))[0])
        for c in [X.SkinnyCase(r) for r in X.skinny_table()[4:8]]:
            errs.append(X.check_skinny(c, *X.run_skinny(ops, c, DEV))[0])
        for c in [X.GateUpCase(1, *X.GU_CASES[3], False), X.GateUpCase(*X.GU_BATCHED[2], True)]:
            errs.append(X.check_gate_up(c, X.run_gate_up(ops, c, DEV))[0])
        for c in [X.DownCase(r) for r in X.down_table()[::7]]:
            errs.append(X.check_down(c, X.run_down(ops, c, DEV)))
        for c in [X.CombineCase(r) for r in X.combine_table()[4:12:2]]:
            errs.append(X.check_combine(c, *X.run_combine(ops, c, DEV))[0])
        n += 3 + 4 + 2 + len(X.down_table()[::7]) + 4
    finally:
        _lib.set_elem("bf16")
    _report([e for e in errs if e], n)
