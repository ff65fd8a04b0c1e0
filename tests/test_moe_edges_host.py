"""tests/moe_exact.py proven on the CPU before anyone trusts it: the guards fire, fp32 sums in other orders give the fp64 references, the
generators do what they state, the references alone stay inside every bound the GPU test applies, and the case tables cover what their comments
claim and agree with the header and with ops.moe_rows.  No GPU, no emulator.  DESIGN.md section 22b."""
import os
import re

import pytest
import torch

from tests import decode_exact as D
from tests import moe_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE = X.route_table()


def _sum_orders(prod):
    """prod fp32 [n, K] -> the row sums in fp32, sequentially forwards, backwards and in a random permutation (every prefix rounded)."""
    K = prod.shape[1]
    g = torch.Generator().manual_seed(5)
    return [torch.cumsum(prod[:, o], 1, dtype=torch.float32)[:, -1] for o in (torch.arange(K), torch.arange(K - 1, -1, -1), torch.randperm(K, generator=g))]


# ------------------------------------------------------------------------------------------------------------ the guards
def test_guards_fire_when_a_range_is_widened(monkeypatch):
    X.GemmCase(X.GRow(8, (129, 1, 0, 33, 0, 0, 0, 0), 128, 1088, "plain"))
    with pytest.raises(AssertionError, match="exactness guard"):
        X.GemmCase(X.GRow(8, (129, 1, 0, 33, 0, 0, 0, 0), 128, 1088, "plain"), wide=True)
    X.DownCase(X.DRow(1, 4, 4, 5, X.DOWN_K_LDS, True))                     # the narrowed range holds at the largest K
    with pytest.raises(AssertionError, match="exactness guard"):
        X.DownCase(X.DRow(1, 4, 4, 5, X.DOWN_K_LDS, True), wide=True)
    with pytest.raises(AssertionError, match="not a multiple"):
        D.guard(torch.tensor([[1.5]], dtype=torch.float64), torch.ones(1, 1, dtype=torch.float64), None, None, 1.0, 1.0)
    X.RouteCase(X.RRow("route", 37, 8, 2, "free", 4096))
    monkeypatch.setattr(X, "FREE_NNZ", 64)                                 # 64 nonzero router columns: scores up to +-256
    with pytest.raises(AssertionError, match="logit spread"):
        X.RouteCase(X.RRow("route", 37, 8, 2, "free", 4096))


def test_the_order_case_is_what_its_docstring_says():
    """Slot order gives RNE of the exact value, the reverse order the other neighbour -- worked in fp32 on the CPU."""
    c = X.DownCase.order_case()
    w, d = c.wts.float()[0], c.dots.float()[0, :, 0]
    assert torch.equal(d.double(), c.dots[0, :, 0]) and torch.equal(w.double(), c.wts[0])
    fma = lambda a, b, o: (a.double() * b.double() + o.double()).float()  # one rounding: the products and sums here are exact in fp64
    zero = torch.zeros((), dtype=torch.float32)
    fwd = fma(w[1], d[1], fma(w[0], d[0], zero))
    rev = fma(w[0], d[0], fma(w[1], d[1], zero))
    assert fwd.bfloat16().item() == 1.0078125 == c.expected()[0, 0].item() and rev.bfloat16().item() == 1.0


# ------------------------------------------------------------------------------------------------------------ order independence
def test_three_fp32_orders_give_the_router_scores():
    for row in ROUTE[::7]:
        if row.S > 1100:
            continue
        c = X.RouteCase(row)
        x, wr = c.x.float(), c.wr.float()
        for e in range(0, c.E, max(1, c.E // 4)):
            for s in _sum_orders(x * wr[e][None, :]):
                assert torch.equal(s.double(), c.sc[:, e].double()), c.coords()
        for s in _sum_orders(x * x):
            assert bool((s == 16.0 * c.D).all())


def test_three_fp32_orders_give_the_gemm_and_gemv_references():
    for row in X.gemm_table()[::5]:
        c = X.GemmCase(row)
        a, w = c.a64.float(), c.w64.float()
        for i in (0, c.R // 2, c.R - 1):
            r = int(c.rows[i])
            for n in (0, c.N - 1):
                for s in _sum_orders((a[r] * w[int(c.owner[r]), n])[None, :]):
                    assert s.double().item() == c.acc[i, n].item(), c.coords()
    for row in X.down_table()[::6]:
        c = X.DownCase(row)
        a, w = c.store["a"][:c.S * c.k, :c.K], c.store["w"][:, :c.N, :c.K]
        for t in range(c.S):
            for j in range(c.k):
                for s in _sum_orders((w[c.ids[t, j], c.N - 1] * a[t * c.k + j])[None, :]):
                    assert s.double().item() == c.dots[t, j, c.N - 1].item(), c.coords()
            # the slot-order fma chain and its reverse, in fp32: dyadic weights make every step exact
            o = r = torch.zeros(c.N, dtype=torch.float32)
            for j in range(c.k):
                o = c.wts[t, j].float() * c.dots[t, j].float() + o
                r = c.wts[t, c.k - 1 - j].float() * c.dots[t, c.k - 1 - j].float() + r
            res = c.res[t].float() if c.res is not None else 0.0
            assert torch.equal((o + res).double(), c.ref[t]) and torch.equal((r + res).double(), c.ref[t]), c.coords()
    for row in X.combine_table()[::3]:
        c = X.CombineCase(row)
        for t in range(c.S):
            acc = torch.zeros(c.D, dtype=torch.float32)
            for j in range(c.k):
                acc = c.wts[t, j].float() * c.y[c.inv[t, j]].float() + acc
            assert torch.equal((c.x1[t].float() + acc).double(), c.ref[t]), c.coords()
            st = c.expected()[t].float()
            for s in _sum_orders((st * st)[None, :]):
                assert s.double().item() == float((st.double() ** 2).sum()), c.coords()


# ------------------------------------------------------------------------------------------------------------ the generators
def test_planted_generator_reproduces_its_table_and_free_generator_meets_its_tie_share():
    tied = 0
    for row in ROUTE:
        if row.S > 1100:
            continue
        c = X.RouteCase(row)
        assert c.spread <= 64, c.coords()                                  # the logit-spread bound, on every case
        if row.mode != "free":
            assert torch.equal(c.ids, c.want), c.coords()
        else:
            assert c.tied_rows >= X.FREE_TIE_SHARE, (c.coords(), c.tied_rows)
        if row.mode == "ties":
            assert c.tied_rows > 0 or row.arg in ("pair", "chosen"), c.coords()
            if row.arg in ("chosen", "all"):
                assert bool(c.chosen_tie.all())
            if row.arg == "all":
                assert torch.equal(c.ids, torch.arange(c.k)[None, :].expand(c.S, c.k))
            tied += 1
        if row.mode == "counts":
            vec = (X.COUNT_VECTORS_ROWS if row.entry == "rows" else X.COUNT_VECTORS)[row.arg][0]
            assert c.counts.tolist() == list(vec), c.coords()
    assert tied >= 20


def test_a_planted_table_that_breaks_the_tie_rule_is_rejected():
    g = torch.Generator().manual_seed(1)
    with pytest.raises(AssertionError, match="does not follow"):
        X.planted(torch.tensor([[5, 2]]), 8, g, levels=(6, 6), rest=-2)    # equal scores: the lower index must come first
    X.planted(torch.tensor([[2, 5]]), 8, g, levels=(6, 6), rest=-2)


def test_reference_tables_on_a_hand_worked_example():
    ids = torch.tensor([[2, 0], [0, 1], [2, 1]])
    counts, offs, gather, inv = X.tables_ref(ids, 4, 128, 512)
    assert counts.tolist() == [2, 2, 2, 0] and offs.tolist() == [0, 128, 256, 384, 384]
    assert gather[:3].tolist() == [0, 1, -1] and gather[128:130].tolist() == [1, 2] and gather[256:258].tolist() == [0, 2] and int((gather >= 0).sum()) == 6
    assert inv.tolist() == [[256, 0], [1, 128], [257, 129]]
    counts, offs, gather, inv = X.tables_ref(ids, 4, 1, 6)
    assert offs.tolist() == [0, 2, 4, 6, 6] and gather.tolist() == [0, 1, 1, 2, 0, 2]


# ------------------------------------------------------------------------------------------------------------ the references alone
def test_references_alone_stay_inside_every_bound(capsys):
    worst = [0.0, 0, 0]
    for row in ROUTE[::3]:
        if row.S > 1100:
            continue
        w, r, l = X.reference_alone_route(X.RouteCase(row))
        worst = [max(worst[0], w), max(worst[1], r), max(worst[2], l)]
    assert worst[0] <= X.WTS_TOL and worst[1] <= X.RSTD_ULPS and worst[2] <= X.LOGIT_ULPS, worst
    nd = tot = 0
    cases = [X.GemmCase(r) for r in X.gemm_table()[:18] if r.epi != "plain"] + [X.SkinnyCase(r) for r in X.skinny_table() if r.swiglu] + \
            [X.GateUpCase(1, *a, False) for a in X.GU_CASES] + [X.GateUpCase(*a, True) for a in X.GU_BATCHED]
    for c in cases:
        acc = c.acc if hasattr(c, "acc") else None
        if acc is None:
            continue
        y32 = X._epilogue(acc.float(), getattr(c, "rs_live", None), True, torch.float32)
        d = D.ulp_distance(y32.bfloat16(), c.ref.float().bfloat16())
        assert int(d.max()) <= 1 and int((d > 0).sum()) <= max(1, c.R * c.n_out // 100), c.coords()
        nd, tot = nd + int((d > 0).sum()), tot + d.numel()
    rs = 0
    for row in X.combine_table():
        c = X.CombineCase(row)
        st = c.expected().float()
        rs = max(rs, int(X.ulp32(torch.rsqrt((st * st).mean(1) + X.EPS), c.rstd_ref()).max()))
    assert rs <= X.RSTD_ULPS
    with capsys.disabled():
        print(f"\nreferences alone (torch fp32 against fp64): wts {worst[0]:.2e}, rstd {worst[1]} steps, logits {worst[2]} steps; SwiGLU {nd} of {tot} "
              f"outputs one step off; combine rstd {rs} steps")


def test_rounding_at_the_store_is_exercised():
    sh, ties, n = 0.0, 0, 0
    for row in X.down_table():
        s, t = X.DownCase(row).rounding_share()
        sh, ties, n = sh + s, ties + t, n + 1
    assert sh / n > 0.10 and ties > 0, (sh / n, ties)
    sh, ties, n = 0.0, 0, 0
    for row in X.gemm_table():
        if row.epi == "plain" and row.E < 64:
            s, t = X.GemmCase(row).rounding_share()
            sh, ties, n = sh + s, ties + t, n + 1
    assert sh / n > 0.10 and ties > 0, (sh / n, ties)
    assert sum(X.CombineCase(r).rounding_count() for r in X.combine_table()) >= 100


# ------------------------------------------------------------------------------------------------------------ the tables
def test_constants_match_the_header_and_ops():
    from videollama2_amd import ops
    src = open(os.path.join(ROOT, "videollama2_amd", "csrc", "k_moe.h")).read()
    for name, val in (("MOE_MAX_E", X.MOE_MAX_E), ("MOE_MAX_K", X.MOE_MAX_K), ("MOE_SCAN_MAX", X.MOE_SCAN_MAX)):
        assert int(re.search(rf"#define {name} (\d+)", src).group(1)) == val
    assert X.MOE_BM == ops.MOE_BM
    for S, k, E in ((1, 1, 1), (5, 2, 8), (449, 2, 8), (8192, 2, 8), (4096, 4, 16), (65, 4, 64)):
        assert X.moe_rows(S, k, E) == ops.moe_rows(S, k, E)


def _rows_ok(S, k, E, P):
    return S * k <= X.MOE_SCAN_MAX and 1 <= k <= min(E, X.MOE_MAX_K) and E <= X.MOE_MAX_E and P % X.MOE_BM == 0 and P >= S * k + E * (X.MOE_BM - 1)


def test_every_case_is_accepted_by_the_row_rule_or_is_a_must_refuse_row():
    for row in ROUTE:
        assert _rows_ok(row.S, row.k, row.E, X.moe_rows(row.S, row.k, row.E)), row
    for row in X.gemm_table():
        c = X.GemmCase(row)
        assert _rows_ok(c.S, c.k, c.E, c.P) and int(c.offs[-1]) <= c.P and c.N % 128 == 0 and c.K % 64 == 0, c.coords()
    for row in X.skinny_table():
        assert row.S <= 64 and sum(row.counts) == row.S * row.k and max(row.counts) <= row.S and row.K % 32 == 0 and row.N % (128 if row.swiglu else 64) == 0
    for row in X.down_table():
        assert row.k * row.K * 2 <= 160 * 1024 and row.k <= min(row.E, 4)
    for why, entry, S, E, k, P, msg in X.ROUTE_REFUSALS:
        full = X.moe_rows(S, k, E)
        assert not _rows_ok(S, k, E, full if P is None else full - 128 if P == "small" else full + 64), why
    for why, batched, S, k, K, msg in X.DOWN_REFUSALS:
        assert k * K * 2 == 160 * 1024 + 64 and 4 * X.DOWN_K_LDS * 2 == 160 * 1024


def test_tables_cover_what_their_comments_claim():
    for entry in ("route", "rows"):
        rows = [r for r in ROUTE if r.entry == entry]
        assert {r.S for r in rows} >= set(X.ROUTE_S) and {r.E for r in rows} == set(X.ROUTE_E) and {r.k for r in rows} == set(X.ROUTE_K)
        assert {(r.S, r.k) for r in rows} >= {(8192, 2), (4096, 4)}
        assert {r.arg for r in rows if r.mode == "free"} == set(X.FREE_D)
        assert {(r.arg, r.k) for r in rows if r.mode == "ties"} >= {(kind, k) for kind in X.TIES for k in (2, 3, 4)}
        vecs = [v for v, _ in (X.COUNT_VECTORS if entry == "route" else X.COUNT_VECTORS_ROWS).values()]
        assert {c for v in vecs for c in v} >= {0, 1, 127, 128, 129, 256, 257}
        assert any(v[0] == 0 for v in vecs) and any(v[-1] == 0 for v in vecs)
        assert {tuple(i for i, c in enumerate(v) if c) for v in vecs if sum(1 for c in v if c) == 1} >= {(0,), (3,), (7,)}
    assert {r.E for r in ROUTE if r.entry == "gemv"} >= {1, 2, 8, 17, 64} and {r.k for r in ROUTE if r.entry == "gemv"} == {1, 2, 3, 4}
    gt = X.gemm_table()
    for E in (2, 8, 64):
        rows = [r for r in gt if r.E == E and not r.shrink]
        assert {r.counts[0] for r in rows} == {r.counts[-1] for r in rows} == set(X.GEMM_COUNTS)
        if E > 2:
            assert {c for r in rows for c in r.counts[1:-1]} == set(X.GEMM_COUNTS)
    assert {r.N for r in gt} == {128, 256, 384} and {r.K for r in gt} == set(X.G.K_ALL) and {r.epi for r in gt} == set(X.MOE_EPIS)
    grids = {X.GemmCase(r).grid % 8 == 0 for r in gt if r.E < 64}
    assert grids == {True, False}, "xcd_remap: workgroup counts that are and are not multiples of 8"
    st = X.skinny_table()
    assert {r.S for r in st} == set(X.SKINNY_S) and {c for r in st for c in r.counts} >= {0, 1, 15, 16, 17, 33, 64}
    assert {r.rowmap for r in st} == {True, False} and {r.N for r in st} == {128, 1024}
    assert {D.skinny_plan(r.S, r.N, r.K)["mt"] for r in st} == {1, 2, 4}
    assert D.skinny_plan(5, 128, 1184)["ks"] == 1 and {D.skinny_plan(5, r.N, r.K)["ks"] for r in st} >= {1, 2, 3, 16}
    dt = X.down_table()
    assert {r.K for r in dt} == set(X.DOWN_K) | {X.DOWN_K_LDS} and {r.N for r in dt} >= set(X.DOWN_N) and {r.k for r in dt} == {1, 2, 3, 4}
    assert {r.S for r in dt if r.batched} == {1, 2, 5} and {r.res for r in dt} == {True, False}
    assert {(k, K > 4096) for _, E, k, N, K, res, b in dt} >= {(k, two) for k in (1, 2, 3, 4) for two in (False, True)}
    for E, k, N, K in X.GU_CASES:
        ids = X.GateUpCase(1, E, k, N, K, False).ids[0].tolist()
        assert E - 1 in ids and (k == 1 or 0 in ids)
    assert {(E, k) for E, k, _, _ in X.GU_CASES} >= {(4, 1), (4, 2), (4, 4), (64, 1), (64, 2), (64, 4)}
    ct = X.combine_table()
    assert {r.D for r in ct} == set(X.COMBINE_D) and {r.k for r in ct} == {1, 2, 3, 4} and {r.S for r in ct} == {1, 5} and {r.alias for r in ct} == {True, False}
    asc = desc = 0
    for r in ct:
        inv = X.CombineCase(r).inv
        if r.k > 1:
            asc, desc = asc + int((inv[:, 1:] > inv[:, :-1]).sum()), desc + int((inv[:, 1:] < inv[:, :-1]).sum())
    assert asc > 0 and desc > 0, "slots on rows in and out of ascending order"


# ------------------------------------------------------------------------------------------------------------ the checkers catch faults
def test_checkers_report_planted_faults():
    c = X.DownCase(X.DRow(1, 4, 2, 5, 72, True))
    st = torch.full((8 + 5 + 8,), X.SENTINEL, dtype=torch.bfloat16)
    st[8:13] = c.expected()[0]
    assert X.check_down(c, st) is None
    bad = st.clone()
    bad[9] = (bad[9].float() * (1 + 2.0 ** -7)).bfloat16()                  # one step
    assert "differ" in X.check_down(c, bad)
    bad = st.clone()
    bad[13] = 0.0
    assert "frame" in X.check_down(c, bad)
    c = X.RouteCase(X.RRow("rows", 33, 8, 2, "ties", "chosen"))
    f = lambda t, fill, dt: torch.cat((torch.full((8,), fill, dtype=dt), t.reshape(-1).to(dt), torch.full((8,), fill, dtype=dt)))
    out = dict(ids=f(c.ids, X.ISENT, torch.int32), wts=f(c.wts_ref, X.SENTINEL, torch.float32), logits=f(c.logits_ref, X.SENTINEL, torch.float32),
               counts=f(c.counts, X.ISENT, torch.int32), offs=f(c.offs, X.ISENT, torch.int32), gather=f(c.gather, X.ISENT, torch.int32),
               inv=f(c.inv, X.ISENT, torch.int32))
    assert X.check_route(c, out)[0] == []
    swapped = dict(out)
    ids = c.ids.clone()
    ids[4] = ids[4].flip(0)                                                  # the tie broken to the higher index on one row
    swapped["ids"] = f(ids, X.ISENT, torch.int32)
    assert "ids differ on 1 of 33 rows" in X.check_route(c, swapped)[0][0]
    g = c.gather.clone()
    g[[0, 1]] = g[[1, 0]]
    swapped = dict(out, gather=f(g, X.ISENT, torch.int32))
    assert any("gather" in e for e in X.check_route(c, swapped)[0])
    w = c.wts_ref.clone().float()
    w[0, 0] += 2.0 ** -24
    assert any("exactly 1 / 2" in e for e in X.check_route(c, dict(out, wts=f(w, X.SENTINEL, torch.float32)))[0])
