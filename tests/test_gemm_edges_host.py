"""The exact-input edge cases of tests/gemm_exact.py on the CPU: the helper proven (both guards, fp32 sums in other associations, the checker
against planted faults, the references alone within the cap) and every row of the case tables held against csrc/gemm_plan.h, so that a later
edit of the plan cannot hollow out tests/test_gpu_gemm_edges.py.  DESIGN.md section 15b."""
import ctypes

import pytest
import torch

from tests import gemm_exact as G
from tests.test_gemm_plan_host import IN_KEYS, PRODUCT_AUTO_FORMS, plan_lib  # noqa: F401  (the shim and its fixture; that test is not edited)

SMALL = {k: v for k, v in G.all_tables().items() if k != "mixed"}       # the mixed-form shapes are large: their references run on the device


def _plan(lib, row):
    d = G.plan_inputs(row)
    ins = [int(d.get(k, 0)) for k in IN_KEYS]
    out = ctypes.create_string_buffer(1024)
    lib.plan((ctypes.c_longlong * len(ins))(*ins), out, len(out))
    fin, launches = out.value.decode().split("|")
    ls = []
    for l in launches.split(";"):
        f = l.split()
        ls.append(dict(form=f[0], th=int(f[1]), tw=int(f[2]), m0=int(f[3]), rows=int(f[4]), mode=int(f[11]), split=int(f[13]), dyn=int(f[14])))
    return int(fin), ls


# ------------------------------------------------------------------------------------------------------------ generators and guards
@pytest.mark.parametrize("group", sorted(SMALL))
def test_every_case_passes_the_guards_and_other_fp32_orders_give_the_reference(group):
    """Both guards hold for every row (asserted in Case), and the epilogue on accumulators summed in fp32 in three other associations (16-wide
    steps, 32-wide steps over reversed tiles, three partial sums) equals the fp64 reference bit for bit on every exact epilogue: the order
    independence the GPU test relies on, without a GPU."""
    inexact, ties, n = 0.0, 0, 0
    for row in SMALL[group]:
        c = G.Case(row)
        assert c.bound < 2 ** 24 and c.quantum >= 2.0 ** -20, c.coords()
        for acc32 in G.acc_in_other_orders(c):
            assert torch.equal(acc32.double(), c.acc), c.coords()
        if G.approx(row):
            continue
        y32 = c.epilogue(c.acc.float(), torch.float32)
        assert y32.dtype == torch.float32 and torch.equal(c.expected(y32.double()), c.expected()), c.coords()
        if c.e["stats"]:
            assert c.stats_bound < 2 ** 24
            y = c.expected().float().reshape(c.M, -1, 4, 16)                # sums of 16, then of 4, in fp32
            s32 = torch.stack((y.sum(-1, dtype=torch.float32).sum(-1, dtype=torch.float32), (y * y).sum(-1, dtype=torch.float32).sum(-1, dtype=torch.float32)), -1)
            assert torch.equal(s32, c.stats_ref()), c.coords()
        if not c.e["f32"]:
            sh, t = c.rounding_share()
            inexact, ties, n = inexact + sh, ties + t, n + 1
    if n:
        print(f"\n{group}: {inexact / n:.2f} of the bf16 outputs need rounding, {ties} exact ties")
        assert inexact / n > 0.10 and ties > 0, f"{group}: RNE at the store is hardly exercised ({inexact / n:.3f}, {ties} ties)"


def test_guards_fire_when_a_range_is_widened():
    G.Case(G.Row("GF_128", 128, 1, 33, 128, 1088, "stats"))
    with pytest.raises(AssertionError, match="statistics guard"):
        G.Case(G.Row("GF_128", 128, 1, 33, 128, 1088, "stats"), wide=True)          # sums of about +-1400: 64 squares pass 2^24
    c = G.Case(G.Row("GF_128", 128, 1, 33, 128, 1088, "ln"))
    c.a64 = c.a64 * 1024.0                                                  # still multiples of the quantum: sums of magnitudes of about 2^25
    with pytest.raises(AssertionError, match="exactness guard"):
        c.guard_case()
    c = G.Case(G.Row("GF_128", 128, 1, 33, 128, 1088, "bias"))
    c.bias = c.bias + 0.5                                                   # off the quantum
    with pytest.raises(AssertionError, match="not a multiple"):
        c.guard_case()


# ------------------------------------------------------------------------------------------------------------ the checker catches faults
FAULT_CASES = [G.Row("GF_128", 128, 1, 129, 256, 192, e) for e in ("plain", "f32", "bias", "res", "bias_res", "stats", "rms", "ln", "norm_out")] + \
              [G.Row("GF_128", 128, 1, 129, 256, 192, e) for e in ("swiglu_res", "qgelu")] + [r for r in G.REMAP[:1]] + [G.GATHER[0]] + \
              [G.Row("GF_FP8_128x256", 128, 4, 129, 256, 256, "bias", fp8=True), G.Row("GF_GEMM6", 256, 70, 257, 256, 1024, "plain", tile_ctr=True, dyn=1)]


@pytest.mark.parametrize("row", FAULT_CASES, ids=lambda r: f"{r.form}-{r.epi}")
def test_checker_reports_planted_faults(row):
    c = G.Case(row)
    good = c.perfect()
    assert G.check_case(c, good)[0] is None
    rows = 1 + c.out_row_of(torch.arange(c.M))
    step = 2.0 if G.approx(row) else 1.0                                     # approximate epilogues: one step is allowed, two are not

    def planted(name, **bufs):
        snap = dict(good)
        snap.update(bufs)
        err, _ = G.check_case(c, snap)
        assert err is not None, f"{c.coords()}: the checker missed: {name}"

    # one element off by one quantum of its type (bf16: the neighbouring number; two for the approximate epilogues)
    o = good["out"].clone()
    m, n = int(rows[c.M - 1]), c.n_out - 1
    if o.dtype == torch.bfloat16:
        o[m, n] = (o[m:m + 1, n].view(torch.int16) + int(step)).view(torch.bfloat16)[0]
    else:
        o[m, n] = torch.nextafter(o[m, n], torch.tensor(float("inf")))
    planted("one element off by one step", out=o)
    # the single row of the last row tile duplicated from its neighbour
    o = good["out"].clone()
    o[rows[c.M - 1], :c.n_out] = o[rows[c.M - 2], :c.n_out]
    planted("the last row duplicated from its neighbour", out=o)
    # a canary overwritten: a pad column, the row behind the last, the row in front of the first
    for where in ((m, c.n_out), (int(rows[-1]) + 1, 0), (0, 3)):
        o = good["out"].clone()
        o[where] = 0.0
        planted(f"canary {where}", out=o)
    if c.bias is not None and not G.approx(row):
        shifted = c.expected(c.epilogue(c.acc, torch.float64) - c.bias + torch.roll(c.bias, 1))
        o = good["out"].clone()
        o[rows, :c.n_out] = shifted
        planted("bias shifted by one column", out=o)
    if c.res is not None and not G.approx(row) and not c.e["f32"]:
        once = c.expected(c.ref - c.res)                                    # rounded in front of the residual, and again behind it
        twice = (once.double() + c.res).float().bfloat16()
        assert not torch.equal(twice, c.expected()), "the inputs do not tell one rounding from two"
        o = good["out"].clone()
        o[rows, :c.n_out] = twice
        planted("the residual rounded twice", out=o)
    if c.e["stats"]:
        s = good["stats"].clone()
        s[c.M, 0], s[c.M, 1] = good["stats"][c.M, 1], good["stats"][c.M, 0]
        assert not torch.equal(s, good["stats"])
        planted("stats_out of one 64-column block swapped with the next", stats=s)
        s = good["stats"].clone()
        s[c.M + 1, 0, 0] = 0.0
        planted("stats_out frame", stats=s)
    if c.e["norm_out"]:
        rn = good["rn"].clone()
        rn[c.M], rn[c.M - 1] = good["rn"][c.M - 1], good["rn"][c.M]
        assert not torch.equal(rn, good["rn"])
        planted("row_norm_out of the last row swapped with its neighbour", rn=rn)
        rn = good["rn"].clone()
        rn[c.M + 1, 1] = 1.0
        planted("row_norm_out frame", rn=rn)
        t = good["tick"].clone()
        t[c.M // 128] = 1
        planted("a row ticket left armed", tick=t)
    if row.tile_ctr:
        t = good["ctr"].clone()
        t[1] = 3
        planted("the tile counter block not re-armed", ctr=t)


# ------------------------------------------------------------------------------------------------------------ the references alone
def test_reference_alone_stays_within_the_cap_on_every_approximate_case():
    """torch fp32 activations / silu against fp64 on the same exact accumulators: at most one bf16 step, and the share within the cap the GPU
    test applies -- the cap leaves the kernels room only beyond what fp32 evaluation itself costs."""
    worst = (0.0, "")
    for group, rows in SMALL.items():
        for row in rows:
            if not G.approx(row):
                continue
            c = G.Case(row)
            nd, far = G.reference_alone_share(c)
            assert far <= 1 and nd <= G.approx_cap(c), (c.coords(), nd, far, G.approx_cap(c))
            pre = c._pre(c.acc, torch.float64)
            pre = pre.reshape(c.M, -1, 2, 32)[:, :, 0] if c.e["swiglu"] else pre
            amp = G.pre_amp(row)
            assert amp / 2 < float(pre.abs().max()) <= amp, f"{c.coords()}: pre-activation values should spread over +-{amp}"
            if nd / (c.M * c.n_out) > worst[0]:
                worst = (nd / (c.M * c.n_out), c.coords())
    print(f"\nlargest reference-alone share {worst[0]:.2e} {worst[1]}")


# ------------------------------------------------------------------------------------------------------------ plan coverage
def test_every_table_row_gets_the_form_tile_and_split_it_claims(plan_lib):  # noqa: F811
    bad = []
    for group, rows in G.all_tables().items():
        for row in list(rows) + (list(G.M_INDEP) if group == "v1_128" else []):
            fin, ls = _plan(plan_lib, row)
            want = row.forms or (row.form,)
            got = tuple(l["form"] for l in ls)
            l0 = ls[0]
            ok = got == want and l0["th"] == row.th and l0["split"] == row.split and l0["dyn"] == row.dyn
            if row.form in ("GF_GEMM9", "GF_MIX16"):
                ok = ok and l0["mode"] == row.mode
            if not ok:
                bad.append(f"{group}: {row}\n    plan: {ls}")
    assert not bad, f"{len(bad)} rows do not get what they claim:\n" + "\n".join(bad[:10])


def test_tables_reach_every_product_form_and_variant(plan_lib):  # noqa: F811
    forms, variants, fp8_variants = set(), set(), set()
    for group, rows in G.all_tables().items():
        for row in rows:
            forms.update(l["form"] for l in _plan(plan_lib, row)[1])
            (fp8_variants if row.fp8 else variants).add(row.variant)
    assert forms >= PRODUCT_AUTO_FORMS, sorted(PRODUCT_AUTO_FORMS - forms)
    # = PRODUCT_VARIANTS of tests/test_gemm_plan_host.py (a local of test_table_reaches_every_form_of_the_automatic_choice there, so it cannot be
    # imported: keep this set in step with that line) without 24 (= variant 0 planned without the persistent form: the same kernels)
    assert variants >= {0, 1, 4, 8, 12, 16, 26, 32, 60, 61, 70, 71, 80, 81, 192, 224, 256}, sorted(variants)
    assert fp8_variants == {0, 4, 8, 12}


def test_mixed_shapes_are_the_smallest_the_plan_splits(plan_lib):  # noqa: F811
    """GF_MIX is reached by the automatic choice only: among the shapes of at most 8192 rows, none with fewer multiply-adds than the table's
    smallest, at K = 1024, gets it."""
    best = min(M * N for M, N, K in G.MIX_SHAPES)
    for N in range(256, 16384 + 1, 256):
        for M in range(1024, min(best // N, 8192) + 1):
            row = G.Row("GF_MIX", 256, 0, M, N, 1024, "plain")
            if M * N < best and _plan(plan_lib, row)[1][0]["form"] == "GF_MIX":
                pytest.fail(f"{M} x {N} x 1024 is a smaller mixed-form shape than the table's")
