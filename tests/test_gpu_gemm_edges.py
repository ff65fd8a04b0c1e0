"""The tiled GEMM family (vl2_gemm: every product form of csrc/gemm_plan.h, forced variant by forced variant, split-K, the remap and gathered
forms, the fp8 forms and the mixed launches of the automatic choice) on exact inputs at the tile edges, on the MI355X: tests/gemm_exact.py's
case tables through ops.gemm / ops.gemm_fp8.  fp32 accumulation is exact in any order on these inputs, so every output equals the fp64 reference
bit for bit -- `torch.equal`, no tolerance, the 16 x 16 x 32 set, split-K and fp8 included; only the activations and silu of SwiGLU are
approximate, held to one bf16 step with the cap `approx_cap`.  Every operand is a strided view of a poisoned allocation, every output, stats_out
and row_norm_out sits inside a sentinel frame, and every case runs twice on the same buffers.  tests/test_gemm_edges_host.py holds the tables
against the plan on the CPU.  DESIGN.md section 15b; measured figures: profiles/r15_gemm_edges.md."""
import pytest
import torch

from tests import gemm_exact as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from videollama2_amd import _lib, ops as o
    _lib.load()
    o.attach_workspace(DEV)
    return o


def _run(ops, rows, ref_dev="cpu"):
    errs, n, shares = [], 0, {}
    for row in rows:
        c = G.Case(row, dev=ref_dev)
        first, second = G.run_case(ops, c, DEV)
        err, nd = G.check_case(c, first)
        err2, _ = G.check_case(c, second)
        n += 1
        if err or err2:
            errs.append(err or "second run on the same buffers: " + err2)
        elif not G.same_bits(first, second):
            errs.append(f"{c.coords()}: two runs on the same buffers differ")
        if G.approx(row):
            kind = "swiglu" if c.e["swiglu"] else c.e["act"]
            d, t, w = shares.get(kind, (0, 0, 0.0))
            shares[kind] = (d + nd, t + c.M * c.n_out, max(w, nd / (c.M * c.n_out)))
        if ref_dev != "cpu":
            del c, first, second
            torch.cuda.empty_cache()
    for kind, (d, t, w) in sorted(shares.items()):
        print(f"\n  {kind}: {d} of {t} outputs one bf16 step from RNE of the fp64 value ({d / t:.2e}); largest share of a case {w:.2e}, cap 1.00e-02", end="")
    assert not errs, f"{len(errs)} of {n} cases failed:\n" + "\n".join(errs[:16])


@pytest.mark.parametrize("group", sorted(G.FAMILY))
def test_forced_variant_edges(ops, group):
    _run(ops, G.FAMILY[group])


@pytest.mark.parametrize("group", sorted(G.FP8))
def test_fp8_edges(ops, group):
    _run(ops, G.FP8[group])


def test_splitk_edges(ops):
    _run(ops, G.SPLITK)


def test_remap_edges(ops):
    _run(ops, G.REMAP)


def test_gathered_edges(ops):
    _run(ops, G.GATHER)


@pytest.mark.parametrize("row", G.MIXED, ids=lambda r: f"{r.form}-v{r.variant}-{r.M}x{r.N}x{r.K}-{r.epi}")
def test_mixed_form_shapes(ops, row):
    """The launches only the automatic choice makes, at the smallest shapes that get them; the reference is torch fp64 on the device (exact under
    the guard, and no code shared with the kernels)."""
    _run(ops, [row], ref_dev=DEV)


@pytest.mark.parametrize("row", G.M_INDEP, ids=lambda r: r.form)
def test_rows_do_not_depend_on_m_across_a_tile_boundary(ops, row):
    c = G.Case(row)
    m1 = G.M_INDEP_M1
    big = G.run_case(ops, c, DEV)[-1]
    small = G.run_case(ops, c, DEV, m_rows=m1)[-1]
    assert G.check_case(c, big)[0] is None
    assert torch.equal(small["out"][1:1 + m1], big["out"][1:1 + m1]), "rows [0, m1) differ between the call on M rows and the call on m1 rows"
    assert bool((small["out"][1 + m1:] == G.SENTINEL).all()) and bool((small["out"][0] == G.SENTINEL).all())


def test_rejections_leave_the_framed_output_untouched(ops):
    """Every refusal of vl2_gemm that the tables brush against: the call raises and writes nothing (the checks precede every launch)."""
    from videollama2_amd import _lib
    M = 33

    def bufs(N, K, n_out=None, f32=False, lda_pad=8, fp8=False):
        n_out = n_out or N
        dt = torch.uint8 if fp8 else torch.bfloat16
        a = torch.zeros((M + 1, K + lda_pad), dtype=dt, device=DEV)
        w = torch.zeros((N + 1, K + (16 if fp8 else 8)), dtype=dt, device=DEV)
        out = torch.full((M + 2, n_out + 8), G.SENTINEL, dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)
        return a[:M, :K], w[:N, :K], out

    calls = []

    def add(why, N, K, variant=0, fp8=False, lda_pad=None, **kw):
        lda_pad = (16 if fp8 else 8) if lda_pad is None else lda_pad       # a legal row stride unless the stride is what the call is about
        n_out = N // 2 if kw.get("swiglu") else N
        a, w, out = bufs(N, K, n_out, kw.get("out_f32", False), lda_pad, fp8)
        if kw.pop("bias", False):
            kw["bias"] = torch.zeros(N, dtype=torch.float32, device=DEV)
        if kw.pop("stats", False):
            kw["stats_out"] = torch.full((M, N // 64, 2), G.SENTINEL, dtype=torch.float32, device=DEV)
        calls.append((why, variant, fp8, a, w, out, n_out, kw))

    add("N % 128", 192, 64)
    add("K % 64", 128, 96)
    add("ld % 8", 128, 64, lda_pad=4)
    add("variant 16 with an activation", 256, 64, variant=16, act=G.ACT_CODE["gelu"])
    add("variant 16 with N % 256", 384, 64, variant=16)
    add("variant 26 with N % 256", 384, 64, variant=26)
    add("fp8 with K % 128", 256, 192, fp8=True)                            # lda = ldw = 208, N % 256 == 0: K is the only violation
    add("fp8 with lda % 16", 256, 256, fp8=True, lda_pad=8)                # ... and here the row stride of A is
    add("SwiGLU with bias", 128, 64, swiglu=True, bias=True)
    add("stats with fp32 out", 128, 64, out_f32=True, stats=True)
    try:
        for why, variant, fp8, a, w, out, n_out, kw in calls:
            ops.set_gemm_variant(variant)
            with pytest.raises(_lib.Vl2HipError):
                if fp8:
                    ops.gemm_fp8(a, torch.ones((M, 2), device=DEV), w, torch.ones(w.shape[0], device=DEV), out=out[1:M + 1, :n_out], **kw)
                else:
                    ops.gemm(a, w, out=out[1:M + 1, :n_out], **kw)
                pytest.fail(f"accepted: {why}")
            torch.cuda.synchronize()
            assert bool((out == G.SENTINEL).all()), f"output written: {why}"
            if "stats_out" in kw:
                assert bool((kw["stats_out"] == G.SENTINEL).all()), f"stats_out written: {why}"
    finally:
        ops.set_gemm_variant(0)
