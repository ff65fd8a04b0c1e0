"""vl2_attn_fwd (prefill, extend beyond 64 rows, both vision towers) on MI355X, bit for bit on exact key-selecting inputs
(tests/attn_fwd_exact.py: THE RULE, the trap, the guard, the case tables): all 16 kernel instances of csrc/k_attn.h and
csrc/k_attn2.h -- head_dim 64 / 96 / 128, causal or full, one or two KV groups, one or two key streams, the class-token peel, the three causal
grid orders -- in the towers' fused layout, the decoders' and a batch of requests with their own caches, poisoned past nk and framed by
sentinels, under every variant that serves a case, in the bf16 and the fp16 build.  Every comparison is torch.equal against the fp64 softmax
over the visible keys rounded once; that the tables pass here is the measurement that exp2(0) == 1, exp2(x <= -200) == 0 and 1.0f / L is exact
for a power-of-two L on the bare v_exp_f32 / the division these kernels use.  The exact inputs only make weights 0 and 1: one random-input case
per kernel instance checks graded weights per (row, head) against a rounding model.  (Variant 5, lab: tests/test_gpu_lab.py; the CPU twin with
the generator proofs: tests/test_attn_fwd_edges_emu.py.)"""
import pytest
import torch

from tests import attn_fwd_exact as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
CASES = F.all_cases()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib, ops as o
    _lib.load()
    return o


def _groups(cases):
    """The tables in groups of a few seconds at the most."""
    groups = {}
    for c in cases:
        key = f"CAUSAL_GRID_B{c.B}" if c.table == "CAUSAL_GRID" else c.table
        groups.setdefault(key, []).append(c)
    return groups


def _run(ops, cases, elem):
    """Failures are collected over the cases of a test and reported with their coordinates (case, variant, round, request, head, row, the
    first differing element, expected and received bits: `F.describe`)."""
    errs, n = [], 0
    for c in cases:
        errs += F.run_case(ops, c, elem, DEV)
        n += F.rounds_of(c) * len(F.variants_of(c))
    assert not errs, f"{len(errs)} of {n} launches failed:\n" + "\n".join(errs[:16])


_BF16 = _groups(CASES)
_FP16 = _groups(F.fp16_cases())


@pytest.mark.parametrize("group", sorted(_BF16))
def test_attn_fwd_exact(ops, group):
    """Every case of every table, every round of selectors, every variant that serves the case."""
    _run(ops, _BF16[group], BF)


@pytest.mark.parametrize("group", sorted(_FP16))
def test_attn_fwd_exact_fp16_build(ops, group):
    """The fp16 build (-2048 and the V values are exact in fp16): one row per table edge class, every kernel instance."""
    from videollama2_amd import _lib
    _lib.set_elem("fp16")
    try:
        _run(ops, _FP16[group], torch.float16)
    finally:
        _lib.set_elem("bf16")


# ---------------------------------------------------------------------------------------------------------------- graded weights
@pytest.mark.parametrize("elem", [BF, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("spec", F.GRADED, ids=lambda s: "D%d%s_N%d" % (s[0], "c" if s[1] else "f", s[5]))
def test_graded_weights_per_row_against_the_rounding_model(ops, spec, elem):
    """Random inputs: softmax weights of every size, rescale factors strictly inside (0, 1), the deferred rescale (a tile maximum within 2^6
    of the running one), P rounded to the element type -- what the exact inputs cannot reach.  The error is taken per (request, head, row), so
    one wrong row shows (it cannot move a norm over the tensor), against the fp64 softmax, with NaN past nk and in the padding.

    The bound is computed here, from the reference alone: the ROUNDING MODEL (`F.graded_reference`) is the softmax at the kernel's precision --
    fp32 scores and weights, P rounded to the element type before it meets V, the denominator from the unrounded weights, the result rounded
    once.  Its largest per-row rel-L2 against the fp64 softmax is what those two roundings cost on these inputs; the kernel's largest per-row
    error must stay within F.GRADED_MARGIN = 1.5 of it.  Why 1.5: kernel and model make the same two roundings but not at the same points --
    the kernel rounds P relative to the RUNNING maximum (up to 2^6 above the final one's scale, another binade of the same relative size) and
    sums in tile order -- so the two maxima are two draws of the same per-row error distribution over some hundred rows, not one number.
    Measured (profiles/r17_attn_fwd_edges.md): kernel / model between 0.92 and 1.36 over every instance and both builds.  An error above twice
    the model's would be a finding (a lost tile, a wrong rescale: those cost a row 1e-2 and more), not a margin to widen."""
    from videollama2_amd import _lib
    c = F.graded_case(*spec)
    q, K, V = F.graded_inputs(c, elem)
    ref, model = F.graded_reference(c, q, K, V, elem)
    e_model = float(F.row_rel(model[..., :c.used], ref[..., :c.used]).max())
    _lib.set_elem("fp16" if elem == torch.float16 else "bf16")
    try:
        opnd = F.Operands(c, q, K, V, elem, DEV)
        Wo = c.H * c.D + 8
        bad = []
        for v in F.variants_of(c):
            o = F.launch(ops, c, opnd, v, DEV)
            y = torch.as_strided(o.view(-1), (c.B, c.H, c.nq, c.D), ((c.nq + 2) * Wo, c.D, Wo, 1), Wo)
            e = F.row_rel(y[..., :c.used], ref[..., :c.used])
            print(f"graded {c.name} {F.instance(c, v)} (variant {v}) {elem}: kernel {float(e.max()):.3e} model {e_model:.3e} ratio {float(e.max()) / e_model:.2f}")
            if not float(e.max()) <= F.GRADED_MARGIN * e_model:
                b, h, r = torch.nonzero(e == e.max())[0].tolist()
                bad.append(f"variant {v}: request {b} head {h} row {r}: rel-L2 {float(e.max()):.3e} > {F.GRADED_MARGIN} x {e_model:.3e}")
            if not bool((y[..., c.used:] == 0).all()):
                bad.append(f"variant {v}: the unused dims of the output are not zero")
            frame = torch.ones(o.shape, dtype=torch.bool)
            frame[:, 1:c.nq + 1, :c.H * c.D] = False
            if not (bool((o[frame] == F.SENTINEL).all()) and opnd.intact()):
                bad.append(f"variant {v}: the sentinel frame, q, k or v changed")
        assert not bad, c.name + "\n" + "\n".join(bad)
    finally:
        _lib.set_elem("bf16")
