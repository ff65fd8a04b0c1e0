"""The split-KV attention family on MI355X, bit for bit on exact key-selecting inputs (tests/attn_exact.py: THE RULE, the guard, the case tables;
DESIGN.md section 18): vl2_attn_decode (pos by value and *pos_dev with three ctx_cap), vl2_attn_decode_batched (strides, poison, row stability,
a request past the cache end), vl2_attn_decode_kv8 / _kv8_batched (the same tables on the fp8 caches, and the dequantised-cache property at long
contexts), vl2_attn_decode_shared and vl2_attn_append at the edges of their split plans -- every case through all three regimes of
attn_combine_head where its context reaches them.  The exact inputs only make weights 0 and 1: one random-input case per regime checks graded
weights against the fp64 softmax.  (The lab form vl2_attn_decode_fused: tests/test_gpu_lab.py; the CPU twin: tests/test_attn_edges_emu.py.)"""
import pytest
import torch

from tests import attn_exact as A
from tests import fp8kv_oracle as KV
from tests.util import TOL_BF16_OUT, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib, ops as o
    _lib.load()
    return o


def _decode_table(ops, group, nkv, positions, elem, kv8=False):
    errs, n = [], 0
    for pos in positions:
        st = A.DecodeState(group, nkv, pos, elem, DEV, kv8=kv8)
        for form, rnd in A.decode_launches(st.rounds, every_round=True):
            err = A.run_decode(ops, st, form, rnd)
            n += 1
            if err:
                errs.append(err)
    assert not errs, f"{len(errs)} of {n} launches failed:\n" + "\n".join(errs[:12])


# ---------------------------------------------------------------------------------------------------------------- vl2_attn_decode
@pytest.mark.parametrize("group,nkv", A.DECODE_GROUPS, ids=lambda v: str(v))
@pytest.mark.parametrize("half", [0, 1], ids=["short", "long"])
def test_decode_exact(ops, group, nkv, half):
    """Every position of the table, every form, every selector: torch.equal to the fp64 softmax rounded once."""
    cut = A.DECODE_POS.index(4095)
    _decode_table(ops, group, nkv, A.DECODE_POS[:cut] if half == 0 else A.DECODE_POS[cut:], BF)


def test_decode_exact_fp16_build(ops):
    from videollama2_amd import _lib
    _lib.set_elem("fp16")
    try:
        for group, nkv in ((4, 2), (7, 2)):
            _decode_table(ops, group, nkv, A.REGIME_POS, torch.float16)
    finally:
        _lib.set_elem("bf16")


# ---------------------------------------------------------------------------------------------------------------- vl2_attn_decode_batched
@pytest.mark.parametrize("group", [4, 7, 8])
@pytest.mark.parametrize("mix", range(len(A.BATCH_POS)))
def test_batched_exact(ops, group, mix):
    errs = A.batched_errors(ops, group, 2, A.BATCH_POS[mix], BF, DEV)
    assert not errs, "\n".join(errs)


# ---------------------------------------------------------------------------------------------------------------- the fp8 caches
@pytest.mark.parametrize("group,nkv", A.DECODE_GROUPS, ids=lambda v: str(v))
@pytest.mark.parametrize("half", [0, 1], ids=["short", "long"])
def test_decode_kv8_exact(ops, group, nkv, half):
    cut = A.DECODE_POS.index(4095)
    _decode_table(ops, group, nkv, A.DECODE_POS[:cut] if half == 0 else A.DECODE_POS[cut:], BF, kv8=True)


@pytest.mark.parametrize("group", [4, 7])
@pytest.mark.parametrize("mix", range(len(A.BATCH_POS)))
def test_batched_kv8_exact(ops, group, mix):
    errs = A.batched_errors(ops, group, 2, A.BATCH_POS[mix], BF, DEV, kv8=True)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("pos", [2047, 2048, 4160])
def test_kv8_equals_the_16bit_kernel_on_the_dequantised_cache_at_long_contexts(ops, pos):
    """The property of tests/test_gpu_fp8kv.py (which stops at 256 rows) on general random inputs in the general combine: a random cache with
    row magnitudes over 2^-8 .. 2^8, a random q, a new row that is on the fp8 grid (K zero, V a dequantised row) -> the fp8 kernel's output
    is torch.equal to vl2_attn_decode's on the dequantised cache, and both caches hold the same values afterwards."""
    nkv, smax = 2, A.smax_for(pos)
    g = torch.Generator().manual_seed(pos)
    mk = lambda: (torch.randn(nkv, smax, 128, generator=g) * torch.exp2(torch.randint(-8, 9, (nkv, smax, 1), generator=g).float())).bfloat16()
    (k8, ks), (v8, vs) = KV.quant_cache_rows(mk()), KV.quant_cache_rows(mk())
    kd, vd = KV.dequant_cache(k8, ks), KV.dequant_cache(v8, vs)
    assert torch.equal(kd.bfloat16().float(), kd) and torch.equal(vd.bfloat16().float(), vd)
    cos, sin = (t.to(DEV) for t in (A.random_decode_inputs(4, nkv, pos, BF)[k] for k in ("cos", "sin")))
    for group in (4, 7):
        nh = nkv * group
        qkv = (torch.randn((nh + 2 * nkv) * 128, generator=g) * 1.5).bfloat16()
        qkv[nh * 128:(nh + nkv) * 128] = 0
        qkv[(nh + nkv) * 128:] = vd[:, (pos + 7) % smax].reshape(-1).bfloat16()
        qkv = qkv.to(DEV)
        kv8 = tuple(t.to(DEV) for t in (k8, v8, ks, vs))
        k16, v16 = kd.bfloat16().to(DEV), vd.bfloat16().to(DEV)
        out8 = torch.zeros(nh * 128, dtype=BF, device=DEV)
        out16 = torch.ones(nh * 128, dtype=BF, device=DEV)
        _, partial = A.partial_ws(nh * ((pos + 64) // 64) * 130, DEV)
        ops.attn_decode_kv8(qkv, kv8, cos, sin, partial, out8, nh, nkv, pos, A.SCALE)
        ops.attn_decode(qkv, k16, v16, cos, sin, partial, out16, nh, nkv, pos, A.SCALE)
        torch.cuda.synchronize()
        assert torch.equal(out8, out16), (group, pos, int((out8 != out16).sum()))
        assert torch.equal(KV.dequant_cache(kv8[0], kv8[2]), k16.float().cpu()) and torch.equal(KV.dequant_cache(kv8[1], kv8[3]), v16.float().cpu())


# ---------------------------------------------------------------------------------------------------------------- vl2_attn_decode_shared
@pytest.mark.parametrize("group,nkv", A.SHARED_GROUPS, ids=lambda v: str(v))
@pytest.mark.parametrize("case", A.SHARED_CASES, ids=lambda c: f"P{c[0]}_cap{c[1]}_nb{c[2]}")
def test_shared_prefix_exact(ops, case, group, nkv):
    P, own_cap, nb, owns = case
    err = A.SharedCase(P, own_cap, nb, owns, group, nkv, BF, DEV).run(ops)
    assert not err, err


# ---------------------------------------------------------------------------------------------------------------- vl2_attn_append
@pytest.mark.parametrize("case", A.APPEND_CASES, ids=lambda c: "P%d_n%d_g%d_kv%d" % c)
def test_append_exact(ops, case):
    err = A.AppendCase(*case, BF, DEV).run(ops)
    assert not err, err


# ---------------------------------------------------------------------------------------------------------------- graded weights
@pytest.mark.parametrize("group", [4, 7])
@pytest.mark.parametrize("pos", [2048, 4160, 16448])
def test_graded_weights_meet_the_fp64_softmax(ops, pos, group):
    """Random inputs, so the slices carry weights of every size: one case per combine regime, single and batched (the batch holds the request
    twice, around a short one), poison past pos, against the fp64 softmax at the project's tolerance."""
    nkv = 2
    d = A.random_decode_inputs(group, nkv, pos, BF)
    nh, smax = d["nh"], d["smax"]
    cos, sin = d["cos"].to(DEV), d["sin"].to(DEV)
    out = torch.zeros(nh * 128, dtype=BF, device=DEV)
    _, partial = A.partial_ws(nh * ((pos + 64) // 64) * 130, DEV)
    ops.attn_decode(d["qkv"].to(DEV), d["k"].to(DEV), d["v"].to(DEV), cos, sin, partial, out, nh, nkv, pos, A.SCALE)
    e = rel(out, d["ref"])
    print(f"graded weights pos {pos} group {group}: rel-L2 {e:.3e}")
    assert e < TOL_BF16_OUT, e
    s = A.random_decode_inputs(group, nkv, 70, BF, seed=1)
    pad = lambda t: torch.cat([t, torch.full((nkv, smax - t.shape[1], 128), float("nan"), dtype=BF)], 1)
    qkv = torch.stack([d["qkv"], s["qkv"], d["qkv"]]).to(DEV)
    kc = torch.stack([d["k"], pad(s["k"]), d["k"]]).to(DEV)
    vc = torch.stack([d["v"], pad(s["v"]), d["v"]]).to(DEV)
    outb = torch.zeros(3, nh * 128, dtype=BF, device=DEV)
    _, pb = A.partial_ws(3 * nh * (smax // 64) * 130, DEV)
    ops.attn_decode_batched(qkv, kc, vc, cos, sin, pb, outb, nh, nkv, torch.tensor([pos, 70, pos], dtype=torch.int32, device=DEV), smax, A.SCALE)
    assert torch.equal(outb[0], out) and torch.equal(outb[2], out)              # row stability on general inputs
    e = rel(outb[1], s["ref"])
    assert e < TOL_BF16_OUT, e
