"""The exact key-selecting cases of tests/attn_fwd_exact.py on the CPU: the generators proven (guard, selector coverage, the trap, the fp32
summation orders), the causal grid order and the launcher's plan restated and pinned, and the same case tables as
tests/test_gpu_attn_fwd_edges.py through the host emulator build of csrc/k_attn.h and csrc/k_attn2.h (tests/emu has every instance of both
files except the lab variant 5).  DESIGN.md section 18b."""
import os
import re

import pytest
import torch

from tests import attn_fwd_exact as F
from tests.emu.backend import emulated_backend

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = F.all_cases()
# What the emulator is too slow for (one workgroup at a time, every work-item a fiber; each runs in tests/test_gpu_attn_fwd_edges.py, nothing
# else is dropped): the CAUSAL_GRID row at B = 6 -- 57600 query rows, 450 workgroups per variant.  Its order (plain longest-first on one
# stream) is proven a permutation below, and the kernel arithmetic behind it is that of the B = 1 and B = 4 rows.
EMU_DROPPED = lambda c: c.table == "CAUSAL_GRID" and c.B == 6


# ------------------------------------------------------------------------------------------------------------ the generators themselves
def test_nothing_in_the_product_imports_the_helper():
    for d, _, files in os.walk(os.path.join(ROOT, "videollama2_amd")):
        for f in files:
            if f.endswith(".py"):
                assert "attn_fwd_exact" not in open(os.path.join(d, f)).read(), f


def test_attn_exact_tables_keep_their_bits():
    """The section 18 tables this file's helper sits beside."""
    from tests import attn_exact as A
    assert A.DECODE_POS == (0, 15, 16, 63, 64, 71, 2047, 2048, 2063, 4095, 4096, 4159, 4160, 16383, 16384, 16447, 16448)
    assert A.DECODE_GROUPS == ((4, 2), (7, 2), (8, 2), (1, 4)) and len(A.SHARED_CASES) == 9 and len(A.APPEND_CASES) == 12


def _one_request(c):
    inp = F.inputs(c, 0)
    g = c.H // c.nkv
    return inp.q[0].double(), inp.K[0].double().repeat_interleave(g, 0), inp.V[0].double().repeat_interleave(g, 0), inp.vis, F.scale_of(c)


@pytest.mark.parametrize("name", ["CAUSAL_S:D128c_B1_H2_kv1_nq200_nk200_off0_decoder", "FULL_64:D64f_B2_H2_kv2_nq150_nk150_off0_fused_pad",
                                  "FULL_96:D96f_B2_H2_kv2_nq200_nk200_off0_fused"])
def test_guard_fires_on_a_near_miss_a_count_of_three_a_wide_v_an_off_quantum_v_and_no_match(name):
    c = next(c for c in CASES if c.name == name)
    q, K, V, vis, sc = _one_request(c)
    F.guard(q, K, V, vis, sc)
    row = 100
    bad = q.clone()
    bad[0, row] = bad[0, row] / 2                         # -1024 per mismatched digit: -130 (D 128) .. -185 (D 64) in the exp2 domain
    with pytest.raises(AssertionError, match="non-selected key scores"):
        F.guard(bad, K, V, vis, sc)
    three = torch.tensor([[0b111 << 5] + [1] * (c.ndig - 1)])                       # digit 0 in {5, 6, 7}, the other digits 0: keys 5, 6, 7
    bad = q.clone()
    cc = c._replace(B=1, nq=1)
    bad[0, row] = F.q_rows(cc, three[None, None].expand(1, c.H, 1, c.ndig))[0, 0, 0].double()
    with pytest.raises(AssertionError, match="not a power of two"):
        F.guard(bad, K, V, vis, sc)
    with pytest.raises(AssertionError, match="2\\^24"):
        F.guard(q, K, V * 2.0 ** 22, vis, sc)
    with pytest.raises(AssertionError, match="multiple of the quantum"):
        F.guard(q, K, V + 0.125, vis, sc)
    bad = q.clone()
    bad[1, 3, :c.used] = F.NEG                            # no key matches any digit: the maximum is not 0
    with pytest.raises(AssertionError, match="head 1 row 3: the maximum score"):
        F.guard(bad, K, V, vis, sc)
    wide = F.inputs(c, 0).V * 2.0 ** 120                  # not representable in fp16: the operands must be exact in the element type
    with pytest.raises(AssertionError, match="not exact"):
        i2 = F.Inputs(c, 0)
        i2.V = wide
        i2.operands(torch.float16)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_selector_lists_cover_the_edges_of_every_table_row(c):
    """For every query row of the case: the single keys, the trap and the sets that must be in its list are in it, with the visible counts
    they are there for.  (The guard is asserted on the launched tensors by `Inputs`; this checks what the lists AIM at.)"""
    masks, count, order, n = F.row_lists(c)
    last = F.last_visible(c)
    K = {k: i for i, k in enumerate(F.KINDS)}
    inlist = torch.zeros(count.shape, dtype=torch.bool)
    for r in range(c.nq):
        inlist[r, order[r, :n[r]]] = True
    hit = lambda kind: F.matches(masks[:, K[kind]], max(c.nk, 1) + 64, c.ndig)          # (64 keys past nk: what a selector would match there)
    T = last // 64 * 64
    # single keys: key 0, the last visible key, the one before it, the first key of the last visible tile, the last of the tile before, 31 | 32, 63 | 64
    for kind, j in (("key0", last * 0), ("last", last), ("last-1", last - 1), ("tile_first", T), ("prev_tile_last", T - 1),
                    ("key31", last * 0 + 31), ("key32", last * 0 + 32), ("key63", last * 0 + 63), ("key64", last * 0 + 64)):
        vis = (j >= 0) & (j <= last)
        assert torch.equal(inlist[:, K[kind]], vis), (c.name, kind)
        assert bool((count[vis, K[kind]] == 1).all()) and bool(hit(kind)[torch.arange(c.nq)[vis], j[vis]].all()), (c.name, kind)
    # the trap: in EVERY row's list; it matches the last visible key and the key after it; visible count 1 (2 where digit 0 of `last` is 31)
    t = hit("trap")
    rows = torch.arange(c.nq)
    assert bool(inlist[:, K["trap"]].all()) and bool(t[rows, last].all()) and bool(t[rows, last + 1].all()), c.name
    d31 = (last & 31) == 31
    assert torch.equal(count[:, K["trap"]], torch.where(d31 & (last >= 31), 2, 1)), c.name
    # sets: keys 0 .. 31 and the last visible block, each cut by the diagonal or nk, whenever the cut leaves a power of two
    pow2 = lambda x: (x & (x - 1)) == 0
    cut0, cutl = torch.clamp(last, max=31) + 1, (last & 31) + 1
    assert torch.equal(inlist[:, K["block0"]], pow2(cut0)) and torch.equal(count[:, K["block0"]], cut0), c.name
    assert torch.equal(inlist[:, K["block_last"]], pow2(cutl)) and torch.equal(count[:, K["block_last"]], cutl), c.name
    assert torch.equal(inlist[:, K["block_prev"]], last >= 32) and bool((count[last >= 32, K["block_prev"]] == 32).all()), c.name
    if c.causal and c.nq >= 32 and c.off == 0 and c.nk >= c.nq:
        assert {1, 2, 4, 8, 16, 32} <= set(count[inlist[:, K["block_last"]], K["block_last"]].tolist()), c.name
    # spaced sets: 32 apart (two keys in every tile), 64 apart (one in every tile), 128 apart in the even / the odd tiles only
    tile = torch.arange(c.nk + 64) // 64
    for kind, parity in (("even_tiles", 0), ("even_tiles_hi", 0), ("odd_tiles", 1), ("odd_tiles_hi", 1)):
        m = hit(kind)
        assert bool(((tile[None, :] % 2 == parity) | ~m).all()), (c.name, kind)
    far = last >= 255
    for kind in ("apart32", "apart32_next", "apart64", "even_tiles", "even_tiles_hi", "odd_tiles", "odd_tiles_hi"):
        i = K[kind]
        assert bool(pow2(count[inlist[:, i], i]).all()), (c.name, kind)
        assert bool(inlist[far, i].all()) and bool((count[far, i] >= 2).all()), (c.name, kind)
    if bool(far.any()):
        m = hit("apart32")[far][:, :c.nk]
        assert bool(m[:, tile[:c.nk] % 2 == 0].any(1).all()) and bool(m[:, tile[:c.nk] % 2 == 1].any(1).all())          # both streams / groups are fed
        nxt = hit("apart32_next")[far]                                                          # ends one step of 32 short of the hidden key last + 1
        assert bool((nxt[torch.arange(int(far.sum())), last[far] + 1 - 32] | ((last[far] & 31) == 31)).all())
    if c.D == 128 and c.ndig == 4:
        assert bool(inlist[:, K["apart1024"]].all()) and bool(hit("apart1024")[rows, last].all()), c.name
    # every (request, head, row) picks from its list by an index that depends on all three
    p = F.picks(c, 0)
    if c.nq >= 64 and c.H >= 2:
        assert bool((p[:, 0] != p[:, 1]).any()) and bool((p[:, :, 1:] != p[:, :, :-1]).any()), c.name
    if c.B >= 2 and c.nq >= 64:
        assert bool((p[0] != p[1]).any()), c.name
    # every causal row runs the trap in at least one head of every request of every launch
    if c.causal:
        for rnd in range(F.rounds_of(c)):
            assert bool((F.picks(c, rnd) == K["trap"]).any(1).all()), (c.name, rnd)
    # WHAT IS LAUNCHED, not only what the lists hold: in every request, the kinds launched over the rounds of the case are exactly the kinds
    # that are in some row's list (independently of `rounds_of`, which counts the rounds this takes) ...
    listed = {k for r in range(c.nq) for k in order[r, :n[r]].tolist()}
    assert listed == set(torch.nonzero(inlist.any(0)).flatten().tolist())
    ran = F.launched(c)
    assert len(ran) == c.B and all(x == listed for x in ran), (c.name, [sorted(F.KINDS[k] for k in listed - x) for x in ran])
    # ... every case, full attention included, launches the trap in every request ...
    assert all(K["trap"] in x for x in ran), c.name
    # ... and at the class-token shapes and the one-row cases row 0 runs its whole list in every request
    if F.is_cls_shape(c) or c.nq == 1:
        for b in range(c.B):
            ran0 = set()
            for rnd in range(F.rounds_of(c)):
                ran0 |= set(F.picks(c, rnd)[b, :, 0].tolist())
            assert ran0 == set(order[0, :n[0]].tolist()), (c.name, b)
    if F.is_cls_shape(c):
        l0 = {F.KINDS[i] for i in order[0, :n[0]].tolist()}
        assert {"key0", "block0", "block_prev", "last", "trap"} <= l0           # key 0 alone; a set with key 0; sets and keys without it


def test_reference_is_the_mean_of_the_selected_rows_in_three_fp32_orders():
    c = next(c for c in CASES if c.table == "EXTEND" and c.nq == 200)
    inp = F.inputs(c, 0)
    g = c.H // c.nkv
    q, K, V = inp.q[0].double(), inp.K[0].double().repeat_interleave(g, 0), inp.V[0].repeat_interleave(g, 0)
    gen = torch.Generator().manual_seed(3)
    seen = set()
    for h in range(c.H):
        for r in range(h % 2, c.nq, 2):
            hit = ((K[h] @ q[h, r]) == 0) & inp.vis[r]
            rows = V[h][hit]
            assert len(rows) == int(inp.count[0, h, r])
            seen.add(len(rows))
            for o in (torch.arange(len(rows)), torch.arange(len(rows) - 1, -1, -1), torch.randperm(len(rows), generator=gen)):
                acc = torch.cumsum(rows[o], 0, dtype=torch.float32)[-1] * torch.tensor(1.0 / len(rows), dtype=torch.float32)
                assert torch.equal(acc, inp.ref[0, h, r].float())
    assert {1, 2, 4, 8, 32} <= seen


# ------------------------------------------------------------------------------------------------------------ the plan the tables rely on
def test_causal_grid_order_is_a_permutation_and_the_grid_table_reaches_all_three_orders():
    for file, NS in ((1, 1), (2, 1), (2, 2)):
        for nqb in range(1, 41):
            for G in range(1, 641):
                got = sorted(F.causal_qb(r * G + (G - 1) * (r & 1), nqb, G, NS, file) for r in range(nqb))         # (any g of rank r: x = r G + g)
                assert got == list(range(nqb)), (file, NS, nqb, G)
    assert all(sorted(F.causal_qb(r * G, nqb, G, 1, 2, skip=False) for r in range(nqb)) == list(range(nqb)) for nqb in range(1, 41) for G in (1, 32, 128, 300))
    grid = [c for c in CASES if c.table == "CAUSAL_GRID"]
    nqb = 3
    assert [(c.B, (c.nq + 127) // 128, c.H * c.B) for c in grid] == [(1, nqb, 32), (4, nqb, 128), (6, nqb, 192)]
    orders = {(c.B, NS): F.causal_order(nqb, c.H * c.B, NS) for c in grid for NS in (1, 2)}
    assert orders == {(1, 1): "long_then_ascending", (1, 2): "long_then_ascending", (4, 1): "partnered_first", (4, 2): "longest_first",
                      (6, 1): "longest_first", (6, 2): "longest_first"}
    # B = 4 on one stream: the n2 = 1 block that gets a partner (the second longest) first, then the longest alone, then the shortest
    assert [F.causal_qb(r * 128, 3, 128, 1) for r in range(3)] == [1, 2, 0]
    assert [F.causal_qb(r * 128, 3, 128, 2) for r in range(3)] == [2, 1, 0] and [F.causal_qb(r * 32, 3, 32, 1) for r in range(3)] == [2, 1, 0]


def test_the_launch_plan_the_tables_rely_on():
    """Which shapes are class-token shapes, the 352 threshold, the instances the tables reach -- and the launcher's lines that `F.instance`,
    `F.is_cls_shape` and `F.causal_qb` restate, in the product and in the emulator: a change to a plan cannot hollow the tables out unseen."""
    cls = sorted((c.nq, c.layout) for c in CASES if F.is_cls_shape(c))
    assert cls == [(65, "fused"), (129, "fused"), (193, "fused"), (257, "fused"), (577, "fused")]
    plain129 = next(c for c in CASES if c.D == 64 and c.nq == 129 and c.H != c.nkv)
    assert F.instance(plain129, 0) == "attn2<64f,NS1>"                         # group 2: the plain tiling under variant 0
    rem = {c.nq: (c.nq - 1) & 127 for c in CASES if F.is_cls_shape(c)}
    assert {n for n, r in rem.items() if r == 0} == {129, 257} and {n for n, r in rem.items() if 0 < r <= 96} == {65, 193, 577}
    auto = {c.H: F.instance(c, 0) for c in CASES if c.table == "CAUSAL_AUTO"}
    assert auto == {176: "attn2<128c,NS2>", 177: "attn2<128c,NS1>"} and 2 * 176 == 352
    assert all(F.instance(c, 0) == "attn2<128c,NS2>" for c in CASES if c.D == 128 and c.causal and c.table != "CAUSAL_AUTO")
    reached = {F.instance(c, v) for c in CASES for v in F.variants_of(c)}
    assert reached == {"attn<64f>", "attn<64c>", "attn<128f>", "attn<128c>", "attn<128c,NG2>", "attn<96f>",
                       "attn2<64f,NS1>", "attn2<64c,NS1>", "attn2<128f,NS1>", "attn2<128c,NS1>", "attn2<64f,CLS,NS1>",
                       "attn2<64f,NS2>", "attn2<64c,NS2>", "attn2<128f,NS2>", "attn2<128c,NS2>", "attn2<64f,CLS,NS2>"}
    assert {F.instance(c, v) for c in F.fp16_cases() for v in F.variants_of(c)} == reached                  # the fp16 build's share runs every instance
    assert {c.table for c in F.fp16_cases()} == {c.table for c in CASES} and {65, 129, 577} <= {c.nq for c in F.fp16_cases() if F.is_cls_shape(c)}
    for kernel_file in ("attn", "attn2"):                                       # every operand layout at least once per kernel file
        lay = {c.layout for c in CASES for v in F.variants_of(c) if F.instance(c, v).startswith(kernel_file + "<")}
        assert lay == {"fused", "decoder", "batch"}
        assert any(c.rpad for c in CASES for v in F.variants_of(c) if F.instance(c, v).startswith(kernel_file + "<") and c.layout != "fused")
    squash = lambda s: re.sub(r"\s+", "", re.sub(r"//[^\n]*", "", s))
    abi = squash(open(os.path.join(ROOT, "videollama2_amd", "csrc", "vl2_abi.hip")).read())
    emu = squash(open(os.path.join(ROOT, "tests", "emu", "emu_kernels.cpp")).read())
    shape = "D==64&&!causal&&nq==nk&&nk>64&&(nk-1)%64==0&&group==1"
    why = ("a line of the launch plan that tests/attn_fwd_exact.py restates has changed: re-check `F.instance`, `F.is_cls_shape` and `F.causal_qb` "
           "against the new source (and what the tables then reach) BEFORE updating the pinned text")
    for src in (abi, emu):
        assert "constboolcls_peel=variant==0&&" + shape in src, why
        assert "if(variant==0&&D==128&&causal&&(long)((nq+127)/128)*H<=352)variant=4;if(variant==0&&(D==64||D==128))variant=3;" in src, why
        assert "(nq-1+127)/128+((((nq-1)&127)==0||((nq-1)&127)>96)?1:0)" in src, why
    assert "constboolcls_peel4=variant==4&&" + shape in abi and "constboolpeel4=" + shape in emu, why
    k2 = squash(open(os.path.join(ROOT, "videollama2_amd", "csrc", "k_attn2.h")).read())
    assert "qb=(SKIP&&nqb*G>(NS==2?256:512))?nqb-1-r:(r<nfirst?nqb-1-r:r-nfirst);" in k2, why
    assert "if(SKIP&&NS==1&&nqb*G<=512&&nqb>nfirst){" in k2 and "qb=r<n2?nqb-1-alone-r:r<nfirst?nqb-1-(r-n2):r-nfirst;" in k2, why
    assert "constboolcls_in_last=cls_rem!=0&&cls_rem<=96;" in k2, why
    k1 = squash(open(os.path.join(ROOT, "videollama2_amd", "csrc", "k_attn.h")).read())
    assert "qb=r<nfirst?nqb-1-r:r-nfirst;" in k1, why


# ------------------------------------------------------------------------------------------------------------ the case tables on the emulator
def _emu_groups():
    """The tables in groups of a few seconds each."""
    groups = {}
    for c in CASES:
        if EMU_DROPPED(c):
            continue
        key = c.table
        if c.table == "CAUSAL_GRID":
            key = f"CAUSAL_GRID_B{c.B}"
        elif c.table == "FULL_64":
            key = "FULL_64_N577" if c.nq == 577 else "FULL_64"
        groups.setdefault(key, []).append(c)
    return groups


_GROUPS = _emu_groups()


@pytest.mark.parametrize("group", sorted(_GROUPS))
def test_attn_fwd_edges_on_the_emulator(group):
    """Every case of the tables (but EMU_DROPPED), every round, every variant that serves it: torch.equal to the fp64 softmax rounded once,
    the sentinel frame and q, k, v untouched."""
    errs, n = [], 0
    with emulated_backend():
        from videollama2_amd import ops
        for c in _GROUPS[group]:
            errs += F.run_case(ops, c, BF, "cpu")
            n += F.rounds_of(c) * len(F.variants_of(c))
    assert not errs, f"{len(errs)} of {n} launches failed:\n" + "\n".join(errs[:12])


@pytest.mark.parametrize("spec", F.GRADED, ids=lambda s: "D%d%s_N%d" % (s[0], "c" if s[1] else "f", s[5]))
def test_graded_weights_on_the_emulator(spec):
    """Random inputs (weights of every size, rescale factors inside (0, 1), the deferred rescale) per (row, head) against the fp64 softmax,
    within GRADED_MARGIN of the rounding model's largest per-row error (tests/test_gpu_attn_fwd_edges.py has the reasoning)."""
    c = F.graded_case(*spec)
    q, K, V = F.graded_inputs(c, BF)
    ref, model = F.graded_reference(c, q, K, V, BF)
    e_model = float(F.row_rel(model[..., :c.used], ref[..., :c.used]).max())
    opnd = F.Operands(c, q, K, V, BF, "cpu")
    Wo = c.H * c.D + 8
    with emulated_backend():
        from videollama2_amd import ops
        for v in F.variants_of(c):
            o = F.launch(ops, c, opnd, v, "cpu")
            y = torch.as_strided(o.view(-1), (c.B, c.H, c.nq, c.D), ((c.nq + 2) * Wo, c.D, Wo, 1), Wo)
            e = float(F.row_rel(y[..., :c.used], ref[..., :c.used]).max())
            print(f"graded {c.name} variant {v}: kernel {e:.3e} model {e_model:.3e}")
            assert e <= F.GRADED_MARGIN * e_model, (c.name, v, e, e_model)
            assert bool((y[..., c.used:] == 0).all()) and opnd.intact()
