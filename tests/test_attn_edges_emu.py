"""The exact key-selecting attention cases of tests/attn_exact.py on the CPU: the generators proven (guard, selectors, RoPE tables, the fp8
round trip, the restated split plans and what the tables reach), and the same case tables as tests/test_gpu_attn_edges.py through the host
emulator build of the kernel sources (tests/emu) for the entry points it has: vl2_attn_decode, vl2_attn_decode_batched and the lab form
vl2_attn_decode_fused.  The fp8-KV, shared-prefix and append kernels are not in the emulator: they run on the GPU only.  DESIGN.md section 18."""
import pytest
import torch

from tests import attn_exact as A
from tests.emu.backend import emulated_backend

BF = torch.bfloat16
# What the emulator is too slow for (every one of them runs in tests/test_gpu_attn_edges.py; nothing else is dropped): the contexts of 257 and
# more slices at the groups 8 and 1 -- the weight chunks of the combine are per q head and do not know the group, and the groups 4 and 7 run them
# here -- and the second batched mix, which holds three such contexts, at group 7.
EMU_DROPPED_DECODE = lambda group, pos: pos >= 16383 and group in (8, 1)
EMU_DROPPED_BATCH = lambda group, mix: mix == 1 and group == 7


# ------------------------------------------------------------------------------------------------------------ the generators themselves
def test_nothing_in_the_product_imports_the_helper():
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "videollama2_amd")
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                assert "attn_exact" not in open(os.path.join(d, f)).read(), f


def test_guard_fires_on_a_near_miss_a_count_of_three_and_a_wide_v():
    r = A.Request(4, 2, 100)
    K, V = r.keys64()
    A.guard(r.q, K, V, 4)
    q = r.q.clone()
    q[0] = q[0] / 2                                     # -1024 per mismatch: -130 in the exp2 domain
    with pytest.raises(AssertionError, match="non-selected key scores"):
        A.guard(q, K, V, 4)
    q = r.q.clone()
    q[0] = A.q_pattern(A.digits(7), A.salt(0, 0))
    q[0, A.salt(0, 0) + 5] = q[0, A.salt(0, 0) + 6] = 0.0      # digit 0 in {5, 6, 7}: three keys
    with pytest.raises(AssertionError, match="not a power of two"):
        A.guard(q, K, V, 4)
    with pytest.raises(AssertionError, match="2\\^24"):
        A.guard(r.q, K, V * 2.0 ** 22, 4)
    with pytest.raises(AssertionError, match="multiple of the quantum"):
        A.guard(r.q, K, V + 0.125, 4)
    q = r.q.clone()
    q[0] = A.NEG                                        # no key matches any digit: the maximum is not 0
    with pytest.raises(AssertionError, match="maximum score"):
        A.guard(q, K, V, 4)


def test_selectors_cover_the_edge_rows_and_cut_sets_at_every_table_position():
    cut = set()
    for pos in A.DECODE_POS:
        sels = A.selectors(pos)
        keys = torch.arange(pos + 1)
        singles = {int(keys[A.matches(s, keys)][0]) for s in sels if None not in s}
        assert {0, pos, max(pos - 1, 0), pos // 64 * 64} <= singles, pos
        if pos >= 64:
            assert {pos // 64 * 64 - 1, 63, 64} <= singles, pos
        for s in sels:
            n = int(A.matches(s, keys).sum())
            assert n >= 1 and n & (n - 1) == 0, (pos, s, n)
            if None in s and n < 32 ** sum(d is None for d in s):
                cut.add(n)
        if pos >= 2047:
            counts = {s: int(A.matches(s, keys).sum()) for s in sels if None in s}
            assert 32 in counts.values() and 1024 in counts.values(), (pos, counts)               # one slice; 16 slices; 1024 keys
            assert any(s[2] is None and s[0] is not None and n >= 2 for s, n in counts.items()), (pos, counts)     # keys 1024 apart
    assert {1, 8, 16} <= cut, cut                        # sets that the context cuts to 16, 8 and 1 of their members


def test_rope_tables_are_exact_rotations_and_the_inverse_round_trips():
    cos, sin = A.rope_tables(9)
    assert set(cos.flatten().tolist()) == {1.0, 0.0, -1.0} and bool((cos * cos + sin * sin == 1).all())
    assert not torch.equal(cos[3], cos[4]) and not torch.equal(cos[4, :-1], cos[4, 1:])          # a neighbouring row or column is another rotation
    w = torch.randn(3, 128, dtype=torch.float64)
    for p in range(9):
        assert torch.equal(A.rope(A.unrope(w, cos[p].double(), sin[p].double()), cos[p].double(), sin[p].double()), w)
    r = A.Request(7, 2, 4160)
    wrong = A.rope(r.qkv64[:r.nh * 128].view(r.nh, 128), *(t[4159].double() for t in A.rope_tables(4161)))
    assert not torch.equal(wrong, r.q)                  # the neighbouring table row does not give the query


def test_fp8_round_trip_of_the_exact_rows():
    for elem in (torch.bfloat16, torch.float16):
        r = A.Request(4, 2, 200)
        k, v = A.poisoned_cache(r, 256, elem)
        k8, v8, ks, vs = A.kv8_of(k, v, 200)            # asserts the round trip
        assert bool((k8[:, 200:] == 0x7F).all()) and bool(ks[:, 200:].isnan().all()) and bool(k[:, 200:].isnan().all())
        assert len(set(vs[:, :200].flatten().tolist())) > 1, "the V rows must carry different scales"


def test_reference_is_the_mean_of_the_selected_rows_in_three_fp32_orders():
    r = A.Request(4, 2, 4160, sels=[s for s in A.selectors(4160) if None in s] + [A.digits(4160)])
    K, V = r.keys64()
    ref, counts = r.reference()
    assert max(counts) >= 1024 and min(counts) == 1
    g = torch.Generator().manual_seed(3)
    for h in (0, counts.index(max(counts))):
        hit = (K[h // 4] @ r.q[h]) == 0
        rows = V[h // 4][hit].float()
        for order in (torch.arange(len(rows)), torch.arange(len(rows) - 1, -1, -1), torch.randperm(len(rows), generator=g)):
            acc = torch.cumsum(rows[order], 0, dtype=torch.float32)[-1] * (1.0 / len(rows))
            assert torch.equal(acc, ref[h * 128:(h + 1) * 128].float())      # (fp64 leaves 1e-76 where the mean is 0)


def test_split_plans_restated_and_what_the_tables_reach():
    from videollama2_amd import ops
    for P, own_cap, nb, owns in A.SHARED_CASES:
        assert A.shared_splits(P)[1] == ops.shared_prefix_splits(P)
        assert all(0 <= o < own_cap for o in owns)
    sp = {P: A.shared_splits(P) for P, *_ in A.SHARED_CASES}
    assert sp[1] == (128, 1) and sp[128] == (128, 1) and sp[129] == (128, 2) and sp[3072] == (128, 24) and sp[3073] == (192, 17)
    live = {ops.shared_live_slices(P, P + o) for P, cap, nb, owns in A.SHARED_CASES for o in owns}
    assert {32, 33} <= live                             # the last early combine and the first general one
    assert {nb for _, _, nb, _ in A.SHARED_CASES} == {1, 5, 33} and {c for _, c, _, _ in A.SHARED_CASES} >= {64, 512, 576}
    plans = {c: A.append_splits(*c) for c in A.APPEND_CASES}
    assert max(n for _, n in plans.values()) == 32 and min(n for _, n in plans.values()) == 1
    assert {n * g for _, n, g, _ in A.APPEND_CASES} >= {128, 132, 126, 133}
    P, n, g, nkv = 90, 64, 4, 2                         # the early return: block 0's last row ends before split 1 begins
    chunk, ns = plans[(P, n, g, nkv)]
    assert ns == 2 and P + 127 // g < chunk <= P + n - 1
    slices = {(p + 64) // 64 for p in A.DECODE_POS}
    assert {1, 2, 32, 33, 64, 65, 66, 256, 257, 258} <= slices


# ------------------------------------------------------------------------------------------------------------ the case tables on the emulator
@pytest.mark.parametrize("group,nkv", A.DECODE_GROUPS, ids=lambda v: str(v))
def test_decode_edges_on_the_emulator(group, nkv):
    errs, n = [], 0
    with emulated_backend():
        from videollama2_amd import ops
        for pos in A.DECODE_POS:
            if EMU_DROPPED_DECODE(group, pos):
                continue
            st = A.DecodeState(group, nkv, pos, BF, "cpu")
            for form, rnd in A.decode_launches(st.rounds):
                err = A.run_decode(ops, st, form, rnd)
                n += 1
                if err:
                    errs.append(err)
    assert not errs, f"{len(errs)} of {n} launches failed:\n" + "\n".join(errs[:12])


@pytest.mark.parametrize("group,nkv", [(4, 2), (7, 2)], ids=lambda v: str(v))
def test_fused_decode_edges_on_the_emulator(group, nkv):
    errs = []
    with emulated_backend():
        from videollama2_amd import ops
        for pos in A.DECODE_POS:
            st = A.DecodeState(group, nkv, pos, BF, "cpu")
            cnt = torch.zeros(nkv, dtype=torch.int32)
            err = A.run_decode(ops, st, "cap_smax", pos % st.rounds, fused_cnt=cnt)
            if err:
                errs.append(err)
            assert cnt.tolist() == [((pos + 64) // 64) * ((group + 3) // 4)] * nkv
    assert not errs, "\n".join(errs[:12])


@pytest.mark.parametrize("group,mix", [(g, m) for g in (4, 7) for m in range(len(A.BATCH_POS)) if not EMU_DROPPED_BATCH(g, m)])
def test_batched_edges_on_the_emulator(group, mix):
    with emulated_backend():
        from videollama2_amd import ops
        errs = A.batched_errors(ops, group, 2, A.BATCH_POS[mix], BF, "cpu")
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("group", [4, 7])
def test_graded_weights_on_the_emulator(group):
    """Random inputs (weights of every size) at the shortest general-combine position, against the fp64 softmax."""
    from tests.util import TOL_BF16_OUT, rel
    pos, nkv = 2048, 2
    d = A.random_decode_inputs(group, nkv, pos, BF)
    with emulated_backend():
        from videollama2_amd import ops
        out = torch.zeros(d["nh"] * 128, dtype=BF)
        _, partial = A.partial_ws(d["nh"] * ((pos + 64) // 64) * 130, "cpu")
        ops.attn_decode(d["qkv"], d["k"].clone(), d["v"].clone(), d["cos"], d["sin"], partial, out, d["nh"], nkv, pos, A.SCALE)
    e = rel(out, d["ref"])
    assert e < TOL_BF16_OUT, e
