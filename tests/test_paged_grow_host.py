"""Growing reservations page by page and preemption by swap, host side only (no launch): `paging.rows_next`,
`plan_growth` and `admit_grow` against brute-force restatements over small exhaustive ranges, their invariants, a pure-Python simulation of
whole queues (tests/paged_grow_sim.py) that always drains and conserves pages, the declaration of vl2_kv_pages_move against the ctypes table,
the argument refusals of the library and of `ops.kv_pages_move`, the batcher's refusals before any kernel, and -- with recording stubs on the
emulated backend -- the real batcher's schedule, table rows and swap launches against the simulation."""
import ctypes
import itertools
import os
import random
import re

import pytest
import torch

from oracle import vl2_oracle as O
from tests.paged_grow_sim import simulate
from videollama2_amd.paging import PagePool, admit_grow, pages_for, pages_needed, plan_growth, rows_next

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
NAME = "vl2_kv_pages_move"
SS = (1, 63, 64, 65)


# ---------------------------------------------------------------------------------------------------------------- rows_next
def test_rows_next_counts_the_rows_a_step_writes_and_ends_on_the_whole_reservation():
    for msl in (66, 128, 200, 256):
        for S in SS:
            max_new_cap = msl - S + 1                                  # submit's clamp
            rows = 0
            for k in range(max_new_cap):                               # step k emits token k and writes row S + k (nothing past the cache end)
                rows = max(rows, min(S + k + 1, msl))
                assert rows_next(S, k, msl) == rows, (msl, S, k)
                assert rows_next(S, k, msl) - rows_next(S, max(k - 1, 0), msl) in (0, 1)
            for max_new in range(1, max_new_cap + 1):
                assert pages_for(rows_next(S, max_new - 1, msl)) == pages_needed(S, max_new, msl), (msl, S, max_new)
    assert [pages_for(r) for r in (0, 1, 64, 65, 128, 129)] == [0, 1, 1, 2, 2, 3]


# ---------------------------------------------------------------------------------------------------------------- plan_growth
def _brute_plan(in_flight, free):
    """The smallest newest suffix of victims after which every survivor's grant fits what is free plus what the victims held."""
    reqs = sorted(in_flight)
    want = lambda r: max(0, -(-r[2] // 64) - r[1])
    for v in range(len(reqs)):
        keep, out = reqs[:len(reqs) - v], reqs[len(reqs) - v:]
        if sum(want(r) for r in keep) <= free + sum(r[1] for r in out):
            return [(r[0], want(r)) for r in keep if want(r)], [r[0] for r in reversed(out)]
    return None


def _states():
    """(pages held, rows_next) of a request of S prompt rows about to take step n: it holds what its previous step needed."""
    out = []
    for S in SS:
        for n in (0, 63, 64):
            held = pages_for(rows_next(S, n - 1, 256)) if n else pages_for(rows_next(S, 0, 256))
            out.append((held, rows_next(S, n, 256)))
    return sorted(set(out))


def test_plan_growth_equals_the_brute_force_and_keeps_its_invariants():
    states = _states()
    assert any(pages_for(rows) > held for held, rows in states) and any(pages_for(rows) == held for held, rows in states)
    n_cases = n_preempting = 0
    for k in range(1, 5):
        for combo in itertools.product(states, repeat=k):
            orders = random.Random(hash(combo) & 0xffff).sample(range(10), k)           # the order of the list is not the admission order
            in_flight = [(o, held, rows) for o, (held, rows) in zip(orders, combo)]
            total = sum(held for held, _ in combo)
            for n_pages in range(2, 9):
                free = n_pages - 1 - total
                if free < 0:
                    continue
                want = _brute_plan(in_flight, free)
                if want is None:                                         # the oldest alone does not fit: submit's check excludes it
                    with pytest.raises(RuntimeError, match="nobody left to preempt"):
                        plan_growth(in_flight, free)
                    continue
                grants, victims = plan_growth(in_flight, free)
                assert (grants, victims) == want, (in_flight, free)
                n_cases += 1
                n_preempting += bool(victims)
                by = {o: (held, rows) for o, held, rows in in_flight}
                oldest_first = sorted(by)
                assert victims == sorted(oldest_first[len(by) - len(victims):], reverse=True)       # exactly the newest suffix, newest first
                assert min(by) not in victims                                                      # never the oldest
                if sum(max(0, pages_for(rows) - held) for held, rows in by.values()) <= free:
                    assert victims == []                                                           # none while the free pages suffice
                granted = dict(grants)
                assert [o for o, _ in grants] == sorted(granted) and all(n > 0 for n in granted.values())
                for o, (held, rows) in by.items():
                    if o not in victims:
                        assert held + granted.get(o, 0) == pages_for(rows)                         # survivors hold ceil(rows_next / 64)
                    else:
                        assert o not in granted
                assert sum(granted.values()) <= free + sum(by[o][0] for o in victims)
    assert n_cases > 5000 and n_preempting > 500, (n_cases, n_preempting)               # the ranges really reach both outcomes


# ---------------------------------------------------------------------------------------------------------------- admit_grow
def _brute_admit(needs, free_slots, free_pages, n_in_flight):
    """The largest k such that every request of the first k passes, in turn, the three conditions stated in the issue."""
    best = 0
    for k in range(1, len(needs) + 1):
        slots, pages, flying, ok = free_slots, free_pages, n_in_flight, True
        for need in needs[:k]:
            joins = slots > 0 and need <= pages and (n_in_flight == 0 or pages - need >= flying + 1)
            if not joins:
                ok = False
                break
            slots, pages, flying = slots - 1, pages - need, flying + 1
        if not ok:
            break
        best = k
    return best


def test_admit_grow_equals_the_brute_force():
    seen = set()
    for k in range(0, 5):
        for needs in itertools.product((1, 2, 3), repeat=k):
            for free_slots in range(0, 5):
                for free_pages in range(0, 8):
                    for flying in range(0, 4):
                        got = admit_grow(list(needs), free_slots, free_pages, flying)
                        assert got == _brute_admit(needs, free_slots, free_pages, flying), (needs, free_slots, free_pages, flying)
                        seen.add(got)
    assert seen == {0, 1, 2, 3, 4}
    assert admit_grow([3], 1, 3, 0) == 1                # the headroom rule is waived while nothing is in flight
    assert admit_grow([3], 1, 4, 1) == 0                # ... and holds otherwise: 2 in flight afterwards need 2 free pages
    assert admit_grow([3], 1, 5, 1) == 1
    assert admit_grow([1, 1, 1, 1], 4, 4, 0) == 4       # ... for the whole step: an idle batcher fills its slots on the prompts' pages
    assert admit_grow([1, 1], 2, 4, 1) == 1             # one in flight: the first leaves 3 >= 2, the second would leave 2 < 3
    assert admit_grow([4, 1], 2, 3, 0) == 0             # strict FIFO: nobody passes a head that does not fit
    assert admit_grow([1], 0, 7, 1) == 0


# ---------------------------------------------------------------------------------------------------------------- whole queues
def test_simulated_queues_always_drain_and_conserve_pages():
    rng = random.Random(20)
    preempting = resumed = 0
    for trial in range(300):
        msl = rng.choice((200, 256))
        n_pages = rng.randint(3, 9)
        max_slots = rng.randint(1, 4)
        reqs = []
        while len(reqs) < rng.randint(1, 9):
            S, budget = rng.choice(SS + (5, 70, 129)), rng.choice((1, 2, 8, 64, 70, 130, 2048))
            if pages_needed(S, min(budget, msl - S + 1), msl) <= n_pages - 1:
                reqs.append((S, budget, rng.choice((1, 3, 64, 100, 5000))))
        arrivals = sorted(rng.randint(0, 40) for _ in reqs) if trial % 2 else None
        out = simulate(reqs, n_pages, max_slots, msl, arrivals)            # asserts conservation and the per-request bound at every step
        assert sorted(out["finish"]) == list(range(len(reqs)))
        assert max(out["in_flight"]) <= max_slots and out["resumes"] == out["preemptions"]
        preempting += out["preemptions"] > 0
        resumed += out["resumed_elsewhere"]
    assert preempting >= 10 and resumed > 0, (preempting, resumed)        # the trials really reach preemption


def test_the_schedules_of_the_gpu_tests_do_what_those_tests_need():
    """tests/test_gpu_paged_grow.py chose its lengths on this simulation: the occupancy case and the preemption case."""
    from tests.test_gpu_paged_grow import OCCUPANCY, PREEMPT
    occ = simulate(OCCUPANCY["requests"], OCCUPANCY["n_pages"], 4, 256)
    assert all(pages_needed(S, b, 256) == 3 for S, b, _ in OCCUPANCY["requests"]) and OCCUPANCY["n_pages"] == 5
    assert occ["in_flight"][0] == 4 and occ["preemptions"] == 0
    pre = simulate(PREEMPT["requests"], PREEMPT["n_pages"], PREEMPT["max_slots"], 256)
    assert pre["preemptions"] >= 1 and pre["resumes"] == pre["preemptions"] and len(pre["finish"]) == len(PREEMPT["requests"])


# ---------------------------------------------------------------------------------------------------------------- the entry point
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib
    return _lib.load()


def _declared(name):
    header = open(os.path.join(ROOT, "include", "vl2hip.h")).read()
    product = re.sub(r"#ifdef VL2_EXPERIMENTAL.*?#endif /\* VL2_EXPERIMENTAL[^\n]*", "", header, flags=re.S)
    m = re.search(r"\b(int32_t|int64_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", product)
    assert m, f"{name} is not declared in the product part of include/vl2hip.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        args.append(ctypes.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
    return CTYPE[m.group(1)], args


def test_header_declaration_matches_the_ctypes_table(lib):
    from videollama2_amd import _lib
    assert set(_lib.PAGED_SWAP_SIGNATURES) == {NAME}
    ret, args = _declared(NAME)
    assert ret is ctypes.c_int32 and args == _lib.PAGED_SWAP_SIGNATURES[NAME]
    assert getattr(lib, NAME).argtypes == args and getattr(lib, NAME).restype is ctypes.c_int32
    assert NAME in _lib.EXPORTS and NAME not in _lib.SIGNATURES                # the emulator's symbol set is unchanged
    assert not any(NAME in t for t in (_lib.PAGED_KV_SIGNATURES, _lib.PAGED_PREFIX_SIGNATURES, _lib.PAGED_FP8KV_SIGNATURES))
    for path in (_lib.LIB_PATH, _lib.LIB_PATHS["fp16"], _lib.LAB_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), NAME), path
    assert lib.vl2_version() == 7


def test_library_refuses_bad_arguments_before_launching(lib):
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)          # stand-in device pointers: every case fails its checks first

    def move(pool=p, arena=p, ids=p, n=3, n_pages=9, page_bytes=32768, to_arena=1):
        return lib.vl2_kv_pages_move(pool, arena, ids, n, n_pages, page_bytes, to_arena, None)

    cases = [(k, -1, "null pointer") for k in (dict(pool=None), dict(arena=None), dict(ids=None))]
    cases += [(dict(n=-1), -1, "n -1 outside"), (dict(n=65536), -1, "n 65536 outside"), (dict(n_pages=0), -2, "n_pages 0"),
              (dict(page_bytes=0), -2, "page_bytes 0 must be"), (dict(page_bytes=-16), -2, "page_bytes -16 must be"),
              (dict(page_bytes=520), -2, "page_bytes 520 must be a positive multiple of 16"), (dict(pool=odd), -2, "16-byte aligned"),
              (dict(arena=odd), -2, "16-byte aligned")]
    for to_arena in (0, 1):
        for kw, rc, msg in cases:
            assert move(to_arena=to_arena, **kw) == rc, (kw, lib.vl2_last_error_string().decode())
            err = lib.vl2_last_error_string().decode()
            assert msg in err and NAME in err, (kw, err)
        assert move(n=0, to_arena=to_arena) == 0                    # no pages: no error and no launch
    assert move(n=0, n_pages=0) == -2                               # ... but the checks come first


def test_wrapper_refuses_before_the_library_is_touched(monkeypatch):
    from videollama2_amd import _lib, ops

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    bf, i32, u8, f32 = torch.bfloat16, torch.int32, torch.uint8, torch.float32
    nkv = 2
    rows = lambda n=12, dt=bf: torch.zeros(n, nkv, 64, 128, dtype=dt)
    scales = lambda n=12: torch.ones(n, nkv, 64, dtype=f32)
    ids = torch.tensor([3, 1, 2], dtype=i32)
    for pool, arena in ((rows(), rows(4)), (rows(dt=u8), rows(4, u8)), (scales(), scales(4))):
        good = dict(pool=pool, arena=arena, page_ids=ids, to_arena=True)
        cases = [(dict(pool=pool.double()), TypeError, "pool must be .* rows, torch.uint8 codes or torch.float32 row scales"),
                 (dict(arena=arena.to(torch.int16)), TypeError, "arena must be"), (dict(page_ids=ids.long()), TypeError, "page_ids must be torch.int32"),
                 (dict(pool=pool[:, :, :32]), ValueError, "pool must be \\[n_pages, nkv, 64"),
                 (dict(pool=pool.reshape(12, -1)), ValueError, "pool must be \\[n_pages, nkv, 64"),
                 (dict(pool=torch.cat([pool, pool])[::2]), ValueError, "pages must be contiguous"),
                 (dict(arena=torch.cat([arena, arena])[::2]), ValueError, "pages must be contiguous"),
                 (dict(page_ids=torch.zeros(6, dtype=i32)[::2]), ValueError, "page_ids must be a contiguous int32 vector"),
                 (dict(page_ids=ids[None]), ValueError, "page_ids must be a contiguous int32 vector"),
                 (dict(arena=arena[:2]), ValueError, "arena must hold at least 3 pages"),
                 (dict(arena=arena[:, :1].contiguous()), ValueError, "arena must hold at least 3 pages"),
                 (dict(arena=arena.reshape(4, -1)), ValueError, "arena must hold at least 3 pages"),
                 ({}, ValueError, "must be a device tensor")]
        for to_arena in (True, False):
            for kw, exc, msg in cases:
                with pytest.raises(exc, match=msg):
                    ops.kv_pages_move(**{**good, **kw, "to_arena": to_arena})
    with pytest.raises(TypeError, match="pool must be"):
        ops.kv_pages_move(rows(dt=torch.float16), rows(4, torch.float16), ids, True)        # the other build's 16-bit type


# ---------------------------------------------------------------------------------------------------------------- the batcher
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


@pytest.fixture()
def stubbed(golden_small, monkeypatch):
    """A decoder on the emulated backend whose every kernel call is recorded with its arguments and does nothing (`calls`); `arm()` makes any
    further call fail."""
    from tests.emu.backend import emulated_backend
    from videollama2_amd import _lib
    from videollama2_amd.decoder import HipMistralDecoder
    cfg = golden_small["cfg"]
    sd = O.seeded_state_dict(cfg, golden_small["seed"], only=_keep)
    with emulated_backend():
        dec = HipMistralDecoder(cfg, sd, "cpu", max_seq_len=256)
        calls, state = [], dict(armed=False)

        def call(name, *a):
            assert not state["armed"], f"a kernel was called: {name}"
            calls.append((name, a))
        monkeypatch.setattr(_lib, "call", call)
        yield dec, calls, lambda on=True: state.update(armed=on)
        dec._bb_busy = None


def _x(n, dec):
    return torch.zeros(n, dec.D, dtype=torch.bfloat16)


def test_refusals_come_with_their_reasons_before_any_kernel(stubbed):
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.serving import ContinuousBatcher, ModelBatcher
    dec, calls, arm = stubbed
    arm()
    with pytest.raises(RuntimeError, match="reserve=\"grow\" grows reservations in the page pool: call decoder.enable_paged_kv\\(n_pages\\) first"):
        ContinuousBatcher(dec, max_slots=2, use_graph=False, reserve="grow")
    assert getattr(dec, "_bb", None) is None                         # refused before the slot buffers exist
    for bad in ("grown", None, True, "WHOLE"):
        with pytest.raises(ValueError, match="reserve must be \"whole\" or \"grow\""):
            ContinuousBatcher(dec, max_slots=2, use_graph=False, reserve=bad)
    m = VideoLLaMA2Hip.__new__(VideoLLaMA2Hip)
    torch.nn.Module.__init__(m)
    m.decoder = dec
    with pytest.raises(RuntimeError, match="reserve=\"grow\" grows reservations in the page pool"):
        m.batcher(max_slots=2, use_graph=False, reserve="grow")
    with pytest.raises(ValueError, match="reserve must be"):
        ModelBatcher(m, 2, None, False, "paged")
    for fp8 in (False, True):
        dec.enable_paged_kv(8, fp8=fp8)
        assert ContinuousBatcher(dec, max_slots=2, use_graph=False).reserve == "whole"           # the default
        mb = m.batcher(max_slots=2, use_graph=False, reserve="grow")
        b = mb.inner
        assert b.reserve == "grow" and b.preemptions == b.resumes == 0 and len(b.swapped) == 0
        # a resident prefix and growth refuse each other, either way round
        with pytest.raises(NotImplementedError, match="open_prefix: this batcher grows its reservations page by page \\(reserve=\"grow\"\\)"):
            b.open_prefix(_x(130, dec))
        with pytest.raises(NotImplementedError, match="open_prefix: this batcher grows its reservations"):
            mb.open_video(torch.arange(3, 80), None)
        assert dec._bb["pool"].n_free == 7 and b._prefix is None
        # the worst case still has to fit the pool, and is still what `need` records
        dec.enable_paged_kv(4, fp8=fp8)
        b = m.batcher(2, None, False, "grow").inner
        with pytest.raises(ValueError, match="needs 4 pages \\(200 prompt rows \\+ 57 new tokens\\), the pool serves 3"):
            b.submit(_x(200, dec), max_new_tokens=500)
        assert b.in_flight() == 0
        b.submit(_x(100, dec), max_new_tokens=29)
        assert b.waiting[0].need == 3 and b.waiting[0].S == 100 and b.in_flight() == 1
        b.waiting.clear()
    dec.enable_paged_kv(8)
    whole = ContinuousBatcher(dec, max_slots=2, use_graph=False)
    h = object()
    grow = ContinuousBatcher(dec, max_slots=2, use_graph=False, reserve="grow")
    with pytest.raises(NotImplementedError, match="submit: this batcher grows its reservations page by page"):
        grow.submit(_x(3, dec), max_new_tokens=2, prefix=h)
    assert whole.in_flight() == grow.in_flight() == 0
    assert calls == []


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_the_batcher_follows_the_simulated_schedule_and_swaps_through_the_arena(stubbed, fp8):
    """The preemption case of the GPU tests on recording stubs: steps, victims, pages per step and resumes are the simulation's; a swap is
    one vl2_kv_pages_move per pool per layer each way, through one arena per pool kind, on the victim's page ids; growth is a table-row
    copy and nothing else."""
    from tests.test_gpu_paged_grow import PREEMPT
    from videollama2_amd.serving import ContinuousBatcher
    dec, calls, arm = stubbed
    reqs, n_pages, max_slots = PREEMPT["requests"], PREEMPT["n_pages"], PREEMPT["max_slots"]
    plan = simulate(reqs, n_pages, max_slots, 256)
    dec.enable_paged_kv(n_pages, fp8=fp8)
    b = ContinuousBatcher(dec, max_slots=max_slots, use_graph=False, reserve="grow")
    rid = [b.submit(_x(S, dec), max_new_tokens=budget) for S, budget, _ in reqs]
    bb = dec._bb
    pools_per_layer = 4 if fp8 else 2
    held, victims, moves, pages_before = [], [], [], {}
    while b.in_flight():
        flying = {r.rid: r for r in b.slots if r is not None}
        pages_before.update({r.rid: list(r.pages) for r in flying.values()})
        del calls[:]
        table_before = bb["table"].clone()
        b.step()
        mv = [a for n, a in calls if n == NAME]
        out = [r for r in flying.values() if r.swap is not None]
        back = b.resumes - sum(1 for m in moves if m == "in")
        assert len(mv) == (len(out) + back) * dec.n_layers * pools_per_layer
        for v in out:
            victims.append(v.rid)
            moves.append("out")
            saved, logits = v.swap
            n = len(pages_before[v.rid])
            assert v.pages is None and len(saved) == dec.n_layers * pools_per_layer and v.slot is None
            assert all(t.shape[0] == n for t in saved) and logits.shape == bb["logits"][0].shape
            assert sum(t.numel() * t.element_size() for t in saved) == n * dec.kv_page_bytes()
        moves.extend(["in"] * back)
        if mv:
            arenas = {a[1] for a in mv}
            assert len(arenas) == (2 if fp8 else 1) and arenas == {t.data_ptr() for t in b._arena.values()}
            assert all(t.shape[0] == bb["pages_per_seq"] for t in b._arena.values())
            assert {a[4] for a in mv} == {n_pages} and {a[6] for a in mv} == ({1} if out else {0})
            pool_ptrs = [t.data_ptr() for li in range(dec.n_layers) for t in b._pools_of(li)]
            assert [a[0] for a in mv] == pool_ptrs * (len(out) + back)
        live = {r.rid: r for r in b.slots if r is not None}
        # the table: a live request's row names its pages, every other row is parked
        for s in range(max_slots):
            r = b.slots[s]
            assert bb["table"][s].tolist() == (r.pages + [-1] * (4 - len(r.pages)) if r is not None else [0, -1, -1, -1]), s
        assert bb["pool"].n_free + sum(len(r.pages) for r in live.values()) == n_pages - 1
    assert b.steps == plan["steps"] and victims == plan["victims"] and b.preemptions == plan["preemptions"] == b.resumes
    assert moves.count("out") == moves.count("in") == b.preemptions >= 1
    assert sorted(b.finished) == rid and [len(b.finished[r]) for r in rid] == [n for _, _, n in reqs]
    assert bb["pool"].n_free == n_pages - 1 and bb["table"].tolist() == [[0, -1, -1, -1]] * max_slots and len(b.swapped) == 0
    # the default policy on the same pool never issues the move
    del calls[:]
    w = ContinuousBatcher(dec, max_slots=max_slots, use_graph=False)
    for S, budget, _ in reqs:
        w.submit(_x(S, dec), max_new_tokens=budget)
    w.run()
    assert NAME not in [n for n, _ in calls] and w.steps > b.steps
