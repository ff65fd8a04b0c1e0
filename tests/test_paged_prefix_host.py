"""A shared prefix held once in the page pool, host side only (no launch): the page arithmetic against brute force, FIFO admission on the own
reservations, the declarations of the two entry points against the ctypes table, the argument refusals of the library and of the Python
wrappers (before anything is enqueued), and -- on the emulated backend with every kernel call stubbed -- the batcher's refusals with their
reasons, its pool accounting, the table rows after open, admit, retire and close, and the values a live hole is parked at."""
import ctypes
import os
import re

import pytest
import torch

from oracle import vl2_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
NAMES = ("vl2_attn_decode_shared_paged", "vl2_kv_page_gather")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- page arithmetic
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 127, 128, 149, 1621])
def test_shared_rows_and_own_pages_against_a_brute_force_count(P):
    from videollama2_amd.paging import own_pages_needed, pages_needed, shared_rows
    Pf = shared_rows(P)
    assert Pf == max(r for r in range(0, P + 1, 64)) and Pf % 64 == 0 and 0 <= P - Pf < 64
    for n in (1, 5, 63, 64, 65):
        for max_new in (1, 64, 130):
            for max_seq_len in (4096, P + n + max_new, P + n + max_new - 1, P + n + 1, P + n):
                # the rows the request can ever hold, cut at the cache end; the pages they fall in that are not whole pages of the prefix
                rows = [p for p in range(P + n + max_new) if p < max_seq_len]
                own = {p // 64 for p in rows} - set(range(Pf // 64))
                got = own_pages_needed(P, n, max_new, max_seq_len)
                assert got == len(own), (P, n, max_new, max_seq_len)
                assert got + Pf // 64 == pages_needed(P + n, max_new, max_seq_len)
                assert got >= 1                                        # the row after the shared rows is never in a shared page


def test_prefix_parked_row():
    from videollama2_amd.paging import prefix_parked_row
    for pre in ([], [4], [7, 2, 9]):
        for pps in range(len(pre) + 1, len(pre) + 4):
            row = prefix_parked_row(pre, pps)
            assert len(row) == pps and row[:len(pre)] == pre and row[len(pre)] == 0 and all(x == -1 for x in row[len(pre) + 1:])
    with pytest.raises(ValueError, match="do not fit"):
        prefix_parked_row([1, 2], 2)


def test_fifo_admission_on_own_reservations_with_a_blocking_head():
    """1621-row prefix (25 shared pages), questions of 8 rows and 128 new tokens: 3 own pages each; a long one needs 5.  A pool that holds the
    prefix and 7 more pages."""
    from videollama2_amd.paging import PagePool, admit_fifo, own_pages_needed
    P = 1621
    small, big = own_pages_needed(P, 8, 128, 4096), own_pages_needed(P, 8, 256, 4096)
    assert (small, big) == (3, 5) and 25 + 64 * small == 217
    pool = PagePool(1 + 25 + 7)
    pre = pool.alloc(25)
    assert pre == list(range(1, 26))
    assert admit_fifo([small, big, small], 4, pool.n_free) == 1            # 3, then 5 > 4 left: the head of the rest blocks, the small one waits
    a = pool.alloc(small)
    assert admit_fifo([big, small], 3, pool.n_free) == 0
    pool.free(a)
    assert admit_fifo([big, small], 3, pool.n_free) == 1
    b = pool.alloc(big)
    assert admit_fifo([small], 2, pool.n_free) == 0 and not set(b) & set(pre)
    pool.free(b); pool.free(pre)
    assert pool.n_free == 32


# ---------------------------------------------------------------------------------------------------------------- declarations
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


def test_header_declarations_match_the_ctypes_table(lib):
    from videollama2_amd import _lib
    assert set(_lib.PAGED_PREFIX_SIGNATURES) == set(NAMES)
    for name in NAMES:
        ret, args = _declared(name)
        assert ret is ctypes.c_int32 and args == _lib.PAGED_PREFIX_SIGNATURES[name], name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int32
        assert name in _lib.EXPORTS and name not in _lib.SIGNATURES            # the emulator's symbol set is unchanged
        assert name not in _lib.PAGED_KV_SIGNATURES and name not in _lib.SHARED_PREFIX_SIGNATURES
        for path in (_lib.LIB_PATH, _lib.LIB_PATHS["fp16"], _lib.LAB_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert lib.vl2_version() == 7


def test_library_refuses_bad_arguments_before_launching(lib):
    p = ctypes.c_void_p(4096)                                       # stand-in device pointers: every case fails its checks first
    odd = ctypes.c_void_p(4100)
    per = lib.vl2_attn_decode_shared_partial_floats(128, 128, 8)
    assert per == 8 * (1 + 2) * 130

    def attn(qkv=p, kpool=p, vpool=p, table=p, pre=p, cos=p, sin=p, partial=p, out=p, pos_dev=p, B=3, qkv_bs=1536, table_bs=4, n_pages=9, nh=8,
             nkv=2, P=128, own_cap=128, rope_rows=256, partial_floats=3 * per, out_bs=1024):
        return lib.vl2_attn_decode_shared_paged(qkv, kpool, vpool, table, pre, cos, sin, partial, partial_floats, out, B, qkv_bs, table_bs, n_pages,
                                                out_bs, nh, nkv, P, own_cap, rope_rows, pos_dev, 0.088, None)

    cases = [(k, -1, "null pointer") for k in (dict(qkv=None), dict(kpool=None), dict(vpool=None), dict(table=None), dict(pre=None), dict(cos=None),
                                               dict(sin=None), dict(partial=None), dict(out=None), dict(pos_dev=None))]
    cases += [(dict(B=0), -1, "B > 0"), (dict(nh=7), -2, "nh = nkv*group"), (dict(n_pages=0), -2, "n_pages 0"), (dict(n_pages=-3), -2, "n_pages -3"),
              (dict(P=0), -2, "P 0 must be a positive multiple of 64"), (dict(P=-64), -2, "P -64 must be"), (dict(P=100), -2, "P 100 must be"),
              (dict(own_cap=0), -2, "own_cap 0 must be"), (dict(own_cap=100), -2, "own_cap 100 must be"),
              (dict(own_cap=192, rope_rows=512, partial_floats=10 ** 6), -2, "2 prefix pages + 3 own pages outside a table row of 4 pages"),
              (dict(table_bs=3), -2, "outside a table row of 3 pages"), (dict(rope_rows=255), -2, "positions up to 255 outside the cos/sin tables (255"),
              (dict(partial_floats=3 * per - 1), -2, f"partial of {3 * per - 1} floats, need {3 * per}"),
              (dict(B=40000, partial_floats=10 ** 12), -2, "too many requests (40000)"),
              (dict(kpool=odd), -2, "16-byte alignment"), (dict(vpool=odd), -2, "16-byte alignment"), (dict(qkv=odd), -2, "16-byte alignment"),
              (dict(qkv_bs=1537), -2, "16-byte alignment"), (dict(qkv_bs=1024), -2, "rows must hold"), (dict(out_bs=1000), -2, "rows must hold")]
    for kw, rc, msg in cases:
        assert attn(**kw) == rc, (kw, lib.vl2_last_error_string().decode())
        err = lib.vl2_last_error_string().decode()
        assert msg in err and "vl2_attn_decode_shared_paged" in err, (kw, err)

    def gath(kpool=p, vpool=p, k16=p, v16=p, row=p, nkv=2, smax=256, n_pages=9, p0=0, p1=10):
        return lib.vl2_kv_page_gather(kpool, vpool, k16, v16, row, nkv, smax, n_pages, p0, p1, None)

    cases = [(k, -1, "null pointer") for k in (dict(k16=None), dict(v16=None), dict(kpool=None), dict(vpool=None), dict(row=None))]
    cases += [(dict(nkv=0), -1, "nkv, smax > 0"), (dict(n_pages=0), -2, "n_pages 0"), (dict(p0=11, p1=10), -2, "rows [11, 10) outside"),
              (dict(p1=257), -2, "rows [0, 257) outside"), (dict(p0=-1), -2, "rows [-1, 10) outside"), (dict(k16=odd), -2, "16-byte aligned"),
              (dict(v16=odd), -2, "16-byte aligned"), (dict(kpool=odd), -2, "16-byte aligned"), (dict(vpool=odd), -2, "16-byte aligned")]
    for kw, rc, msg in cases:
        assert gath(**kw) == rc, (kw, lib.vl2_last_error_string().decode())
        err = lib.vl2_last_error_string().decode()
        assert msg in err and "vl2_kv_page_gather" in err, (kw, err)
    assert gath(p0=10, p1=10) == 0                                  # an empty range is no error and no launch


def test_wrappers_refuse_before_the_library_is_touched(monkeypatch):
    from videollama2_amd import _lib, ops

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    bf, i32 = torch.bfloat16, torch.int32
    nh, nkv, B, pps = 8, 2, 2, 4
    pool = lambda n=5: torch.zeros(n, nkv, 64, 128, dtype=bf)
    per = ops.shared_partial_floats(128, 128, nh)
    good = dict(qkv=torch.zeros(B, 12 * 128, dtype=bf), kpool=pool(), vpool=pool(), table=torch.zeros(B, pps, dtype=i32),
                prefix_pages=torch.zeros(2, dtype=i32), cos_t=torch.zeros(256, 64), sin_t=torch.zeros(256, 64), partial=torch.zeros(B * per),
                out=torch.zeros(B, nh * 128, dtype=bf), nh=nh, nkv=nkv, P=128, own_cap=128, pos_dev=torch.zeros(B, dtype=i32), scale=0.088)
    cases = [(dict(nh=7), ValueError, "nh = nkv \\* group"), (dict(qkv=good["qkv"][:, :-128]), ValueError, "qkv must be"),
             (dict(qkv=good["qkv"].half()), TypeError, "qkv must be torch.bfloat16"), (dict(kpool=pool().half()), TypeError, "kpool must be"),
             (dict(table=good["table"].long()), TypeError, "table must be torch.int32"),
             (dict(prefix_pages=good["prefix_pages"].long()), TypeError, "prefix_pages must be torch.int32"),
             (dict(pos_dev=good["pos_dev"].long()), TypeError, "pos_dev must be torch.int32"),
             (dict(kpool=torch.zeros(5, nkv, 32, 128, dtype=bf)), ValueError, "pools must be \\[n_pages, nkv, 64, 128\\]"),
             (dict(vpool=pool(6)), ValueError, "pools must be"),
             (dict(kpool=pool(10)[::2], vpool=pool(10)[::2]), ValueError, "pages must be contiguous"),
             (dict(P=0), ValueError, "P 0 must be a positive multiple of 64"), (dict(P=100), ValueError, "P 100 must be"),
             (dict(own_cap=0), ValueError, "own_cap 0 must be"), (dict(own_cap=65), ValueError, "own_cap 65 must be"),
             (dict(table=good["table"][0]), ValueError, "page table must be int32"), (dict(table=good["table"][:1]), ValueError, "page table must be int32"),
             (dict(table=good["table"][:, :3]), ValueError, "2 prefix \\+ 2 own pages"),
             (dict(table=torch.zeros(B, 8, dtype=i32)[:, ::2]), ValueError, "page table must be int32"),
             (dict(prefix_pages=good["prefix_pages"][:1]), ValueError, "at least 2 entries"),
             (dict(prefix_pages=torch.zeros(4, dtype=i32)[::2]), ValueError, "prefix_pages must be a contiguous"),
             (dict(prefix_pages=torch.zeros(1, 2, dtype=i32)), ValueError, "prefix_pages must be a contiguous"),
             (dict(cos_t=torch.zeros(255, 64), sin_t=torch.zeros(255, 64)), ValueError, "cos / sin tables"),
             (dict(pos_dev=good["pos_dev"][:1]), ValueError, "positions"), (dict(out=good["out"][:, :-1]), ValueError, "out \\[B, nh \\* 128\\]"),
             (dict(partial=good["partial"][:-1]), ValueError, "partial holds"), ({}, ValueError, "must be a device tensor")]
    for kw, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            ops.attn_decode_shared_paged(**{**good, **kw})
    cache = lambda: torch.zeros(nkv, 256, 128, dtype=bf)
    good = dict(kpool=pool(), vpool=pool(), kcache=cache(), vcache=cache(), table_row=torch.zeros(pps, dtype=i32), p0=0, p1=10)
    cases = [(dict(kcache=cache().half()), TypeError, "kcache must be"), (dict(table_row=good["table_row"].long()), TypeError, "table_row must be torch.int32"),
             (dict(vpool=pool().float()), TypeError, "vpool must be"), (dict(kpool=pool()[:, :, :32]), ValueError, "pools must be"),
             (dict(kcache=cache()[:1], vcache=cache()[:1]), ValueError, "contiguous 16-bit caches"),
             (dict(kcache=torch.zeros(nkv, 512, 128, dtype=bf)[:, ::2]), ValueError, "contiguous 16-bit caches"),
             (dict(table_row=good["table_row"][:3]), ValueError, "at least 4 entries"), (dict(table_row=torch.zeros(1, pps, dtype=i32)), ValueError, "table row must be"),
             (dict(p0=11), ValueError, "rows \\[11, 10\\) outside"), (dict(p1=257), ValueError, "rows \\[0, 257\\) outside"),
             (dict(p0=-1), ValueError, "rows \\[-1, 10\\) outside"), ({}, ValueError, "must be a device tensor")]
    for kw, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            ops.kv_page_gather(**{**good, **kw})


# ---------------------------------------------------------------------------------------------------------------- the batcher
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


@pytest.fixture()
def stubbed(golden_small, monkeypatch):
    """A decoder on the emulated backend whose every kernel call is recorded and does nothing (`calls`); `arm()` makes any further call fail."""
    from tests.emu.backend import emulated_backend
    from videollama2_amd import _lib, ops
    from videollama2_amd.decoder import HipMistralDecoder
    cfg = golden_small["cfg"]
    sd = O.seeded_state_dict(cfg, golden_small["seed"], only=_keep)
    with emulated_backend():
        dec = HipMistralDecoder(cfg, sd, "cpu", max_seq_len=256)
        calls, state = [], dict(armed=False)

        def call(name, *a):
            assert not state["armed"], f"a kernel was called: {name}"
            calls.append(name)
        monkeypatch.setattr(_lib, "call", call)
        # (this wrapper asks the library for its workspace size first, which the emulator does not export)
        monkeypatch.setattr(ops, "attn_append", lambda *a, **k: call("vl2_attn_append"))
        yield dec, calls, lambda on=True: state.update(armed=on)
        dec._bb_busy = None


def _x(n, dec):
    return torch.zeros(n, dec.D, dtype=torch.bfloat16)


def test_open_submit_and_close_refusals_come_with_their_reasons_before_any_kernel(stubbed):
    from videollama2_amd.decoder import HipMixtralDecoder
    from videollama2_amd.serving import ContinuousBatcher, PrefixHandle
    dec, calls, arm = stubbed
    arm()
    b = ContinuousBatcher(dec, max_slots=2, use_graph=False)
    with pytest.raises(RuntimeError, match="open_prefix: the resident prefix lives in the page pool.*enable_paged_kv"):
        b.open_prefix(_x(130, dec))
    with pytest.raises(RuntimeError, match="close_prefix: no prefix is open"):
        b.close_prefix()
    with pytest.raises(ValueError, match="closed or was opened on another batcher"):
        b.submit(_x(3, dec), prefix=PrefixHandle(130, [1, 2], _x(2, dec)))
    with pytest.raises(ValueError, match="prefix must be the handle open_prefix returned, got int"):
        b.submit(_x(3, dec), prefix=7)
    dec.enable_paged_kv(6)
    b = ContinuousBatcher(dec, max_slots=2, use_graph=False)
    # everything the shared-prefix mode refuses, paging itself excepted
    dec.tp_always_reduce = True
    with pytest.raises(NotImplementedError, match="shared-prefix decode: single-rank decoders only"):
        b.open_prefix(_x(130, dec))
    dec.tp_always_reduce = False
    dec.hd = 64
    with pytest.raises(NotImplementedError, match="shared-prefix decode: head_dim 128 only \\(this decoder has 64\\)"):
        b.open_prefix(_x(130, dec))
    dec.hd = 128
    dec.prefill_fp8 = True
    with pytest.raises(NotImplementedError, match="shared-prefix decode: .*enable_fp8_prefill\\(False\\)"):
        b.open_prefix(_x(130, dec))
    dec.prefill_fp8 = False
    mix = object.__new__(HipMixtralDecoder)
    with pytest.raises(NotImplementedError, match="(?i)mixtral"):
        mix._shared_prefix_refusals(paged_ok=True)
    # the prefix itself
    with pytest.raises(ValueError, match="a prefix of 63 rows has no whole page of 64 rows to share"):
        b.open_prefix(_x(63, dec))
    with pytest.raises(ValueError, match="a prefix of 256 rows leaves no room for a suffix row in the KV cache \\(256\\)"):
        b.open_prefix(_x(256, dec))
    dec.enable_paged_kv(3)
    b = ContinuousBatcher(dec, max_slots=2, use_graph=False)
    with pytest.raises(ValueError, match="the prefix needs 2 pages and one request at least 1 more, the pool has 2 free \\(of 2"):
        b.open_prefix(_x(130, dec))
    assert dec._bb["pool"].n_free == 2 and dec._bb["table"].tolist() == [[0, -1, -1, -1]] * 2
    # requests waiting
    rid = b.submit(_x(10, dec), max_new_tokens=4)
    with pytest.raises(RuntimeError, match="open_prefix: 1 requests are waiting or in flight"):
        b.open_prefix(_x(64, dec))
    assert b.waiting[0].rid == rid
    b.waiting.clear()
    # the switches that stay refused under paging
    with pytest.raises(NotImplementedError, match="shared-prefix decode: the paged KV cache is on"):
        dec.generate_batch([_x(3, dec)], max_new_tokens=2, shared_prefix=_x(64, dec))
    with pytest.raises(NotImplementedError, match="fp8 KV cache: the paged KV cache is on"):
        dec.enable_fp8_kv()
    assert calls == []


def test_pool_accounting_table_rows_and_hole_parking(stubbed, monkeypatch):
    from videollama2_amd import ops
    from videollama2_amd.serving import ContinuousBatcher
    dec, calls, arm = stubbed
    dec.enable_paged_kv(8)                                           # 7 pages serve; pages_per_seq 4
    b = ContinuousBatcher(dec, max_slots=3, use_graph=False)
    bb = dec._bb
    pool = bb["pool"]
    # with no prefix open, submit is today's
    r = b.submit(_x(100, dec), max_new_tokens=29)
    assert b.waiting[0].need == 3 and b.waiting[0].x.shape[0] == 100 and b.waiting[0].rid == r
    b.waiting.clear()
    assert calls == []
    # open: the shared rows are prefilled once and scattered into 2 pages; every slot is parked behind them
    epoch = dec.cache_epoch
    h = b.open_prefix(_x(149, dec))
    assert (h.P, h.shared_rows, h.pages, h.tail.shape[0], h.own_cap, h.open) == (149, 128, [1, 2], 21, 128, True)
    assert h.prefix_pages.tolist() == [1, 2] and h.prefix_pages.dtype == torch.int32
    assert h.partial.numel() == 3 * ops.shared_partial_floats(128, 128, dec.nh)
    assert calls.count("vl2_kv_page_scatter") == dec.n_layers and "vl2_kv_page_gather" not in calls
    assert dec.pos == 128 and h.epoch == dec.cache_epoch == epoch + 1
    assert pool.n_free == 5 and bb["table"].tolist() == [[1, 2, 0, -1]] * 3
    arm()
    with pytest.raises(RuntimeError, match="open_prefix: a prefix is open already"):
        b.open_prefix(_x(64, dec))
    with pytest.raises(ValueError, match="a prefix is open on this batcher: pass prefix=handle"):
        b.submit(_x(5, dec), max_new_tokens=3)
    with pytest.raises(ValueError, match="at least one row of its own"):
        b.submit(_x(0, dec), max_new_tokens=3, prefix=h)
    with pytest.raises(ValueError, match="sequence length 257 exceeds the KV cache \\(256\\)"):
        b.submit(_x(108, dec), max_new_tokens=3, prefix=h)
    other = ContinuousBatcher.__new__(ContinuousBatcher)
    other.dec, other._prefix = dec, None
    with pytest.raises(ValueError, match="closed or was opened on another batcher"):
        ContinuousBatcher.submit(other, _x(5, dec), max_new_tokens=3, prefix=h)
    assert b.in_flight() == 0
    arm(False)
    # the reservations are the own pages; the rows a request's extend computes are tail ++ suffix
    rid = [b.submit(_x(n, dec), max_new_tokens=m, prefix=h) for n, m in ((5, 2), (30, 40), (9, 3), (50, 60))]
    assert [r.need for r in b.waiting] == [1, 2, 1, 2] and [r.x.shape[0] for r in b.waiting] == [26, 51, 30, 71]
    assert [r.max_new for r in b.waiting] == [2, 40, 3, 58]                         # the cache end cuts the last one: 256 - 199 + 1
    seen = []
    monkeypatch.setattr(ops, "attn_decode_shared_paged",
                        lambda qkv, kp, vp, table, pre, cos, sin, partial, out, nh, nkv, P, own_cap, pos, scale:
                        seen.append((table.tolist(), pre.tolist(), partial is h.partial, P, own_cap, pos.tolist())))
    del calls[:]
    b.step()
    # three slots: requests 0, 1, 2 (1 + 2 + 1 pages); request 3 waits for a slot
    assert [None if r is None else r.rid for r in b.slots] == rid[:3] and len(b.waiting) == 1
    assert bb["table"].tolist() == [[1, 2, 3, -1], [1, 2, 4, 5], [1, 2, 6, -1]] and pool.n_free == 1
    assert calls.count("vl2_kv_page_scatter") == 3 * dec.n_layers and "vl2_kv_page_gather" not in calls
    assert len(seen) == dec.n_layers and seen[0] == ([[1, 2, 3, -1], [1, 2, 4, 5], [1, 2, 6, -1]], [1, 2], True, 128, 128, [154, 179, 158])
    assert dec.pos == 128 and h.epoch == dec.cache_epoch
    assert bb["pos"][:3].tolist() == [155, 180, 159]
    b.step()                                                         # request 0 retires (2 tokens): its page goes back, its row is re-parked
    assert b.slots[0] is None and pool.n_free == 2 and bb["table"][0].tolist() == [1, 2, 0, -1]
    del seen[:]
    b.step()                                                         # request 3 (2 pages) joins slot 0 on the freed page and the spare one
    assert b.slots[0].rid == rid[3] and b.slots[0].pages == [3, 7] and bb["table"][0].tolist() == [1, 2, 3, 7]
    assert b.slots[2] is None and bb["table"][2].tolist() == [1, 2, 0, -1] and pool.n_free == 7 - 2 - 2 - 2   # request 2 retired (3 tokens)
    # a foreign use of the single-sequence cache: the next admission restores rows [0, 128) from the pages first
    dec.prefill(_x(40, dec))
    assert dec.pos == 40 and dec.cache_epoch != h.epoch
    del calls[:], seen[:]
    b.slots[0].max_new = len(b.slots[0].tokens) + 1                  # let request 3 retire in the coming step: slot 0 becomes the hole
    b.step()
    assert b.slots[0] is None and b.slots[1] is not None
    r4 = b.submit(_x(1, dec), max_new_tokens=2, prefix=h)
    del calls[:], seen[:]
    b.step()                                                         # request 4 takes slot 0 (the lowest free): gather, extend, scatter
    gathers = [i for i, c in enumerate(calls) if c == "vl2_kv_page_gather"]
    scatters = [i for i, c in enumerate(calls) if c == "vl2_kv_page_scatter"]
    assert len(gathers) == dec.n_layers and len(scatters) == dec.n_layers and max(gathers) < min(scatters)
    assert b.slots[0].rid == r4 and dec.pos == 128 and h.epoch == dec.cache_epoch
    # a live hole: request 4 leaves slot 0 while request 1 goes on in slot 1 -- slot 0 is parked at the shared rows on the parking page, greedy
    b.step()
    assert b.slots[0] is None and b.slots[1] is not None
    bb["samp_T"][0] = 0.7
    del seen[:]
    b.step()
    table, _, _, P, own_cap, pos = seen[0]
    assert table[0] == [1, 2, 0, -1] and pos[0] == 128 and float(bb["samp_T"][0]) == 0.0 and (P, own_cap) == (128, 128)
    assert pos[1] == bb["pos"][1] - 1 and len(pos) == 2
    # close: refused with requests in flight; afterwards every page is back and every row is the plain parked row
    with pytest.raises(RuntimeError, match="close_prefix: 1 requests are waiting or in flight"):
        b.close_prefix()
    b.slots[1].max_new = len(b.slots[1].tokens) + 1
    b.step()
    assert b.in_flight() == 0 and pool.n_free == 5
    b.close_prefix()
    assert pool.n_free == 7 and bb["table"].tolist() == [[0, -1, -1, -1]] * 3 and not h.open and b._prefix is None
    with pytest.raises(ValueError, match="closed or was opened on another batcher"):
        b.submit(_x(5, dec), max_new_tokens=3, prefix=h)
    r = b.submit(_x(100, dec), max_new_tokens=29)                    # and a plain submit is today's again
    assert b.waiting[0].need == 3 and b.waiting[0].rid == r
    b.waiting.clear()


def test_model_batcher_refusals_before_the_encoder(stubbed):
    from videollama2_amd.constants import MODAL_INDEX_MAP
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.serving import ModelBatcher
    dec, calls, arm = stubbed
    arm()
    m = VideoLLaMA2Hip.__new__(VideoLLaMA2Hip)
    torch.nn.Module.__init__(m)
    m.decoder = dec

    def encoder(*a, **k):
        raise AssertionError("the encoder ran")
    m.encode_images_or_videos = encoder
    mb = ModelBatcher(m, max_slots=2, use_graph=False)
    ids = torch.arange(3, 80)
    with pytest.raises(RuntimeError, match="open_prefix: the resident prefix lives in the page pool"):
        mb.open_video(ids, None)
    dec.enable_paged_kv(6)
    mb = ModelBatcher(m, max_slots=2, use_graph=False)
    dec.tp_always_reduce = True
    with pytest.raises(NotImplementedError, match="shared-prefix decode: single-rank decoders only"):
        mb.open_video(ids, None)
    dec.tp_always_reduce = False
    sentinel = next(iter(MODAL_INDEX_MAP.values()))
    with pytest.raises(ValueError, match="open_video: the prefix holds 1 modal sentinels for 0 media"):
        mb.open_video(torch.cat([ids, torch.tensor([sentinel])]), None)
    with pytest.raises(ValueError, match="prefix must be the handle open_video returned"):
        mb.submit(ids, prefix=7)
    with pytest.raises(RuntimeError, match="close_prefix: no prefix is open"):
        mb.close_video()
    assert calls == []
