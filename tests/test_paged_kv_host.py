"""The paged KV cache, host side only (no launch): the page allocator, a request's reservation against a brute-force count, the batcher's
FIFO admission rule, the declarations of the two entry points against the ctypes table, the argument refusals of the library and of the
Python wrappers (before anything is enqueued), and the decoder's, the model's and the batcher's refusals with their reasons."""
import collections
import ctypes
import os
import re

import pytest
import torch

from oracle import vl2_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
NAMES = ("vl2_attn_decode_paged", "vl2_kv_page_scatter")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the allocator
def test_page_pool_order_exhaustion_and_reuse():
    from videollama2_amd.paging import PagePool
    pool = PagePool(8)
    assert pool.n_free == 7
    a = pool.alloc(3)
    assert a == [1, 2, 3] and pool.n_free == 4                     # lowest first, page 0 never
    b = pool.alloc(2)
    assert b == [4, 5] and pool.n_free == 2
    with pytest.raises(RuntimeError, match="3 pages needed, 2 free"):
        pool.alloc(3)
    assert pool.n_free == 2 and pool.alloc(0) == []                # exhaustion took nothing
    pool.free([2, 1])
    assert pool.n_free == 4 and pool.alloc(3) == [1, 2, 6]         # freed ids are reused, lowest first
    rest = pool.alloc(pool.n_free)
    assert rest == [7] and pool.n_free == 0
    assert 0 not in a + b + rest
    # every page handed out exactly once
    pool.free([1, 2, 6]); pool.free(rest); pool.free([3]); pool.free(b)
    assert pool.n_free == 7 and pool.alloc(7) == list(range(1, 8))


def test_page_pool_refuses_bad_frees_and_takes_none_of_them():
    from videollama2_amd.paging import PagePool
    pool = PagePool(6)
    got = pool.alloc(3)                                             # 1, 2, 3
    for ids, msg in (([0], "parking page"), ([1, 0], "parking page"), ([4], "free already"), ([1, 5], "free already"), ([6], "not of this pool"),
                     ([-1], "not of this pool"), ([2, 2], "named twice")):
        with pytest.raises(ValueError, match=msg):
            pool.free(ids)
        assert pool.n_free == 2, ids                                # a refused call frees nothing, not even its valid ids
    pool.free(got)
    with pytest.raises(ValueError, match="double free"):
        pool.free([1])
    assert pool.n_free == 5
    with pytest.raises(ValueError, match="at least the parking page"):
        PagePool(0)
    assert PagePool(1).n_free == 0


@pytest.mark.parametrize("S", [1, 63, 64, 65])
@pytest.mark.parametrize("max_new", [1, 64])
def test_pages_needed_against_a_brute_force_count(S, max_new):
    from videollama2_amd.paging import pages_needed
    for max_seq_len in (4096, 128, 100, 64, S + max_new, S + max_new - 1, max(S, 2)):
        # the rows the request can ever hold: its prompt and one per token it may feed, cut at the cache end; the pages those rows fall in
        rows = [p for p in range(S + max_new) if p < max_seq_len]
        assert pages_needed(S, max_new, max_seq_len) == len({p // 64 for p in rows}), (S, max_new, max_seq_len)


def test_table_rows():
    from videollama2_amd.paging import parked_row, table_row
    assert table_row([5, 2], 4) == [5, 2, -1, -1] and parked_row(3) == [0, -1, -1] and table_row([], 2) == [-1, -1]
    with pytest.raises(ValueError, match="do not fit"):
        table_row([1, 2, 3], 2)


# ---------------------------------------------------------------------------------------------------------------- admission
def test_admission_is_strict_fifo_on_whole_reservations():
    from videollama2_amd.paging import PagePool, admit_fifo
    assert admit_fifo([], 4, 10) == 0
    assert admit_fifo([2, 2, 2], 4, 10) == 3
    assert admit_fifo([2, 2, 2], 2, 10) == 2                        # slots run out
    assert admit_fifo([2, 2, 2], 4, 5) == 2                         # pages run out
    assert admit_fifo([2, 2, 2], 0, 10) == 0
    # a head that does not fit blocks the queue: the small requests behind it are NOT admitted ...
    assert admit_fifo([5, 1, 1], 3, 4) == 0
    assert admit_fifo([3, 5, 1], 3, 7) == 1
    # ... and a later retire admits it: a little simulation on a real pool
    pool, queue, slots = PagePool(8), collections.deque([(0, 4), (1, 5), (2, 1)]), {}
    order = []

    def step():
        k = admit_fifo([need for _, need in queue], 2 - len(slots), pool.n_free)
        for _ in range(k):
            rid, need = queue.popleft()
            slots[rid] = pool.alloc(need)
            order.append(rid)
    step()
    assert order == [0] and pool.n_free == 3                        # request 1 (5 pages) does not fit; request 2 (1 page) waits behind it
    step()
    assert order == [0]
    pool.free(slots.pop(0))
    step()
    assert order == [0, 1, 2] and pool.n_free == 1 and slots[1] == [1, 2, 3, 4, 5] and slots[2] == [6]


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
    assert set(_lib.PAGED_KV_SIGNATURES) == set(NAMES)
    for name in NAMES:
        ret, args = _declared(name)
        assert ret is ctypes.c_int32 and args == _lib.PAGED_KV_SIGNATURES[name], name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int32
        assert name in _lib.EXPORTS and name not in _lib.SIGNATURES            # the emulator's symbol set is unchanged
        for path in (_lib.LIB_PATH, _lib.LIB_PATHS["fp16"], _lib.LAB_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert lib.vl2_version() == 7


def test_library_refuses_bad_arguments_before_launching(lib):
    p = ctypes.c_void_p(4096)                                       # stand-in device pointers: every case fails its checks first
    odd = ctypes.c_void_p(4100)

    def attn(qkv=p, kpool=p, vpool=p, table=p, cos=p, sin=p, partial=p, out=p, pos_dev=p, B=3, qkv_bs=1536, table_bs=4, n_pages=9, nh=8, nkv=2,
             seq_cap=256, ctx_cap=256):
        return lib.vl2_attn_decode_paged(qkv, kpool, vpool, table, cos, sin, partial, out, B, qkv_bs, table_bs, n_pages, 1024, nh, nkv, seq_cap,
                                         pos_dev, ctx_cap, 0.088, None)

    cases = [(k, -1, "null pointer") for k in (dict(qkv=None), dict(kpool=None), dict(vpool=None), dict(table=None), dict(cos=None), dict(sin=None),
                                               dict(partial=None), dict(out=None), dict(pos_dev=None))]
    cases += [(dict(B=0), -1, "B > 0"), (dict(nh=7), -2, "nh = nkv*group"), (dict(n_pages=0), -2, "n_pages 0"), (dict(n_pages=-3), -2, "n_pages -3"),
              (dict(seq_cap=200, ctx_cap=100), -2, "multiple of 64"), (dict(seq_cap=0), -2, "multiple of 64"),
              (dict(seq_cap=320, ctx_cap=100), -2, "outside a table row of 4 pages"), (dict(ctx_cap=257), -2, "ctx_cap 257 outside seq_cap"),
              (dict(ctx_cap=0), -2, "ctx_cap 0 outside seq_cap"), (dict(kpool=odd), -2, "16-byte aligned"), (dict(vpool=odd), -2, "16-byte aligned"),
              (dict(qkv=odd), -2, "16-byte aligned"), (dict(qkv_bs=1537), -2, "16-byte aligned")]
    for kw, rc, msg in cases:
        assert attn(**kw) == rc, (kw, lib.vl2_last_error_string().decode())
        err = lib.vl2_last_error_string().decode()
        assert msg in err and "vl2_attn_decode_paged" in err, (kw, err)

    def scat(k16=p, v16=p, kpool=p, vpool=p, row=p, nkv=2, smax=256, n_pages=9, p0=0, p1=10):
        return lib.vl2_kv_page_scatter(k16, v16, kpool, vpool, row, nkv, smax, n_pages, p0, p1, None)

    cases = [(k, -1, "null pointer") for k in (dict(k16=None), dict(v16=None), dict(kpool=None), dict(vpool=None), dict(row=None))]
    cases += [(dict(nkv=0), -1, "nkv, smax > 0"), (dict(n_pages=0), -2, "n_pages 0"), (dict(p0=11, p1=10), -2, "rows [11, 10) outside"),
              (dict(p1=257), -2, "rows [0, 257) outside"), (dict(p0=-1), -2, "rows [-1, 10) outside"), (dict(k16=odd), -2, "16-byte aligned"),
              (dict(v16=odd), -2, "16-byte aligned"), (dict(kpool=odd), -2, "16-byte aligned"), (dict(vpool=odd), -2, "16-byte aligned")]
    for kw, rc, msg in cases:
        assert scat(**kw) == rc, (kw, lib.vl2_last_error_string().decode())
        err = lib.vl2_last_error_string().decode()
        assert msg in err and "vl2_kv_page_scatter" in err, (kw, err)
    assert scat(p0=10, p1=10) == 0                                  # an empty range is no error and no launch


def test_wrappers_refuse_before_the_library_is_touched(monkeypatch):
    from videollama2_amd import _lib, ops

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    bf, i32 = torch.bfloat16, torch.int32
    nh, nkv, B, pps = 8, 2, 2, 4
    pool = lambda n=5: torch.zeros(n, nkv, 64, 128, dtype=bf)
    good = dict(qkv=torch.zeros(B, 12 * 128, dtype=bf), kpool=pool(), vpool=pool(), table=torch.zeros(B, pps, dtype=i32), cos_t=torch.zeros(256, 64),
                sin_t=torch.zeros(256, 64), partial=torch.zeros(B * nh * 4 * 130), out=torch.zeros(B, nh * 128, dtype=bf), nh=nh, nkv=nkv,
                pos_dev=torch.zeros(B, dtype=i32), ctx_cap=256, scale=0.088)
    cases = [(dict(nh=7), ValueError, "nh = nkv \\* group"), (dict(qkv=good["qkv"][:, :-128]), ValueError, "qkv must be"),
             (dict(qkv=good["qkv"].half()), TypeError, "qkv must be torch.bfloat16"), (dict(kpool=pool().half()), TypeError, "kpool must be"),
             (dict(table=good["table"].long()), TypeError, "table must be torch.int32"),
             (dict(pos_dev=good["pos_dev"].long()), TypeError, "pos_dev must be torch.int32"),
             (dict(kpool=torch.zeros(5, nkv, 32, 128, dtype=bf)), ValueError, "pools must be \\[n_pages, nkv, 64, 128\\]"),
             (dict(vpool=pool(6)), ValueError, "pools must be"), (dict(kpool=torch.zeros(5, 3, 64, 128, dtype=bf), vpool=torch.zeros(5, 3, 64, 128, dtype=bf)),
                                                                 ValueError, "pools must be"),
             (dict(kpool=pool(10)[::2], vpool=pool(10)[::2]), ValueError, "pages must be contiguous"),
             (dict(table=good["table"][0]), ValueError, "page table must be int32"), (dict(table=good["table"][:1]), ValueError, "page table must be int32"),
             (dict(table=torch.zeros(B, 8, dtype=i32)[:, ::2]), ValueError, "page table must be int32"),
             (dict(ctx_cap=257), ValueError, "ctx_cap 257 outside the table's 256"), (dict(ctx_cap=0), ValueError, "ctx_cap 0 outside"),
             (dict(cos_t=torch.zeros(255, 64), sin_t=torch.zeros(255, 64)), ValueError, "cos / sin tables"),
             (dict(pos_dev=good["pos_dev"][:1]), ValueError, "positions"), (dict(out=good["out"][:, :-1]), ValueError, "out \\[B, nh \\* 128\\]"),
             (dict(partial=good["partial"][:-1]), ValueError, "partial holds"), ({}, ValueError, "must be a device tensor")]
    for kw, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            ops.attn_decode_paged(**{**good, **kw})
    cache = lambda: torch.zeros(nkv, 256, 128, dtype=bf)
    good = dict(kcache=cache(), vcache=cache(), kpool=pool(), vpool=pool(), table_row=torch.zeros(pps, dtype=i32), p0=0, p1=10)
    cases = [(dict(kcache=cache().half()), TypeError, "kcache must be"), (dict(table_row=good["table_row"].long()), TypeError, "table_row must be torch.int32"),
             (dict(vpool=pool().float()), TypeError, "vpool must be"), (dict(kpool=pool()[:, :, :32]), ValueError, "pools must be"),
             (dict(kcache=cache()[:1], vcache=cache()[:1]), ValueError, "contiguous 16-bit caches"),
             (dict(kcache=torch.zeros(nkv, 512, 128, dtype=bf)[:, ::2]), ValueError, "contiguous 16-bit caches"),
             (dict(table_row=good["table_row"][:3]), ValueError, "at least 4 entries"), (dict(table_row=torch.zeros(1, pps, dtype=i32)), ValueError, "table row must be"),
             (dict(p0=11), ValueError, "rows \\[11, 10\\) outside"), (dict(p1=257), ValueError, "rows \\[0, 257\\) outside"),
             (dict(p0=-1), ValueError, "rows \\[-1, 10\\) outside"), ({}, ValueError, "must be a device tensor")]
    for kw, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            ops.kv_page_scatter(**{**good, **kw})
    with pytest.raises(ValueError, match="n_pages >= 1"):
        ops.kv_pool_alloc(0, nkv, "cpu")
    kp, vp = ops.kv_pool_alloc(3, nkv, "cpu")
    assert kp.shape == vp.shape == (3, nkv, 64, 128) and kp.dtype == bf and not kp.any() and kp.data_ptr() != vp.data_ptr()


# ---------------------------------------------------------------------------------------------------------------- refusals
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


def _no_kernels(monkeypatch):
    """Any kernel call fails the test: the refusals must come before the first one."""
    from videollama2_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a kernel was called")
    monkeypatch.setattr(_lib, "call", boom)


def test_decoder_model_and_batcher_refusals_come_with_their_reasons_before_any_kernel(golden_small, monkeypatch):
    import torch.distributed as dist
    from tests.emu.backend import emulated_backend
    from videollama2_amd.decoder import HipMistralDecoder, HipMixtralDecoder
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.serving import ContinuousBatcher
    cfg = golden_small["cfg"]
    sd = O.seeded_state_dict(cfg, golden_small["seed"], only=_keep)
    x = torch.zeros(3, cfg["llm"]["hidden_size"], dtype=torch.bfloat16)
    with emulated_backend():
        dec = HipMistralDecoder(cfg, sd, "cpu", max_seq_len=256)
        assert dec.paged_kv is False
        assert dec.kv_page_bytes() == dec.n_layers * 2 * dec.nkv * 64 * 128 * 2
        _no_kernels(monkeypatch)
        # each KV switch refuses the other
        dec.enable_fp8_kv()
        with pytest.raises(NotImplementedError, match="paged KV cache: the fp8 KV cache is on.*enable_fp8_kv\\(False\\)"):
            dec.enable_paged_kv(8)
        dec.enable_fp8_kv(False)
        assert dec.enable_paged_kv(8) is dec and dec.paged_kv is True and dec._bb is None
        with pytest.raises(NotImplementedError, match="fp8 KV cache: the paged KV cache is on.*enable_paged_kv\\(0, False\\)"):
            dec.enable_fp8_kv()
        assert dec.fp8_kv is False
        with pytest.raises(ValueError, match="page 0 is the parking page"):
            dec.enable_paged_kv(1)
        # the shared prefix, at the decoder and at the model (before the encoder runs)
        with pytest.raises(NotImplementedError, match="shared-prefix decode: the paged KV cache is on.*enable_paged_kv\\(0, False\\)"):
            dec.generate_batch([x, x], max_new_tokens=2, shared_prefix=x)
        m = VideoLLaMA2Hip.__new__(VideoLLaMA2Hip)
        torch.nn.Module.__init__(m)
        m.decoder = dec
        with pytest.raises(NotImplementedError, match="shared-prefix decode: the paged KV cache is on"):
            m.generate_shared([(torch.tensor([1, 5, 6, 7]), None), (torch.tensor([1, 5, 6, 8]), None)], max_new_tokens=2)
        assert m.enable_paged_kv(8) is m and dec.paged_kv
        # a pool that cannot hold every reservation: refused with the figures, before any kernel, every page still free
        long = torch.zeros(130, x.shape[1], dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="need 9 pages \\(\\[3, 3, 3\\]\\), the pool has 7 free \\(of 7"):
            dec.generate_batch([long, long, long], max_new_tokens=60, use_graph=False)
        assert dec._bb["pool"].n_free == 7 and dec._bb["table"].tolist() == [[0, -1, -1, -1]] * 3
        assert not any(k in dec._bb for k in ("k", "v", "kv8"))
        with pytest.raises(ValueError, match="exceeds the KV cache"):
            dec.generate_batch([torch.zeros(257, x.shape[1])], max_new_tokens=2, use_graph=False)
        # the batcher: a request larger than the whole pool can never run (a reservation is at most ceil(max_seq_len / 64) = 4 pages here)
        dec.enable_paged_kv(4)
        b = ContinuousBatcher(dec, max_slots=2, use_graph=False)
        with pytest.raises(ValueError, match="needs 4 pages \\(200 prompt rows \\+ 57 new tokens\\), the pool serves 3"):
            b.submit(torch.zeros(200, x.shape[1]), max_new_tokens=500)
        assert b.in_flight() == 0
        rid = b.submit(torch.zeros(100, x.shape[1]), max_new_tokens=29)         # 129 rows: 3 pages
        assert b.waiting[0].need == 3 and b.waiting[0].rid == rid
        # ... and with it waiting the switch is refused
        dec._bb_busy = b
        with pytest.raises(RuntimeError, match="enable_paged_kv: a ContinuousBatcher holds requests in flight"):
            dec.enable_paged_kv(0, False)
        b.waiting.clear()
        # switches that can be set after the slots exist
        dec.tp_always_reduce = True
        with pytest.raises(NotImplementedError, match="paged KV cache: single-rank decoders only"):
            dec._decode_kernels_batched(2)
        with pytest.raises(NotImplementedError, match="paged KV cache: single-rank decoders only"):
            dec.enable_paged_kv(8)
        dec.tp_always_reduce = False
        dec.enable_paged_kv(0, False)
        assert dec.paged_kv is False and dec._bb is None
        dec.hd = 64
        with pytest.raises(NotImplementedError, match="paged KV cache: head_dim 128 only \\(this decoder has 64\\)"):
            dec.enable_paged_kv(8)
        dec.hd = 128
        with pytest.raises(NotImplementedError, match="mixtral.*paged KV cache is not built"):
            HipMixtralDecoder.enable_paged_kv(object.__new__(HipMixtralDecoder), 8)
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        with emulated_backend():
            tp = HipMistralDecoder(cfg, sd, "cpu", max_seq_len=16, tp_group=dist.group.WORLD)
            with pytest.raises(NotImplementedError, match="paged KV cache: single-rank decoders only"):
                tp.enable_paged_kv(8)
    finally:
        dist.destroy_process_group()
