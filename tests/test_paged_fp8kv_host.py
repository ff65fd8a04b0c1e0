"""The paged KV cache in fp8, host side only (no launch): the declarations of the two entry points against the ctypes
table, the argument refusals of the library and of the Python wrappers (before anything is enqueued), the decoder's switch
enable_paged_kv(n_pages, fp8=True) on the emulated backend -- its properties, both old cross-refusals with their old text, the slot buffers it
allocates, every refusal with its reason before any kernel -- and, with recording stubs, the launches a prefill and a batched step issue and
the pages generate_batch gives back."""
import ctypes
import os
import re

import pytest
import torch

from oracle import vl2_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
NAMES = ("vl2_attn_decode_kv8_paged", "vl2_kv_page_quant")
ATTENTION_CALLS = ("vl2_attn_decode", "vl2_attn_decode_batched", "vl2_attn_decode_kv8", "vl2_attn_decode_kv8_batched", "vl2_attn_decode_paged",
                   "vl2_attn_decode_shared", "vl2_attn_decode_shared_paged", "vl2_attn_decode_fused")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib
    return _lib.load()


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
    assert set(_lib.PAGED_FP8KV_SIGNATURES) == set(NAMES)
    for name in NAMES:
        ret, args = _declared(name)
        assert ret is ctypes.c_int32 and args == _lib.PAGED_FP8KV_SIGNATURES[name], name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is ctypes.c_int32
        assert name in _lib.EXPORTS and name not in _lib.SIGNATURES            # the emulator's symbol set is unchanged
        assert name not in _lib.PAGED_KV_SIGNATURES and name not in _lib.FP8KV_SIGNATURES and name not in _lib.PAGED_PREFIX_SIGNATURES
        for path in (_lib.LIB_PATH, _lib.LIB_PATHS["fp16"], _lib.LAB_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert lib.vl2_version() == 7


def test_library_refuses_bad_arguments_before_launching(lib):
    p = ctypes.c_void_p(4096)                                       # stand-in device pointers: every case fails its checks first
    odd = ctypes.c_void_p(4100)

    def attn(qkv=p, k8=p, v8=p, ks=p, vs=p, table=p, cos=p, sin=p, partial=p, out=p, pos_dev=p, B=3, qkv_bs=1536, table_bs=4, n_pages=9, nh=8, nkv=2,
             seq_cap=256, ctx_cap=256):
        return lib.vl2_attn_decode_kv8_paged(qkv, k8, v8, ks, vs, table, cos, sin, partial, out, B, qkv_bs, table_bs, n_pages, 1024, nh, nkv, seq_cap,
                                             pos_dev, ctx_cap, 0.088, None)

    cases = [(k, -1, "null pointer") for k in (dict(qkv=None), dict(k8=None), dict(v8=None), dict(ks=None), dict(vs=None), dict(table=None),
                                               dict(cos=None), dict(sin=None), dict(partial=None), dict(out=None), dict(pos_dev=None))]
    cases += [(dict(B=0), -1, "B > 0"), (dict(nh=7), -2, "nh = nkv*group"), (dict(n_pages=0), -2, "n_pages 0"), (dict(n_pages=-3), -2, "n_pages -3"),
              (dict(seq_cap=200, ctx_cap=100), -2, "multiple of 64"), (dict(seq_cap=0), -2, "multiple of 64"),
              (dict(seq_cap=320, ctx_cap=100), -2, "outside a table row of 4 pages"), (dict(ctx_cap=257), -2, "ctx_cap 257 outside seq_cap"),
              (dict(ctx_cap=0), -2, "ctx_cap 0 outside seq_cap"), (dict(k8=odd), -2, "16-byte aligned"), (dict(v8=odd), -2, "16-byte aligned"),
              (dict(qkv=odd), -2, "16-byte aligned"), (dict(qkv_bs=1537), -2, "16-byte aligned"), (dict(B=40000), -2, "too many sequences (40000)")]
    for kw, rc, msg in cases:
        assert attn(**kw) == rc, (kw, lib.vl2_last_error_string().decode())
        err = lib.vl2_last_error_string().decode()
        assert msg in err and "vl2_attn_decode_kv8_paged" in err, (kw, err)

    def quant(k16=p, v16=p, k8=p, v8=p, ks=p, vs=p, row=p, nkv=2, smax=256, n_pages=9, p0=0, p1=10):
        return lib.vl2_kv_page_quant(k16, v16, k8, v8, ks, vs, row, nkv, smax, n_pages, p0, p1, None)

    cases = [(k, -1, "null pointer") for k in (dict(k16=None), dict(v16=None), dict(k8=None), dict(v8=None), dict(ks=None), dict(vs=None), dict(row=None))]
    cases += [(dict(nkv=0), -1, "nkv, smax > 0"), (dict(smax=0), -1, "nkv, smax > 0"), (dict(n_pages=0), -2, "n_pages 0"),
              (dict(p0=11, p1=10), -2, "rows [11, 10) outside"), (dict(p1=257), -2, "rows [0, 257) outside"), (dict(p0=-1), -2, "rows [-1, 10) outside"),
              (dict(k16=odd), -2, "16-byte aligned"), (dict(v16=odd), -2, "16-byte aligned"), (dict(k8=odd), -2, "16-byte aligned"),
              (dict(v8=odd), -2, "16-byte aligned")]
    for kw, rc, msg in cases:
        assert quant(**kw) == rc, (kw, lib.vl2_last_error_string().decode())
        err = lib.vl2_last_error_string().decode()
        assert msg in err and "vl2_kv_page_quant" in err, (kw, err)
    assert quant(p0=10, p1=10) == 0                                 # an empty range is no error and no launch


def test_wrappers_refuse_before_the_library_is_touched(monkeypatch):
    from videollama2_amd import _lib, ops

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    bf, i32, u8, f32 = torch.bfloat16, torch.int32, torch.uint8, torch.float32
    nh, nkv, B, pps = 8, 2, 2, 4
    codes = lambda n=5, nkv=nkv: torch.zeros(n, nkv, 64, 128, dtype=u8)
    scales = lambda n=5, nkv=nkv: torch.ones(n, nkv, 64, dtype=f32)
    pools = lambda **kw: tuple(kw.get(k, mk()) for k, mk in (("k8", codes), ("v8", codes), ("ks", scales), ("vs", scales)))
    good = dict(qkv=torch.zeros(B, 12 * 128, dtype=bf), pools8=pools(), table=torch.zeros(B, pps, dtype=i32), cos_t=torch.zeros(256, 64),
                sin_t=torch.zeros(256, 64), partial=torch.zeros(B * nh * 4 * 130), out=torch.zeros(B, nh * 128, dtype=bf), nh=nh, nkv=nkv,
                pos_dev=torch.zeros(B, dtype=i32), ctx_cap=256, scale=0.088)
    pool_cases = [(pools(k8=codes().to(bf)), TypeError, "k8pool must be torch.uint8"), (pools(v8=codes().char()), TypeError, "v8pool must be torch.uint8"),
                  (pools(ks=scales().to(bf)), TypeError, "kspool must be torch.float32"), (pools(vs=scales().double()), TypeError, "vspool must be torch.float32"),
                  (pools(k8=torch.zeros(5, nkv, 32, 128, dtype=u8)), ValueError, "pools must be codes \\[n_pages, nkv, 64, 128\\] and scales \\[n_pages, nkv, 64\\]"),
                  (pools(v8=codes(6)), ValueError, "pools must be codes"), (pools(ks=scales(6)), ValueError, "pools must be codes"),
                  (pools(vs=torch.ones(5, nkv, 64, 1)), ValueError, "pools must be codes"), (pools(ks=torch.ones(5, nkv, 32)), ValueError, "pools must be codes"),
                  (pools(k8=codes(10)[::2]), ValueError, "pages must be contiguous"), (pools(vs=scales(10)[::2]), ValueError, "pages must be contiguous")]
    cases = [(dict(nh=7), ValueError, "nh = nkv \\* group"), (dict(qkv=good["qkv"][:, :-128]), ValueError, "qkv must be"),
             (dict(qkv=good["qkv"].half()), TypeError, "qkv must be torch.bfloat16"),
             (dict(table=good["table"].long()), TypeError, "table must be torch.int32"),
             (dict(pos_dev=good["pos_dev"].long()), TypeError, "pos_dev must be torch.int32")]
    cases += [(dict(pools8=ps), exc, msg) for ps, exc, msg in pool_cases]
    cases += [(dict(pools8=tuple(t(5, 3) for t in (codes, codes, scales, scales))), ValueError, "pools must be codes"),
              (dict(table=good["table"][0]), ValueError, "page table must be int32"), (dict(table=good["table"][:1]), ValueError, "page table must be int32"),
              (dict(table=torch.zeros(B, 8, dtype=i32)[:, ::2]), ValueError, "page table must be int32"),
              (dict(ctx_cap=257), ValueError, "ctx_cap 257 outside the table's 256"), (dict(ctx_cap=0), ValueError, "ctx_cap 0 outside"),
              (dict(table=good["table"][:, :3]), ValueError, "ctx_cap 256 outside the table's 192"),          # a short table row
              (dict(cos_t=torch.zeros(255, 64), sin_t=torch.zeros(255, 64)), ValueError, "cos / sin tables"),
              (dict(pos_dev=good["pos_dev"][:1]), ValueError, "positions"), (dict(out=good["out"][:, :-1]), ValueError, "out \\[B, nh \\* 128\\]"),
              (dict(partial=good["partial"][:-1]), ValueError, "partial holds"), ({}, ValueError, "must be a device tensor")]
    for kw, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            ops.attn_decode_kv8_paged(**{**good, **kw})
    cache = lambda: torch.zeros(nkv, 256, 128, dtype=bf)
    good = dict(kcache=cache(), vcache=cache(), pools8=pools(), table_row=torch.zeros(pps, dtype=i32), p0=0, p1=10)
    cases = [(dict(kcache=cache().half()), TypeError, "kcache must be"), (dict(table_row=good["table_row"].long()), TypeError, "table_row must be torch.int32")]
    cases += [(dict(pools8=ps), exc, msg) for ps, exc, msg in pool_cases]
    cases += [(dict(kcache=cache()[:1], vcache=cache()[:1]), ValueError, "contiguous 16-bit caches"),
              (dict(kcache=torch.zeros(nkv, 512, 128, dtype=bf)[:, ::2]), ValueError, "contiguous 16-bit caches"),
              (dict(table_row=good["table_row"][:3]), ValueError, "at least 4 entries"), (dict(table_row=torch.zeros(1, pps, dtype=i32)), ValueError, "table row must be"),
              (dict(p0=11), ValueError, "rows \\[11, 10\\) outside"), (dict(p1=257), ValueError, "rows \\[0, 257\\) outside"),
              (dict(p0=-1), ValueError, "rows \\[-1, 10\\) outside"), ({}, ValueError, "must be a device tensor")]
    for kw, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            ops.kv_page_quant(**{**good, **kw})
    with pytest.raises(ValueError, match="n_pages >= 1"):
        ops.kv8_pool_alloc(0, nkv, "cpu")
    k8, v8, ks, vs = ops.kv8_pool_alloc(3, nkv, "cpu")
    assert k8.shape == v8.shape == (3, nkv, 64, 128) and k8.dtype == v8.dtype == u8 and not k8.any() and not v8.any()
    assert ks.shape == vs.shape == (3, nkv, 64) and ks.dtype == vs.dtype == f32 and bool((ks == 1).all()) and bool((vs == 1).all())
    assert len({t.data_ptr() for t in (k8, v8, ks, vs)}) == 4


# ---------------------------------------------------------------------------------------------------------------- the decoder's switch
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


def test_switch_properties_cross_refusals_and_slot_buffers(stubbed):
    dec, calls, arm = stubbed
    arm()
    page16 = dec.n_layers * 2 * dec.nkv * 64 * 128 * 2
    page8 = dec.n_layers * 2 * dec.nkv * 64 * (128 + 4)
    assert dec.paged_kv_fp8 is False and dec.kv_page_bytes() == page16
    # 16-bit pages: today's figures
    assert dec.enable_paged_kv(8) is dec and dec.paged_kv and dec.paged_kv_fp8 is False and dec.kv_page_bytes() == page16
    # fp8 pages, from a decoder whose fp8_kv is off -- and it stays off
    assert dec._ensure_batch(2) is dec._bb and "kpool" in dec._bb
    assert dec.enable_paged_kv(8, fp8=True) is dec
    assert dec.paged_kv is True and dec.paged_kv_fp8 is True and dec.fp8_kv is False and dec.kv8 is None and dec._bb is None
    assert dec.kv_page_bytes() == page8 and page8 * 64 == page16 * 33
    with pytest.raises(NotImplementedError, match="fp8 KV cache: the paged KV cache is on .*: call enable_paged_kv\\(0, False\\) first"):
        dec.enable_fp8_kv()                                          # refused under fp8 pages as under 16-bit ones
    assert dec.fp8_kv is False and dec.paged_kv_fp8
    # switching the page format drops the slot buffers, either way
    bb = dec._ensure_batch(2)
    assert dec._bb is bb
    dec.enable_paged_kv(8)
    assert dec._bb is None and dec.paged_kv and not dec.paged_kv_fp8 and dec.kv_page_bytes() == page16
    bb16 = dec._ensure_batch(2)
    assert "kpool" in bb16 and "pools8" not in bb16
    dec.enable_paged_kv(8, fp8=True)
    assert dec._bb is None and dec.paged_kv_fp8
    # off: the keyword leaves nothing behind
    dec.enable_paged_kv(0, False, fp8=True)
    assert dec.paged_kv is False and dec.paged_kv_fp8 is False and dec.kv_page_bytes() == page16
    # both old cross-refusals keep their text, and the combination is entered through the keyword only
    dec.enable_fp8_kv()
    with pytest.raises(NotImplementedError, match="paged KV cache: the fp8 KV cache is on \\(the pages hold 16-bit rows\\): call enable_fp8_kv\\(False\\) first"):
        dec.enable_paged_kv(8)
    with pytest.raises(NotImplementedError, match="paged KV cache: the fp8 KV cache is on \\(the pages hold 16-bit rows\\): call enable_fp8_kv\\(False\\) first"):
        dec.enable_paged_kv(8, fp8=True)
    assert dec.fp8_kv and not dec.paged_kv
    dec.enable_fp8_kv(False)
    dec.enable_paged_kv(8)
    with pytest.raises(NotImplementedError,
                       match="fp8 KV cache: the paged KV cache is on \\(its pages hold 16-bit rows\\): call enable_paged_kv\\(0, False\\) first"):
        dec.enable_fp8_kv()
    # the slot buffers on fp8 pages: four pools per layer (codes 0, scales 1), the parked table, the allocator, the 16-bit staging cache,
    # and no key of another layout
    dec.enable_paged_kv(5, fp8=True)
    bb = dec._ensure_batch(3)
    assert not any(k in bb for k in ("k", "v", "kv8", "kpool", "vpool"))
    assert len(bb["pools8"]) == dec.n_layers
    for k8, v8, ks, vs in bb["pools8"]:
        assert k8.shape == v8.shape == (5, dec.nkv, 64, 128) and k8.dtype == v8.dtype == torch.uint8 and not k8.any() and not v8.any()
        assert ks.shape == vs.shape == (5, dec.nkv, 64) and ks.dtype == vs.dtype == torch.float32 and bool((ks == 1).all()) and bool((vs == 1).all())
    assert bb["table"].tolist() == [[0, -1, -1, -1]] * 3 and bb["table"].dtype == torch.int32
    assert bb["pool"].n_free == 4 and bb["pages_per_seq"] == 4 and bb["cos_t"].shape[0] >= 256
    assert [tuple(t.shape) for grp in bb["stage"] for t in grp] == [(dec.nkv, 256, 128)] * (2 * dec.n_layers)
    assert all(t.dtype == torch.bfloat16 for grp in bb["stage"] for t in grp)
    pool_bytes = sum(t.numel() * t.element_size() for ps in bb["pools8"] for t in ps)
    assert pool_bytes == 5 * dec.kv_page_bytes()
    assert calls == []


def test_refusals_come_with_their_reasons_before_any_kernel(stubbed, golden_small):
    import torch.distributed as dist
    from tests.emu.backend import emulated_backend
    from videollama2_amd.decoder import HipMistralDecoder, HipMixtralDecoder
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.serving import ContinuousBatcher
    dec, calls, arm = stubbed
    arm()
    x = _x(3, dec)
    dec.enable_paged_kv(8, fp8=True)
    with pytest.raises(ValueError, match="page 0 is the parking page"):
        dec.enable_paged_kv(1, fp8=True)
    # the shared prefix: generate_batch(shared_prefix=), the model's generate_shared, the batcher's open_prefix
    with pytest.raises(NotImplementedError, match="shared-prefix decode: the paged KV cache is on.*enable_paged_kv\\(0, False\\)"):
        dec.generate_batch([x, x], max_new_tokens=2, shared_prefix=x)
    m = VideoLLaMA2Hip.__new__(VideoLLaMA2Hip)
    torch.nn.Module.__init__(m)
    m.decoder = dec
    with pytest.raises(NotImplementedError, match="shared-prefix decode: the paged KV cache is on"):
        m.generate_shared([(torch.tensor([1, 5, 6, 7]), None), (torch.tensor([1, 5, 6, 8]), None)], max_new_tokens=2)
    b = ContinuousBatcher(dec, max_slots=2, use_graph=False)
    with pytest.raises(NotImplementedError, match="open_prefix: the pages hold fp8 rows and no fp8 form of the shared-prefix kernels is built"):
        b.open_prefix(_x(130, dec))
    assert dec._bb["pool"].n_free == 7 and dec._bb["table"].tolist() == [[0, -1, -1, -1]] * 2 and b._prefix is None
    # the model-level switch passes the keyword through
    dec.enable_paged_kv(0, False)
    assert m.enable_paged_kv(8, fp8=True) is m and dec.paged_kv_fp8 and dec.fp8_kv is False
    assert m.enable_paged_kv(8) is m and dec.paged_kv and not dec.paged_kv_fp8
    m.enable_paged_kv(8, True, True)
    assert dec.paged_kv_fp8
    # a pool that cannot hold every reservation: refused with the figures, every page still free
    long = _x(130, dec)
    with pytest.raises(ValueError, match="need 9 pages \\(\\[3, 3, 3\\]\\), the pool has 7 free \\(of 7"):
        dec.generate_batch([long, long, long], max_new_tokens=60, use_graph=False)
    assert dec._bb["pool"].n_free == 7 and dec._bb["table"].tolist() == [[0, -1, -1, -1]] * 3
    with pytest.raises(ValueError, match="exceeds the KV cache"):
        dec.generate_batch([_x(257, dec)], max_new_tokens=2, use_graph=False)
    # a batcher with requests in flight: the format switch is refused, in both directions
    dec.enable_paged_kv(4, fp8=True)
    b = ContinuousBatcher(dec, max_slots=2, use_graph=False)
    with pytest.raises(ValueError, match="needs 4 pages \\(200 prompt rows \\+ 57 new tokens\\), the pool serves 3"):
        b.submit(_x(200, dec), max_new_tokens=500)
    assert b.in_flight() == 0
    b.submit(_x(100, dec), max_new_tokens=29)
    assert b.waiting[0].need == 3
    dec._bb_busy = b
    for args in ((8,), (8, True, True), (0, False)):
        with pytest.raises(RuntimeError, match="enable_paged_kv: a ContinuousBatcher holds requests in flight"):
            dec.enable_paged_kv(*args)
    assert dec.paged_kv_fp8
    b.waiting.clear()
    # tensor parallelism (also when it is set after the slots exist), head_dim, Mixtral
    dec.tp_always_reduce = True
    with pytest.raises(NotImplementedError, match="paged KV cache: single-rank decoders only"):
        dec._decode_kernels_batched(2)
    with pytest.raises(NotImplementedError, match="paged KV cache: single-rank decoders only"):
        dec.enable_paged_kv(8, fp8=True)
    dec.tp_always_reduce = False
    dec.enable_paged_kv(0, False)
    dec.hd = 64
    with pytest.raises(NotImplementedError, match="paged KV cache: head_dim 128 only \\(this decoder has 64\\)"):
        dec.enable_paged_kv(8, fp8=True)
    dec.hd = 128
    assert not dec.paged_kv and not dec.paged_kv_fp8
    with pytest.raises(NotImplementedError, match="mixtral.*paged KV cache is not built"):
        HipMixtralDecoder.enable_paged_kv(object.__new__(HipMixtralDecoder), 8, fp8=True)
    with pytest.raises(NotImplementedError, match="mixtral.*paged KV cache is not built"):
        HipMixtralDecoder.enable_paged_kv(object.__new__(HipMixtralDecoder), 8, True, True)
    assert calls == []
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        with emulated_backend():
            cfg = golden_small["cfg"]
            tp = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, golden_small["seed"], only=_keep), "cpu", max_seq_len=16, tp_group=dist.group.WORLD)
            with pytest.raises(NotImplementedError, match="paged KV cache: single-rank decoders only"):
                tp.enable_paged_kv(8, fp8=True)
    finally:
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------- the launches
def test_prefill_slot_quantises_once_per_layer_and_a_step_attends_once_per_layer(stubbed):
    from videollama2_amd import ops
    dec, calls, arm = stubbed
    dec.enable_paged_kv(8, fp8=True)
    bb = dec._ensure_batch(3)
    dec._set_table_rows(1, [[5, 2, 7, -1]])
    S = 130
    own_pos = dec.pos
    dec.prefill_slot(1, _x(S, dec), bb["logits"][1])
    assert dec.pos == own_pos
    quant = [a for n, a in calls if n == "vl2_kv_page_quant"]
    assert len(quant) == dec.n_layers and not any(n in ("vl2_kv_page_scatter", "vl2_kv_quant") for n, _ in calls)
    row = bb["table"][1]
    for li, a in enumerate(quant):
        k8, v8, ks, vs = bb["pools8"][li]
        assert a[:7] == (bb["stage"][0][li].data_ptr(), bb["stage"][1][li].data_ptr(), k8.data_ptr(), v8.data_ptr(), ks.data_ptr(), vs.data_ptr(),
                         row.data_ptr()), li
        assert a[7:12] == (dec.nkv, 256, 8, 0, S), li                # nkv, smax, n_pages, [0, S)
    assert row.tolist() == [5, 2, 7, -1] and row.data_ptr() == bb["table"].data_ptr() + 4 * 4
    # one batched step: one vl2_attn_decode_kv8_paged per layer and no other attention call
    for nb in (2, dec.GEMM_BATCH):
        dec.enable_paged_kv(8, fp8=True)
        bb = dec._ensure_batch(nb)
        del calls[:]
        dec._decode_kernels_batched(nb)
        attn = [a for n, a in calls if n == "vl2_attn_decode_kv8_paged"]
        assert len(attn) == dec.n_layers and not any(n in ATTENTION_CALLS for n, _ in calls), nb
        for li, a in enumerate(attn):
            assert a[1:6] == tuple(t.data_ptr() for t in bb["pools8"][li]) + (bb["table"].data_ptr(),), (nb, li)
            assert a[10] == nb and a[12:14] == (4, 8) and a[15:18] == (dec.nh, dec.nkv, 256) and a[18] == bb["pos"].data_ptr() and a[19] == 256
    # ... and on 16-bit pages the step is unchanged
    dec.enable_paged_kv(8)
    dec._ensure_batch(2)
    del calls[:]
    dec._decode_kernels_batched(2)
    names = [n for n, _ in calls]
    assert names.count("vl2_attn_decode_paged") == dec.n_layers and "vl2_attn_decode_kv8_paged" not in names
    assert ops.KV_PAGE_ROWS == 64


def test_generate_batch_returns_every_page_on_success_and_on_an_exception(stubbed, monkeypatch):
    dec, calls, arm = stubbed
    dec.enable_paged_kv(8, fp8=True)
    xs = [_x(70, dec), _x(5, dec), _x(129, dec)]
    seen = []
    real = dec.prefill_slot

    def watching(slot, x, logits_out):
        seen.append((slot, dec._bb["table"][slot].tolist(), dec._bb["pool"].n_free))
        return real(slot, x, logits_out)
    monkeypatch.setattr(dec, "prefill_slot", watching)
    outs = dec.generate_batch(xs, max_new_tokens=4, use_graph=False)
    assert [len(o) for o in outs] == [4, 4, 4]
    assert seen == [(0, [1, 2, -1, -1], 1), (1, [3, -1, -1, -1], 1), (2, [4, 5, 6, -1], 1)]          # 2 + 1 + 3 pages of 7, reserved up front
    bb = dec._bb
    assert bb["pool"].n_free == 7 and bb["table"].tolist() == [[0, -1, -1, -1]] * 3
    names = [n for n, _ in calls]
    assert names.count("vl2_kv_page_quant") == 3 * dec.n_layers and names.count("vl2_attn_decode_kv8_paged") == 3 * dec.n_layers
    assert not any(n in ATTENTION_CALLS or n in ("vl2_kv_page_scatter", "vl2_kv_quant") for n in names)

    def broken(*a, **k):
        assert dec._bb["pool"].n_free == 7 - 3
        raise RuntimeError("prefill failed")
    monkeypatch.setattr(dec, "prefill_slot", broken)
    with pytest.raises(RuntimeError, match="prefill failed"):
        dec.generate_batch(xs[:2], max_new_tokens=4, use_graph=False)
    assert bb is dec._bb and bb["pool"].n_free == 7 and bb["table"].tolist() == [[0, -1, -1, -1]] * 3
