"""The fp8 KV cache, host side only (no launch): the format's known answers (tests/fp8kv_oracle.py), the declarations of the three entry
points (exported, bound in a table of their own, declared outside the experimental block, refusing bad arguments before anything is
enqueued) and the decoder's refusals, which must come before the first kernel call (the emulator has no kv8 kernels)."""
import ctypes
import os
import re

import pytest
import torch

from oracle import fp8_oracle as F8
from oracle import vl2_oracle as O
from tests import fp8kv_oracle as KV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vl2_kv_quant", "vl2_attn_decode_kv8", "vl2_attn_decode_kv8_batched")


# ---------------------------------------------------------------------------------------------------------------- the format
def test_zero_row_gets_scale_one_and_zero_codes():
    q, s = KV.quant_cache_rows(torch.zeros(2, 3, 128))
    assert q.shape == (2, 3, 128) and s.shape == (2, 3)
    assert torch.equal(s, torch.ones(2, 3)) and int(q.max()) == 0
    assert torch.equal(KV.dequant_cache(q, s), torch.zeros(2, 3, 128))


@pytest.mark.parametrize("e", [-100, -20, -3, 0, 5, 40])
def test_amax_at_and_just_above_448_times_a_power_of_two(e):
    at = torch.zeros(1, 2, 128)
    at[0, 0, 17] = -448.0 * 2.0 ** e                      # exactly 448 * 2^e: lands on e
    at[0, 1, 90] = torch.nextafter(torch.tensor(448.0 * 2.0 ** e), torch.tensor(float("inf")))      # one ulp above: e + 1
    at[0, :, 3] = 2.0 ** e
    q, s = KV.quant_cache_rows(at)
    assert s[0, 0].item() == 2.0 ** e and s[0, 1].item() == 2.0 ** (e + 1)
    assert q[0, 0, 17].item() == 0xFE and q[0, 0, 3].item() == 0x38          # -448 and 1.0
    assert q[0, 1, 90].item() == 0x76 and q[0, 1, 3].item() == 0x30          # 224 (448 / 2, the tie goes to the even code) and 0.5


def test_round_trip_error_of_normal_codes():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(4, 64, 128, generator=g) * torch.exp2(torch.randint(-12, 12, (4, 64, 1), generator=g).float())).bfloat16()
    q, s = KV.quant_cache_rows(x)
    d = KV.dequant_cache(q, s)
    normal = (q & 0x78) != 0                              # exponent field non-zero: 4 significant bits, half an ulp = 2^-4 relative
    assert normal.float().mean() > 0.9
    xf = x.float()
    assert bool(((d - xf).abs() <= 2.0 ** -4 * xf.abs())[normal].all())
    assert torch.equal(d.bfloat16().float(), d)          # code * 2^e is a bf16 number
    assert torch.equal(KV.qdq(d), d)                      # rows on the grid stay where they are
    # the [nkv * rows, 128] view is what defines it
    q2, s2 = F8.quant_rows(x.reshape(-1, 128))
    assert torch.equal(q.reshape(-1, 128), q2) and torch.equal(s.reshape(-1), s2)


def test_attention_reference_against_the_oracle_layer_arithmetic():
    g = torch.Generator().manual_seed(4)
    nh, nkv, ctx = 4, 2, 9
    q, k, v = torch.randn(nh, 128, generator=g), torch.randn(nkv, ctx, 128, generator=g), torch.randn(nkv, ctx, 128, generator=g)
    out = KV.attn_decode_ref(q, k, v, 128 ** -0.5).view(nh, 128)
    kk, vv = k.repeat_interleave(2, 0), v.repeat_interleave(2, 0)
    ref = torch.softmax(torch.einsum("hd,hsd->hs", q, kk) * 128 ** -0.5, -1)
    assert torch.allclose(out, torch.einsum("hs,hsd->hd", ref, vv), atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------- declarations
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.vl2_last_error_string().decode()


def test_entry_points_are_exported_and_bound_in_a_table_of_their_own(lib):
    from videollama2_amd import _lib
    assert set(_lib.FP8KV_SIGNATURES) == set(NAMES)
    for path in (_lib.LIB_PATH, _lib.LIB_PATHS["fp16"], _lib.LAB_LIB_PATH):
        plain = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(plain, name), (path, name)
    for name in NAMES:
        assert name in _lib.EXPORTS and name not in _lib.SIGNATURES            # the emulator's symbol set is unchanged
        assert getattr(lib, name).argtypes == _lib.FP8KV_SIGNATURES[name]
    assert lib.vl2_version() == 7


def test_header_declares_them_outside_the_experimental_block():
    header = open(os.path.join(ROOT, "include", "vl2hip.h")).read()
    product = re.sub(r"#ifdef VL2_EXPERIMENTAL.*?#endif /\* VL2_EXPERIMENTAL[^\n]*", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", product), name


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "videollama2_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+\S*(oracle|tests)\b", src, flags=re.M), f


def test_entry_points_refuse_bad_arguments_before_launching(lib):
    p = ctypes.c_void_p(4096)                                       # stand-in device pointers: every case fails its checks first

    def quant(k16=p, ks=p, nkv=2, smax=256, p0=0, p1=8, k8=p):
        return lib.vl2_kv_quant(k16, p, k8, p, ks, p, nkv, smax, p0, p1, None)

    for kw, rc, msg in [(dict(k16=None), -1, "bad args"), (dict(ks=None), -1, "bad args"), (dict(nkv=0), -1, "bad args"),
                        (dict(p0=8, p1=8), -2, "outside the cache"), (dict(p1=257), -2, "outside the cache"), (dict(p0=-1), -2, "outside the cache"),
                        (dict(k8=ctypes.c_void_p(4100)), -2, "16-byte aligned")]:
        assert quant(**kw) == rc, (kw, _err(lib))
        assert msg in _err(lib), (kw, _err(lib))

    def attn(ks=p, nh=8, nkv=2, smax=256, pos=3, pos_dev=None, cap=0, k8=p):
        return lib.vl2_attn_decode_kv8(p, k8, p, ks, p, p, p, p, p, nh, nkv, smax, pos, pos_dev, cap, 0.088, None)

    for kw, rc, msg in [(dict(ks=None), -1, "bad args"), (dict(nh=7), -2, "nh = nkv*group"), (dict(pos=256), -2, "outside the cache"),
                        (dict(pos=-1), -2, "outside the cache"), (dict(pos_dev=p, cap=257), -2, "outside the cache"),
                        (dict(pos_dev=p, cap=0), -2, "outside the cache"), (dict(k8=ctypes.c_void_p(4104)), -2, "16-byte aligned")]:
        assert attn(**kw) == rc, (kw, _err(lib))
        assert msg in _err(lib) and "vl2_attn_decode_kv8" in _err(lib), (kw, _err(lib))

    def battn(B=3, pos_dev=p, cap=256, nh=8, vs=p):
        return lib.vl2_attn_decode_kv8_batched(p, p, p, p, vs, p, p, p, p, B, 1536, 65536, 512, 1024, nh, 2, 256, pos_dev, cap, 0.088, None)

    for kw, rc, msg in [(dict(pos_dev=None), -1, "bad args"), (dict(B=0), -1, "bad args"), (dict(vs=None), -1, "bad args"),
                        (dict(nh=9), -2, "nh = nkv*group"), (dict(cap=300), -2, "outside the cache")]:
        assert battn(**kw) == rc, (kw, _err(lib))
        assert msg in _err(lib) and "vl2_attn_decode_kv8_batched" in _err(lib), (kw, _err(lib))


# ---------------------------------------------------------------------------------------------------------------- refusals
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


def _no_kv8_kernels(monkeypatch):
    """Any kv8 call fails the test: the refusals below must come before the first kernel call."""
    from videollama2_amd import ops

    def boom(*a, **k):
        raise AssertionError("a kv8 kernel was called")
    for name in ("kv_quant", "attn_decode_kv8", "attn_decode_kv8_batched"):
        monkeypatch.setattr(ops, name, boom)


def test_extend_and_prefix_reuse_refuse_on_the_fp8_kv_cache(golden_small, monkeypatch):
    from tests.emu.backend import emulated_backend
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.model import VideoLLaMA2Hip
    cfg = golden_small["cfg"]
    with emulated_backend():
        dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, golden_small["seed"], only=_keep), "cpu", max_seq_len=32)
        assert dec.fp8_kv is False and dec.kv8 is None                      # never the default
        dec.pos = 5
        epoch = dec.cache_epoch
        dec.graph = object()
        assert dec.enable_fp8_kv() is dec and dec.fp8_kv is True
        assert dec.pos == 0 and dec.cache_epoch == epoch + 1 and dec.graph is None
        k8, v8, ks, vs = dec.kv8[0]
        assert len(dec.kv8) == dec.n_layers and k8.dtype == torch.uint8 and k8.shape == (1, 32, 128) and v8.shape == k8.shape
        assert ks.dtype == torch.float32 and ks.shape == (1, 32) and vs.shape == ks.shape
        _no_kv8_kernels(monkeypatch)
        x = torch.zeros(3, dec.D, dtype=torch.bfloat16)
        with pytest.raises(NotImplementedError, match="fp8 KV cache is on.*enable_fp8_kv\\(False\\)"):
            dec.extend(x)
        with pytest.raises(NotImplementedError, match="fp8 KV cache is on"):
            dec.generate(x, start_pos=0)
        m = VideoLLaMA2Hip.__new__(VideoLLaMA2Hip)
        torch.nn.Module.__init__(m)
        m.decoder = dec
        with pytest.raises(NotImplementedError, match="fp8 KV cache is on"):
            m.generate(torch.tensor([[1, 2, 3]]), prefix_cache=True)
        # the slots: fp8 only, plus one sequence's 16-bit staging cache
        bb = dec._ensure_batch(3)
        assert "k" not in bb and "v" not in bb and bb["kv8"][0][0].shape == (3, 1, 32, 128) and bb["stage"][0][0].shape == (1, 32, 128)
        dec.enable_fp8_kv(False)
        assert dec.fp8_kv is False and dec.cache_epoch == epoch + 2 and dec._bb is None and dec.kv8 is None     # freed with the switch
        assert "k" in dec._ensure_batch(3)


def test_mixtral_and_tensor_parallel_decoders_refuse(golden_small, monkeypatch):
    import torch.distributed as dist
    from tests.emu.backend import emulated_backend
    from videollama2_amd.decoder import HipMistralDecoder, HipMixtralDecoder
    _no_kv8_kernels(monkeypatch)
    with pytest.raises(NotImplementedError, match="mixtral.*fp8 KV cache"):
        HipMixtralDecoder.enable_fp8_kv(object.__new__(HipMixtralDecoder))
    cfg = golden_small["cfg"]
    sd = O.seeded_state_dict(cfg, golden_small["seed"], only=_keep)
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        with emulated_backend():
            dec = HipMistralDecoder(cfg, sd, "cpu", max_seq_len=16, tp_group=dist.group.WORLD)
            with pytest.raises(NotImplementedError, match="single-rank decoders only"):
                dec.enable_fp8_kv()
            assert dec.fp8_kv is False and dec.kv8 is None
            one = HipMistralDecoder(cfg, sd, "cpu", max_seq_len=16)
            one.tp_always_reduce = True
            with pytest.raises(NotImplementedError, match="single-rank decoders only"):
                one.enable_fp8_kv()
            one.tp_always_reduce = False
            one.hd = 64
            with pytest.raises(NotImplementedError, match="head_dim 128 only"):
                one.enable_fp8_kv()
    finally:
        dist.destroy_process_group()


def test_switch_is_refused_while_a_batcher_holds_requests(golden_small):
    from tests.emu.backend import emulated_backend
    from videollama2_amd.decoder import HipMistralDecoder
    cfg = golden_small["cfg"]
    with emulated_backend():
        dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, golden_small["seed"], only=_keep), "cpu", max_seq_len=16)

        class Busy:
            def in_flight(self):
                return 2
        dec._bb_busy = Busy()
        with pytest.raises(RuntimeError, match="requests in flight"):
            dec.enable_fp8_kv()
        assert dec.fp8_kv is False


def test_idle_batcher_follows_reallocated_slots_and_a_busy_one_still_refuses(golden_small):
    """16-bit path, no fp8 KV: a batcher with no occupied slot goes on in the slot buffers a larger generate_batch() (or the fp8-KV switch)
    allocated; one that holds a request keeps refusing, as before."""
    from tests.emu.backend import emulated_backend
    from videollama2_amd.decoder import HipMistralDecoder
    from videollama2_amd.serving import ContinuousBatcher
    cfg = golden_small["cfg"]
    with emulated_backend(), torch.no_grad():
        dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, golden_small["seed"], only=_keep), "cpu", max_seq_len=24)
        x = golden_small["inputs_embeds"][:6].bfloat16()
        solo = dec.generate(x, max_new_tokens=3)[0].tolist()
        b = ContinuousBatcher(dec, max_slots=2, use_graph=False)
        first = b.bb
        dec._ensure_batch(3)                                   # what a generate_batch() of three requests does
        assert dec._bb is not first
        rid = b.submit(x, max_new_tokens=3)
        b.step()                                               # idle when the step began: adopts the new buffers, then admits
        assert b.bb is dec._bb and b.slots[0] is not None
        dec._bb = dict(b.bb)                                   # ... and now other buffers under a request in flight
        with pytest.raises(RuntimeError, match="reallocated while requests were in flight"):
            b.step()
        dec._bb = b.bb                                         # (put the buffers back: the request's rows are still in them)
        assert b.run()[rid].tolist() == solo
