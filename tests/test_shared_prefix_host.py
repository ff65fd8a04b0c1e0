"""Batched decode over a shared prompt prefix, host side only (no launch): the declarations of the entry points against the ctypes table,
the argument refusals of the Python wrapper and of the library (before anything is enqueued), the decoder's and the model's refusals with
their reasons, the host-side common-prefix split, own_cap rounding and the live-slice count."""
import ctypes
import os
import re

import pytest
import torch

from oracle import vl2_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


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


def test_header_declarations_match_the_ctypes_table(lib):
    from videollama2_amd import _lib
    assert set(_lib.SHARED_PREFIX_SIGNATURES) == {"vl2_attn_decode_shared"}
    ret, args = _declared("vl2_attn_decode_shared")
    assert ret is ctypes.c_int32 and args == _lib.SHARED_PREFIX_SIGNATURES["vl2_attn_decode_shared"]
    assert lib.vl2_attn_decode_shared.argtypes == args
    ret, args = _declared("vl2_attn_decode_shared_partial_floats")
    assert ret is ctypes.c_int64 and args == [ctypes.c_int32] * 3
    assert lib.vl2_attn_decode_shared_partial_floats.restype is ctypes.c_int64 and lib.vl2_attn_decode_shared_partial_floats.argtypes == args
    for name in ("vl2_attn_decode_shared", "vl2_attn_decode_shared_partial_floats"):
        assert name in _lib.EXPORTS and name not in _lib.SIGNATURES            # the emulator's symbol set is unchanged
        for path in (_lib.LIB_PATH, _lib.LIB_PATHS["fp16"], _lib.LAB_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    assert lib.vl2_version() == 7


def test_library_refuses_bad_arguments_before_launching(lib):
    p = ctypes.c_void_p(4096)                                       # stand-in device pointers: every case fails its checks first

    def call(qkv=p, kown=p, pos_dev=p, B=3, nh=8, nkv=2, P=100, psmax=256, own_cap=64, rope=256, partial_floats=1 << 30, qkv_bs=1536, own_bs=2 * 64 * 128):
        return lib.vl2_attn_decode_shared(qkv, p, p, kown, p, p, p, p, partial_floats, p, B, qkv_bs, own_bs, 1024, nh, nkv, P, psmax, own_cap, rope,
                                          pos_dev, 0.088, None)

    for kw, rc, msg in [(dict(qkv=None), -1, "bad args"), (dict(pos_dev=None), -1, "bad args"), (dict(B=0), -1, "bad args"),
                        (dict(nh=7), -2, "nh = nkv*group"), (dict(P=0), -2, "outside the prefix cache"), (dict(P=257), -2, "outside the prefix cache"),
                        (dict(psmax=1 << 23, P=100), -2, "2 GiB"), (dict(own_cap=0), -2, "multiple of 64"), (dict(own_cap=100), -2, "multiple of 64"),
                        (dict(P=200, rope=256), -2, "cos/sin tables"), (dict(qkv_bs=1000), -2, "16-byte alignment"),
                        (dict(own_bs=64 * 128), -2, "16-byte alignment"), (dict(kown=ctypes.c_void_p(4100)), -2, "16-byte alignment"),
                        (dict(partial_floats=3 * 8 * 2 * 130 - 1), -2, "partial of")]:
        assert call(**kw) == rc, (kw, lib.vl2_last_error_string().decode())
        err = lib.vl2_last_error_string().decode()
        assert msg in err and "vl2_attn_decode_shared" in err, (kw, err)
    assert lib.vl2_attn_decode_shared_partial_floats(0, 64, 8) == 0 and lib.vl2_attn_decode_shared_partial_floats(100, 100, 8) == 0


def test_wrapper_refuses_before_the_library_is_touched(monkeypatch):
    from videollama2_amd import _lib, ops

    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "load", boom)
    bf = torch.bfloat16
    nh, nkv, P, cap = 8, 2, 65, 64
    good = dict(qkv=torch.zeros(2, 12 * 128, dtype=bf), kprefix=torch.zeros(nkv, 128, 128, dtype=bf), vprefix=torch.zeros(nkv, 128, 128, dtype=bf),
                kown=torch.zeros(2, nkv, cap, 128, dtype=bf), vown=torch.zeros(2, nkv, cap, 128, dtype=bf), cos_t=torch.zeros(256, 64),
                sin_t=torch.zeros(256, 64), partial=torch.zeros(2 * ops.shared_partial_floats(P, cap, nh)), out=torch.zeros(2, nh * 128, dtype=bf),
                nh=nh, nkv=nkv, P=P, pos_dev=torch.zeros(2, dtype=torch.int32), scale=0.088)
    cases = [(dict(nh=7), "nh = nkv \\* group"), (dict(qkv=good["qkv"][:, :-128]), "qkv must be"), (dict(P=0), "outside the prefix cache"),
             (dict(P=129), "outside the prefix cache"), (dict(kprefix=good["kprefix"][:, ::2]), "prefix caches must be contiguous"),
             (dict(kown=good["kown"][:1], vown=good["vown"][:1]), "private caches must be"),
             (dict(kown=torch.zeros(2, nkv, 100, 128, dtype=bf), vown=torch.zeros(2, nkv, 100, 128, dtype=bf)), "multiple of 64"),
             (dict(cos_t=torch.zeros(100, 64), sin_t=torch.zeros(100, 64)), "cos / sin tables"), (dict(pos_dev=torch.zeros(1, dtype=torch.int32)), "positions"),
             (dict(partial=good["partial"][:-1]), "partial holds"), ({}, "must be a device tensor")]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            ops.attn_decode_shared(**{**good, **kw})


# ---------------------------------------------------------------------------------------------------------------- formulas
def test_own_cap_rounding():
    from videollama2_amd.ops import shared_own_cap
    assert [shared_own_cap(n, m) for n, m in ((1, 1), (17, 8), (17, 47), (17, 48), (60, 4), (62, 2), (62, 3), (100, 2048))] == \
        [64, 64, 64, 128, 64, 64, 128, 2176]


@pytest.mark.parametrize("P", [1, 63, 64, 65, 128, 129, 200, 1621, 3071, 3073, 4096, 20000])
def test_prefix_splits_and_live_slices_against_a_brute_force_count(P, lib):
    from videollama2_amd import ops
    # the rule, restated: the fewest whole 64-key tiles per split (at least two) that need at most 24 splits
    tiles = -(-P // 64)
    tps = next(t for t in range(2, tiles + 3) if -(-tiles // t) <= 24)
    chunk = tps * 64
    splits = sum(1 for k0 in range(0, P, chunk))
    assert ops.shared_prefix_splits(P) == splits <= 24
    for own_cap in (64, 192):
        assert ops.shared_partial_floats(P, own_cap, 8) == lib.vl2_attn_decode_shared_partial_floats(P, own_cap, 8) == 8 * (splits + own_cap // 64) * 130
    for own in (0, 1, 62, 63, 64, 65, 127, 128, 191):
        ctx = own + 1                                               # own rows the step attends to, the new one included
        live = splits + sum(1 for k0 in range(0, 192, 64) if k0 < ctx)
        assert ops.shared_live_slices(P, P + own) == live


# ---------------------------------------------------------------------------------------------------------------- the common prefix
def test_common_prefix_split():
    from videollama2_amd.model import common_prefix_tokens as cpt
    sent = {-200, -201}
    eq = lambda a, b: a == b
    vid, vid2, vid_longer = ("v", 4), ("w", 4), ("v", 8)
    base = [1, 5, 6, -201, 7, 8]
    # identical prompts: every request keeps one token of its own
    assert cpt([base, base, base], [[vid]] * 3, sent, eq) == len(base) - 1
    # one video, different questions: the prefix runs through the sentinel and the shared text after it
    assert cpt([base + [9], base + [10, 11], base + [12]], [[vid]] * 3, sent, eq) == len(base)
    assert cpt([base + [9], base[:4] + [30, 31]], [[vid]] * 2, sent, eq) == 4
    # no common prefix
    assert cpt([[1, 5], [2, 5]], [[], []], sent, eq) == 0
    # different videos, or one whose frames merely begin with the other's: cut BEFORE the sentinel
    assert cpt([base + [9], base + [10]], [[vid], [vid2]], sent, eq) == 3
    assert cpt([base + [9], base + [10]], [[vid], [vid_longer]], sent, eq) == 3
    # a sentinel without media on one side is not shared either; a second sentinel with other media stops the prefix there
    assert cpt([base + [9], base + [10]], [[vid], []], sent, eq) == 3
    two = [1, -201, 4, -201, 5, 6]
    assert cpt([two, two[:5] + [7]], [[vid, vid2], [vid, vid]], sent, eq) == 3
    # a one-token request leaves nothing to share
    assert cpt([[1], [1, 2]], [[], []], sent, eq) == 0


def test_common_prefix_split_with_the_models_media_comparator():
    """The comparator generate_shared passes in (modal, dtype, shape and contents): an equal copy of the video is shared, another modal,
    other contents or a video whose frames merely begin with the first one's cut the prefix before the sentinel."""
    from videollama2_amd.model import VideoLLaMA2Hip, common_prefix_tokens as cpt
    sent, eq = {-200, -201}, VideoLLaMA2Hip._media_equal
    a = torch.arange(24.).view(2, 3, 2, 2)
    ids = [[1, 5, -201, 7, 9], [1, 5, -201, 7, 10]]
    assert cpt(ids, [[(a, "video")], [(a.clone(), "video")]], sent, eq) == 4
    for other in ((a, "image"), (a + 1, "video"), (torch.cat([a, a]), "video"), (a.double(), "video")):
        assert cpt(ids, [[(a, "video")], [other]], sent, eq) == 2


# ---------------------------------------------------------------------------------------------------------------- refusals
def _keep(n):
    return n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))


def _no_kernels(monkeypatch):
    """Any kernel call fails the test: the refusals must come before the first one."""
    from videollama2_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a kernel was called")
    monkeypatch.setattr(_lib, "call", boom)


def test_decoder_and_model_refusals_come_with_their_reasons_before_any_kernel(golden_small, monkeypatch):
    import torch.distributed as dist
    from tests.emu.backend import emulated_backend
    from videollama2_amd.decoder import HipMistralDecoder, HipMixtralDecoder
    from videollama2_amd.model import VideoLLaMA2Hip
    cfg = golden_small["cfg"]
    sd = O.seeded_state_dict(cfg, golden_small["seed"], only=_keep)
    x = torch.zeros(3, cfg["llm"]["hidden_size"], dtype=torch.bfloat16)
    with emulated_backend():
        dec = HipMistralDecoder(cfg, sd, "cpu", max_seq_len=32)
        dec.enable_fp8_kv()
        _no_kernels(monkeypatch)
        call = lambda d: d.generate_batch([x, x], max_new_tokens=2, shared_prefix=x)
        with pytest.raises(NotImplementedError, match="shared-prefix decode: the fp8 KV cache is on.*enable_fp8_kv\\(False\\)"):
            call(dec)
        # the model-level entry refuses before the encoder runs
        m = VideoLLaMA2Hip.__new__(VideoLLaMA2Hip)
        torch.nn.Module.__init__(m)
        m.decoder = dec
        reqs = [(torch.tensor([1, 5, 6, 7]), None), (torch.tensor([1, 5, 6, 8]), None)]
        with pytest.raises(NotImplementedError, match="shared-prefix decode: the fp8 KV cache is on"):
            m.generate_shared(reqs, max_new_tokens=2)
        dec._fp8_kv = False
        dec.prefill_fp8 = True
        with pytest.raises(NotImplementedError, match="shared-prefix decode: .*extend.*enable_fp8_prefill\\(False\\)"):
            call(dec)
        dec.prefill_fp8 = False
        dec.tp_always_reduce = True
        with pytest.raises(NotImplementedError, match="shared-prefix decode: single-rank decoders only"):
            call(dec)
        dec.tp_always_reduce = False
        dec.hd = 64
        with pytest.raises(NotImplementedError, match="shared-prefix decode: head_dim 128 only \\(this decoder has 64\\)"):
            call(dec)
        dec.hd = 128
        with pytest.raises(ValueError, match="suffix of at least one row"):
            dec.generate_batch([x, x[:0]], shared_prefix=x)
        with pytest.raises(ValueError, match="exceeds the KV cache"):
            dec.generate_batch([torch.zeros(30, x.shape[1])], shared_prefix=x)
        with pytest.raises(NotImplementedError, match="mixtral.*shared-prefix decode is not built"):
            HipMixtralDecoder.generate_batch(object.__new__(HipMixtralDecoder), [x], shared_prefix=x)
        with pytest.raises(NotImplementedError, match="batched decoding not built"):
            HipMixtralDecoder.generate_batch(object.__new__(HipMixtralDecoder), [x])
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        with emulated_backend():
            tp = HipMistralDecoder(cfg, sd, "cpu", max_seq_len=16, tp_group=dist.group.WORLD)
            with pytest.raises(NotImplementedError, match="shared-prefix decode: single-rank decoders only"):
                tp.generate_batch([x], shared_prefix=x)
    finally:
        dist.destroy_process_group()


def test_model_falls_back_to_the_plain_path_without_a_common_prefix(monkeypatch):
    """A common prefix of length 0, or requests whose visual inputs differ (a modal tag is left in a suffix), are not merged:
    generate_shared hands the requests to generate_batch unchanged."""
    from videollama2_amd.model import VideoLLaMA2Hip
    m = VideoLLaMA2Hip.__new__(VideoLLaMA2Hip)
    torch.nn.Module.__init__(m)
    seen = []
    monkeypatch.setattr(VideoLLaMA2Hip, "generate_batch", lambda self, requests, **kw: seen.append((requests, kw)) or "plain")
    a, b = torch.zeros(2, 3, 4, 4), torch.ones(2, 3, 4, 4)
    no_prefix = [(torch.tensor([1, 5]), None), (torch.tensor([2, 5]), None)]
    assert m.generate_shared(no_prefix, max_new_tokens=3) == "plain" and seen[-1] == (no_prefix, dict(max_new_tokens=3))
    other_video = [(torch.tensor([[1, 5, -201, 7]]), [(a, "video")]), (torch.tensor([[1, 5, -201, 8]]), [(b, "video")])]
    assert m.generate_shared(other_video) == "plain" and seen[-1][0] is other_video
