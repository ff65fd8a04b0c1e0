"""MXFP4 expert weights on the Mixtral decoder, host side: the exports, the switch and what stays refused, the argument
checks of the new entry points (before any launch), the exactness of the inputs tests/test_gpu_moe_mxfp4.py runs and the decidability of its
decoder prompts.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

from tests import moe_mxfp4_exact as X4
from tests import moe_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vl2_moe_gemv_mxfp4", "vl2_moe_gemv_batched_mxfp4", "vl2_moe_gemm_skinny_mxfp4")


def _bare():
    from videollama2_amd.decoder import HipMixtralDecoder
    mix = object.__new__(HipMixtralDecoder)
    mix.w = dict(layers=[])                  # (no layer: the switch has nothing to quantise)
    return mix


def _lib_built():
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib
    return _lib, _lib.load()


def test_header_exports_and_signatures_agree():
    _lib, lib = _lib_built()
    assert lib.vl2_version() == 7
    header = open(os.path.join(ROOT, "include", "vl2hip.h")).read()
    assert tuple(_lib.MOE_MXFP4_SIGNATURES) == NAMES
    for name in NAMES:
        assert name in _lib.EXPORTS and name not in _lib.SIGNATURES and name not in _lib.MOE_BATCH_SIGNATURES      # the emulator's symbol set is unchanged
        assert name not in _lib.MOE_FP8_SIGNATURES and name not in _lib.MXFP4_SIGNATURES
        assert hasattr(lib, name)
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        sig = _lib.MOE_MXFP4_SIGNATURES[name]
        assert len(params) == len(sig), (name, len(params), len(sig))
        for p, c in zip(params, sig):
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_float if p.startswith("float") else ctypes.c_int32
            assert c is want, (name, p, c)
    # the 16-bit namesakes' argument lists with q / q_stride / ldq / scale / s_stride / lds in place of W / w_stride / ldw
    six = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32]
    for name, base in (("vl2_moe_gemv_mxfp4", _lib.MOE_SIGNATURES["vl2_moe_gemv"]), ("vl2_moe_gemv_batched_mxfp4", _lib.MOE_BATCH_SIGNATURES["vl2_moe_gemv_batched"])):
        assert _lib.MOE_MXFP4_SIGNATURES[name] == six + base[3:]
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert [p.split()[-1].lstrip("*") for p in m.group(1).split(",")][:6] == ["q", "q_stride", "ldq", "scale", "s_stride", "lds"]
    base = _lib.MOE_BATCH_SIGNATURES["vl2_moe_gemm_skinny"]
    assert _lib.MOE_MXFP4_SIGNATURES["vl2_moe_gemm_skinny_mxfp4"] == base[:4] + six + base[7:]


def _refusals(mix):
    """Every refusal of the Mixtral decoder that holds whatever the MXFP4 switch says (a fresh list: batched decoding is off here)."""
    x = torch.zeros(4, 256)
    return [(lambda: mix.enable_fp8_decode(), "MoE \\(mixtral\\) decoder: fp8 weights not built"),
            (lambda: mix.enable_fp8_decode(False), "MoE \\(mixtral\\) decoder: fp8 weights not built"),
            (lambda: mix.enable_fp8_prefill(), "MoE \\(mixtral\\) decoder: fp8 weights not built"),
            (lambda: mix.enable_mxfp4_decode(), "MoE \\(mixtral\\) decoder: MXFP4 weights not built"),
            (lambda: mix.enable_mxfp4_decode(False), "MoE \\(mixtral\\) decoder: MXFP4 weights not built"),
            (lambda: mix.enable_fp8_kv(), "MoE \\(mixtral\\) decoder: the fp8 KV cache is not built for it \\(its step runs the MoE GEMVs on the 16-bit "
                                          "cache\\): keep the 16-bit cache"),
            (lambda: mix.enable_paged_kv(8), "MoE \\(mixtral\\) decoder: the paged KV cache is not built for it \\(its batched decoding is not\\): keep the "
                                             "contiguous cache"),
            (lambda: mix.enable_paged_kv(8, fp8=True), "MoE \\(mixtral\\) decoder: the paged KV cache is not built for it"),
            (lambda: mix.prefill_batch([], [], None), "MoE \\(mixtral\\) decoder: batched prefill not built"),
            (lambda: mix.generate_batch([x]), "MoE \\(mixtral\\) decoder: batched decoding not built"),
            (lambda: mix._ensure_batch(2), "MoE \\(mixtral\\) decoder: batched / continuous decoding not built"),
            (lambda: mix.prefill(x, cache=([], [])), "MoE \\(mixtral\\) decoder: external caches \\(batched decoding\\) not built"),
            (lambda: mix.generate_batch([x], shared_prefix=x), "MoE \\(mixtral\\) decoder: shared-prefix decode is not built \\(its batched decoding is not\\)"),
            (lambda: mix._shared_prefix_refusals(paged_ok=True), "MoE \\(mixtral\\) decoder: shared-prefix decode is not built")]


def test_switch_is_off_by_default_and_every_refusal_keeps_its_text():
    mix = _bare()
    assert mix.moe_mxfp4 is False and not hasattr(mix, "w4moe")
    for fn, text in _refusals(mix):
        with pytest.raises(NotImplementedError, match=text):
            fn()
    mix.decode_fp8 = mix.decode_mxfp4 = False
    assert mix.enable_moe_mxfp4() is mix and mix.moe_mxfp4 is True and mix.w4moe == [] and mix.moe_fp8 is False
    assert mix.decode_format == "16bit"
    for fn, text in _refusals(mix):
        with pytest.raises(NotImplementedError, match=text):
            fn()
    mix.enable_moe_mxfp4(False)
    assert mix.moe_mxfp4 is False and mix.decode_format == "16bit"
    for fn, text in _refusals(mix):
        with pytest.raises(NotImplementedError, match=text):
            fn()


def test_the_fp8_and_the_mxfp4_switch_refuse_each_other():
    mix = _bare().enable_moe_mxfp4()
    for kw in ({}, dict(tiled=True)):
        with pytest.raises(ValueError, match="MXFP4 expert weights are on: call enable_moe_mxfp4\\(False\\) before enable_moe_fp8\\(\\)"):
            mix.enable_moe_fp8(**kw)
    assert mix.moe_mxfp4 is True and mix.moe_fp8 is False and not hasattr(mix, "w8moe")
    mix.enable_moe_fp8(False)                                      # switching the other OFF is never refused
    assert mix.enable_moe_mxfp4(False).enable_moe_fp8().moe_fp8 is True      # ... and with MXFP4 off fp8 switches on
    mix = _bare().enable_moe_fp8()
    with pytest.raises(ValueError, match="fp8 expert weights are on: call enable_moe_fp8\\(False\\) before enable_moe_mxfp4\\(\\)"):
        mix.enable_moe_mxfp4()
    assert mix.moe_fp8 is True and mix.moe_mxfp4 is False and not hasattr(mix, "w4moe")
    mix.enable_moe_mxfp4(False)
    assert mix.enable_moe_fp8(False).enable_moe_mxfp4().moe_mxfp4 is True


def test_toggling_drops_the_graphs_bumps_the_epoch_and_is_refused_with_requests_in_flight():
    mix = _bare()
    mix.cache_epoch = 3
    for on in (True, False):
        mix._batch_graphs, mix.graph, mix._graph_sample = {(4, False): object()}, object(), (object(), object())
        mix.enable_moe_mxfp4(on)
        assert mix._batch_graphs == {} and mix.graph is None and mix._graph_sample == (None, None)
    assert mix.cache_epoch == 5
    copies = mix.w4moe
    assert mix.enable_moe_mxfp4().w4moe is copies                # the copies are made once

    class Busy:
        n = 2

        def in_flight(self):
            return self.n
    mix._bb_busy = Busy()
    for on in (False, True):
        with pytest.raises(RuntimeError, match="enable_moe_mxfp4: a ContinuousBatcher holds requests in flight"):
            mix.enable_moe_mxfp4(on)
    assert mix.moe_mxfp4 is True and mix.cache_epoch == 6
    mix._bb_busy.n = 0
    assert mix.enable_moe_mxfp4(False).moe_mxfp4 is False


def test_more_than_64_slots_are_refused_with_the_limit_in_the_message():
    mix = _bare().enable_moe_batch().enable_moe_mxfp4()
    for B in (65, 70, 128):
        with pytest.raises(NotImplementedError, match="at most 64 sequences.*no tiled W4A16 grouped GEMM is built"):
            mix._ensure_batch(B)
    mix._bb = dict(B=128, moe={})                                  # slots of a 16-bit batch left over: still refused
    with pytest.raises(NotImplementedError, match="at most 64 sequences"):
        mix._ensure_batch(100)
    assert mix._ensure_batch(64)["B"] == 128                       # (64 and fewer reach the slot buffers)
    assert mix.MOE_MXFP4_ROWS == 64 and mix.MOE_FP8_ROWS == 64 and mix.MOE_GEMM_BATCH == 5 and mix.MOE_SKINNY_ROWS == 0      # the other regimes are untouched
    with pytest.raises(NotImplementedError, match="at most 64 sequences.*no tiled W4A16 grouped GEMM is built"):
        mix._token_block_batched_mxfp4(None, None, None, None, 65, None, None, None)       # a step of more than 64 rows
    mix.enable_moe_mxfp4(False)
    assert mix._ensure_batch(100)["B"] == 128


def test_model_switch_passes_through_and_a_dense_decoder_refuses():
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.decoder import HipMistralDecoder
    model = object.__new__(VideoLLaMA2Hip)
    model.__dict__["decoder"] = _bare()
    assert model.enable_moe_mxfp4() is model and model.decoder.moe_mxfp4 is True
    model.enable_moe_mxfp4(False)
    assert model.decoder.moe_mxfp4 is False
    model.__dict__["decoder"] = object.__new__(HipMistralDecoder)
    with pytest.raises(NotImplementedError, match="enable_moe_mxfp4: the decoder is dense"):
        model.enable_moe_mxfp4()


def test_entry_points_refuse_what_the_kernels_cannot_take_before_launching():
    """Every check runs before every launch, so the pointers are never read and no GPU is needed."""
    _lib, lib = _lib_built()
    p = ctypes.c_void_p(4096)
    err = lambda: lib.vl2_last_error_string()
    N, K, I, S, k, E = 1024, 256, 512, 4, 2, 8
    # ---- vl2_moe_gemv_mxfp4(q, q_stride, ldq, scale, s_stride, lds, x, ids, wts, res, y, E, k, N, K, eps, flags, stream)
    names = ["q", "q_stride", "ldq", "scale", "s_stride", "lds", "x", "ids", "wts", "res", "y", "E", "k", "N", "K", "eps", "flags", "stream"]
    gu = [p, N * K // 2, K // 2, p, N * K // 32, K // 32, p, p, None, None, p, E, k, N, K, 1e-5, 1, None]
    dn = [p, K * I // 2, I // 2, p, K * I // 32, I // 32, p, p, p, p, p, E, k, K, I, 1e-5, 0, None]

    def solo(base, **over):
        a = list(base)
        for key, v in over.items():
            a[names.index(key)] = v
        return lib.vl2_moe_gemv_mxfp4(*a)
    assert solo(gu, q=None) == -1 and b"vl2_moe_gemv_mxfp4: null q" in err()
    assert solo(gu, scale=None) == -1 and b"vl2_moe_gemv_mxfp4: null scale" in err()
    assert solo(gu, ids=None) == -1 and solo(gu, x=None) == -1 and solo(gu, y=None) == -1
    assert solo(gu, N=1023) == -2 and b"N%64==0" in err()
    assert solo(gu, N=992) == -2 and b"vl2_moe_gemv_mxfp4: SWIGLU needs N%64==0" in err()
    assert solo(gu, K=240) == -2 and b"K%32==0" in err()
    assert solo(gu, K=32736, ldq=16368, lds=1023, q_stride=N * 16368, s_stride=N * 1023) == -2 and b"K<=32704" in err()
    assert solo(dn, K=32736, ldq=16368, lds=1023, q_stride=K * 16368, s_stride=K * 1023, k=1) == -2 and b"K<=32704" in err()
    assert solo(gu, ldq=K // 2 - 16) == -2 and solo(gu, ldq=K // 2 + 8, q_stride=N * (K // 2 + 8)) == -2 and solo(gu, lds=K // 32 - 1) == -2
    assert solo(gu, q_stride=N * K // 2 - 16) == -2 and solo(gu, q_stride=N * K // 2 + 8) == -2 and solo(gu, s_stride=N * K // 32 - 1) == -2
    assert b"q_stride >= N*ldq" in err()
    assert solo(gu, q=ctypes.c_void_p(4104)) == -2 and solo(gu, x=ctypes.c_void_p(4104)) == -2
    assert solo(gu, wts=p) == -2 and solo(gu, res=p) == -2
    assert solo(gu, E=65) == -3 and solo(gu, k=5) == -3 and solo(gu, E=1) == -3 and solo(gu, flags=3) == -3 and b"flags other than" in err()
    assert solo(dn, wts=None) == -1 and b"routing weights" in err()
    KR = X4.DOWN4_K_REFUSED
    assert solo(dn, k=4, K=KR, ldq=KR // 2, lds=KR // 32, q_stride=K * KR // 2, s_stride=K * KR // 32) == -2 and b"vl2_moe_gemv_mxfp4: k * K * 2 bytes of activations must fit the LDS" in err()
    # ---- vl2_moe_gemv_batched_mxfp4(q, q_stride, ldq, scale, s_stride, lds, x, ldx, ids, wts, res, ldres, y, ldy, S, E, k, N, K, eps, flags, stream)
    bnames = ["q", "q_stride", "ldq", "scale", "s_stride", "lds", "x", "ldx", "ids", "wts", "res", "ldres", "y", "ldy", "S", "E", "k", "N", "K", "eps",
              "flags", "stream"]
    bgu = [p, N * K // 2, K // 2, p, N * K // 32, K // 32, p, K, p, None, None, 0, p, N // 2, S, E, k, N, K, 1e-5, 1, None]
    bdn = [p, K * I // 2, I // 2, p, K * I // 32, I // 32, p, I, p, p, p, K, p, K, S, E, k, K, I, 1e-5, 0, None]

    def rows(base, **over):
        a = list(base)
        for key, v in over.items():
            a[bnames.index(key)] = v
        return lib.vl2_moe_gemv_batched_mxfp4(*a)
    assert rows(bgu, q=None) == -1 and b"vl2_moe_gemv_batched_mxfp4: null q" in err() and rows(bgu, scale=None) == -1
    assert rows(bgu, ldx=K - 8) == -2 and rows(bgu, ldy=N // 2 - 8) == -2 and rows(bgu, S=0) == -1 and rows(bgu, S=65536) == -2
    assert rows(bgu, N=992) == -2 and b"N%64==0" in err()
    assert rows(bgu, K=240) == -2 and b"vl2_moe_gemv_batched_mxfp4: need K%32==0" in err()
    assert rows(bgu, wts=p) == -2 and rows(bgu, res=p) == -2 and rows(bgu, flags=2) == -3 and rows(bgu, E=65) == -3 and rows(bgu, k=5) == -3
    assert rows(bgu, lds=K // 32 - 1) == -2 and rows(bgu, s_stride=N * K // 32 - 1) == -2 and rows(bgu, q_stride=N * K // 2 - 16) == -2
    assert rows(bdn, wts=None) == -1 and b"routing weights" in err()
    assert rows(bdn, ldx=I + 16) == -2 and b"without a gap" in err()
    assert rows(bdn, ldy=K - 8) == -2 and rows(bdn, ldres=K - 8) == -2
    assert rows(bdn, k=4, K=KR, ldq=KR // 2, lds=KR // 32, ldx=KR, q_stride=K * KR // 2, s_stride=K * KR // 32) == -2 and b"fit the LDS" in err()
    # ---- vl2_moe_gemm_skinny_mxfp4(A, lda, a_rows, rowmap, q, q_stride, ldq, scale, s_stride, lds, C, ldc, counts, offs, S, k, E, N, K, flags, part, part_bytes, stream)
    need = lib.vl2_moe_gemm_skinny_part_bytes(8, k, N, K)
    snames = ["A", "lda", "a_rows", "rowmap", "q", "q_stride", "ldq", "scale", "s_stride", "lds", "C", "ldc", "counts", "offs", "S", "k", "E", "N", "K",
              "flags", "part", "part_bytes", "stream"]
    good = [p, K, 8, p, p, N * K // 2, K // 2, p, N * K // 32, K // 32, p, N // 2, p, p, 8, k, E, N, K, 1, p, need, None]

    def skinny(**over):
        a = list(good)
        for key, v in over.items():
            a[snames.index(key)] = v
        return lib.vl2_moe_gemm_skinny_mxfp4(*a)
    assert skinny(S=65, a_rows=65) == -2 and b"S<=64 (no tiled W4A16 grouped GEMM is built)" in err()
    assert skinny(N=1000) == -2 and b"N%64==0" in err()
    assert skinny(N=960, q_stride=960 * K // 2, s_stride=960 * K // 32) == -2 and b"N%128==0 with SWIGLU" in err()
    assert skinny(K=240) == -2 and b"K%32==0" in err()
    assert skinny(K=32736, lda=32736, ldq=16368, lds=1023, q_stride=N * 16368, s_stride=N * 1023) == -2 and b"K<=32704" in err()
    assert skinny(part_bytes=need - 4) == -1 and b"partial buffer too small" in err()
    assert skinny(part=None) == -1 and skinny(counts=None) == -1 and skinny(offs=None) == -1
    assert skinny(q=None) == -1 and b"vl2_moe_gemm_skinny_mxfp4: null q" in err() and skinny(scale=None) == -1 and b"null scale" in err()
    assert skinny(E=65) == -3 and skinny(k=5) == -3 and skinny(flags=2) == -3
    assert skinny(lda=K - 8) == -2 and skinny(ldq=K // 2 - 16) == -2 and skinny(lds=K // 32 - 1) == -2 and skinny(q_stride=N * K // 2 - 16) == -2
    assert skinny(s_stride=N * K // 32 - 1) == -2 and skinny(q_stride=N * K // 2 + 8) == -2
    assert skinny(ldc=N // 2 - 4) == -2
    assert skinny(a_rows=7) == -2 and b"A has 7 rows, need 8" in err()


# ---------------------------------------------------------------------------------------------------------------- the reference alone
def test_every_exact_case_survives_the_oracles_quantiser_and_holds_its_bound():
    """g * 2^p with a 4 or a 6 in every non-zero block: the oracle's block exponent is p and nothing rounds.  Asserted for EVERY case the GPU
    test runs (none dropped), on tests/mxfp4_oracle.py alone, together with the exactness bound: the sum of |products| in units of the smallest
    one is below 2^24 (Down4Case asserts it at construction; restated here)."""
    rows = X4.down4_table()
    assert len(rows) >= 40
    assert {r.k for r in rows} == {1, 2, 3, 4} and {r.N for r in rows} == set(X4.DOWN4_N) == {1, 3, 4, 5, 41}
    assert {r.S for r in rows if r.batched} == {1, 2, 5} and {r.S for r in rows if not r.batched} == {1}
    assert {r.K for r in rows} == set(X4.DOWN4_K) | {X4.DOWN4_K_LDS} and {r.res for r in rows} == {True, False}
    assert X4.DOWN4_K[:3] == (32, 288, 2080) and X4.DOWN4_K[3:] == (64 * X4.DOWN4_DEPTH * 32, 64 * X4.DOWN4_DEPTH * 32 + 32)
    assert 4 * X4.DOWN4_K_LDS * 2 == 160 * 1024 and X4.DOWN4_K_REFUSED == X4.DOWN4_K_LDS + 32
    for kk in (1, 2, 3, 4):
        assert {(r.K, r.res) for r in rows if r.k == kk and not r.batched} >= {(K, res) for K in (2080, X4.DOWN4_K[4]) for res in (True, False)}
    depth = re.search(r"constexpr int MOE_MX4_DOWN_DEPTH = (\d+);", open(os.path.join(ROOT, "videollama2_amd", "csrc", "k_moe_mxfp4.h")).read())
    assert depth and int(depth.group(1)) == X4.DOWN4_DEPTH         # the pass edge follows the kernel's depth
    zero_block = zero_row = False
    for r in rows:
        c = X4.Down4Case(r)
        assert X4.survives(c.wi), c.coords()
        assert c.isum < 2.0 ** 24 and c.bound < 2.0 ** 24, c.coords()
        blk = c.wi.view(c.E, c.N, -1, 32)
        p = torch.floor(torch.log2(blk.abs().amax(3).clamp(min=2.0 ** -40))) - 2
        assert len(set(p[blk.abs().amax(3) > 0].tolist())) == 3, c.coords()      # the block exponents vary
        zero_block |= bool((blk.abs().amax(3) == 0).any())
        zero_row |= bool((c.wi.abs().amax(2) == 0).any())
    assert zero_block and zero_row
    c = X4.Down4Case.order_case4()
    assert X4.survives(c.wi)
    for (E, k, N, K) in X4.GU4_CASES:
        for S, batched in ((1, False), (X4.GU4_ROWS_S, True)):
            c = X4.GateUp4Case(S, E, k, N, K, batched)
            assert X4.survives(c.wi), (E, k, N, K, S)
            assert c.bound() < 2.0 ** 24, (E, k, N, K, S)
            assert 0 in c.ids[0].tolist() or k == 1
            assert E - 1 in c.ids[0].tolist()
    assert {c[0] for c in X4.GU4_CASES} == {4, 64} and {c[1] for c in X4.GU4_CASES} == {1, 2, 4} and {c[2] for c in X4.GU4_CASES} == {64, 192}
    assert {c[3] for c in X4.GU4_CASES} == {32, 2080, 4096, 4128, 16384, 16416}
    for name, (nb, counts) in X4.SKINNY4_CASES.items():
        assert sum(counts) == 2 * nb and max(counts) <= nb, name
    assert {c for _, cs in X4.SKINNY4_CASES.values() for c in cs} >= {0, 1, 16, 17, 33, 64}
    assert X4.survives(X4.skinny4_stack(8, 1024, 256, 1)) and X4.survives(X4.skinny4_stack(8, 256, 512, 2))
    # a block without a 4 or a 6 does NOT survive when a value falls off the grid at the block's exponent: the check can fail
    bad = torch.zeros((1, 2, 32), dtype=torch.float64)
    bad[0, :, 0], bad[0, :, 1] = 3.0, 0.125
    assert not X4.survives(bad)
    bad[0, :, 0] = 5.0
    assert not X4.survives(bad)


def test_the_order_case_through_the_exactly_rounded_chain():
    c = X4.Down4Case.order_case4()
    d, w = c.dots[0, :, 0].tolist(), c.wts[0].tolist()
    assert torch.tensor(X4.fma_chain(w, d, None)).bfloat16().item() == 1.0078125
    assert torch.tensor(X4.fma_chain(w[::-1], d[::-1], None)).bfloat16().item() == 1.0


def test_the_decoder_prompts_leave_at_least_half_of_the_pairs_decidable():
    """The criterion of the GPU decoder tests, on the CPU alone: the fp32 oracle on the state dict whose expert weights are their dequantised
    MXFP4 copies, free-running greedy, routing margin >= 1e-2 on every layer.  A request counts its leading decidable steps (the GPU test stops
    at the first step below the bar); every request's first decode step is decidable, and at least half of all (request, step >= 1) pairs are."""
    cfg = MO.small_mixtral_cfg(n_layers=2)
    sd = MO.seeded_state_dict(cfg, seed=X4.DEC_SEED, router_scale=4.0)
    sd4 = X4.dequantised_state_dict(sd, cfg)
    for name in ("model.layers.0.mlp.experts.gate_up_proj", "model.layers.1.mlp.experts.down_proj"):
        r = float((sd4[name] - sd[name]).norm() / sd[name].norm())
        assert 0.02 < r < 0.2, (name, r)                                 # (4-bit copies: close to, not equal to, the weights)
    assert len({X4.dec_prompt(i).shape[0] for i in range(64)}) == 40 and X4.dec_prompt(0).shape == (1, 256)
    for ids, what in ((X4.DEC8_IDS, "8 requests"), (X4.DEC64_CHECK, "64 requests"), (X4.DEC8_IDS[:4], "the dequantised 16-bit comparison")):
        pairs = [X4.decidable_pairs(X4.oracle_free_margins(sd4, cfg, X4.dec_prompt(i).float(), X4.DEC_NEW)[1]) for i in ids]
        print(what, "decidable leading steps per request:", pairs)
        assert 2 * sum(pairs) >= len(ids) * (X4.DEC_NEW - 1), (what, pairs)
    for i in X4.DEC64_CHECK:                                             # the stated slack of the chosen six, on both sets of experts
        for d in (sd, sd4):
            assert min(X4.oracle_free_margins(d, cfg, X4.dec_prompt(i).float(), X4.DEC_NEW)[1]) >= 2e-2, i
