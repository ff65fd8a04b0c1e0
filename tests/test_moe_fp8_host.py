"""fp8 expert weights on the Mixtral decoder, host side: the exports, the switch and what stays refused, the argument
checks of the new entry points (before any launch) and the exactness of the inputs tests/test_gpu_moe_fp8.py runs.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

from tests import moe_exact as X
from tests import moe_fp8_exact as X8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vl2_moe_gemv_fp8", "vl2_moe_gemv_batched_fp8", "vl2_moe_gemm_skinny_fp8")


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
    assert tuple(_lib.MOE_FP8_SIGNATURES) == NAMES
    for name in NAMES:
        assert name in _lib.EXPORTS and name not in _lib.SIGNATURES and name not in _lib.MOE_BATCH_SIGNATURES      # the emulator's symbol set is unchanged
        assert hasattr(lib, name)
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        sig = _lib.MOE_FP8_SIGNATURES[name]
        assert len(params) == len(sig), (name, len(params), len(sig))
        for p, c in zip(params, sig):
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_float if p.startswith("float") else ctypes.c_int32
            assert c is want, (name, p, c)
    # the 16-bit namesakes' argument lists with q / q_stride / ldq / scale / s_stride in place of W / w_stride / ldw
    for name, base in (("vl2_moe_gemv_fp8", _lib.MOE_SIGNATURES["vl2_moe_gemv"]), ("vl2_moe_gemv_batched_fp8", _lib.MOE_BATCH_SIGNATURES["vl2_moe_gemv_batched"])):
        assert _lib.MOE_FP8_SIGNATURES[name] == base[:3] + [ctypes.c_void_p, ctypes.c_int64] + base[3:]
    base = _lib.MOE_BATCH_SIGNATURES["vl2_moe_gemm_skinny"]
    assert _lib.MOE_FP8_SIGNATURES["vl2_moe_gemm_skinny_fp8"] == base[:7] + [ctypes.c_void_p, ctypes.c_int64] + base[7:]


def _refusals(mix):
    """Every refusal of the Mixtral decoder that holds whatever the fp8 switch says (a fresh list: batched decoding is off here)."""
    x = torch.zeros(4, 256)
    return [(lambda: mix.enable_fp8_decode(), "MoE \\(mixtral\\) decoder: fp8 weights not built"),
            (lambda: mix.enable_fp8_decode(False), "MoE \\(mixtral\\) decoder: fp8 weights not built"),
            (lambda: mix.enable_fp8_prefill(), "MoE \\(mixtral\\) decoder: fp8 weights not built"),
            (lambda: mix.enable_mxfp4_decode(), "MoE \\(mixtral\\) decoder: MXFP4 weights not built"),
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
    from videollama2_amd.decoder import HipMixtralDecoder
    mix = _bare()
    assert mix.moe_fp8 is False and not hasattr(mix, "w8moe")
    for fn, text in _refusals(mix):
        with pytest.raises(NotImplementedError, match=text):
            fn()
    mix.decode_fp8 = mix.decode_mxfp4 = False
    assert mix.enable_moe_fp8() is mix and mix.moe_fp8 is True and mix.w8moe == []
    assert mix.decode_format == "16bit"
    for fn, text in _refusals(mix):
        with pytest.raises(NotImplementedError, match=text):
            fn()
    mix.enable_moe_fp8(False)
    assert mix.moe_fp8 is False and mix.decode_format == "16bit"
    for fn, text in _refusals(mix):
        with pytest.raises(NotImplementedError, match=text):
            fn()
    from tests import moe_oracle as MO
    for kw in (dict(tp_shard=(0, 2)), dict(tp_group=object()), dict(tp_local=object())):
        with pytest.raises(NotImplementedError, match="MoE \\(mixtral\\) decoder: tensor / expert parallelism not built"):
            HipMixtralDecoder(MO.small_mixtral_cfg(n_layers=1), {}, "cpu", **kw)


def test_toggling_drops_the_graphs_bumps_the_epoch_and_is_refused_with_requests_in_flight():
    mix = _bare()
    mix.cache_epoch = 3
    for on in (True, False):
        mix._batch_graphs, mix.graph, mix._graph_sample = {(4, False): object()}, object(), (object(), object())
        mix.enable_moe_fp8(on)
        assert mix._batch_graphs == {} and mix.graph is None and mix._graph_sample == (None, None)
    assert mix.cache_epoch == 5
    copies = mix.w8moe
    assert mix.enable_moe_fp8().w8moe is copies                  # the copies are made once

    class Busy:
        n = 2

        def in_flight(self):
            return self.n
    mix._bb_busy = Busy()
    for on in (False, True):
        with pytest.raises(RuntimeError, match="enable_moe_fp8: a ContinuousBatcher holds requests in flight"):
            mix.enable_moe_fp8(on)
    assert mix.moe_fp8 is True and mix.cache_epoch == 6
    mix._bb_busy.n = 0
    assert mix.enable_moe_fp8(False).moe_fp8 is False


def test_more_than_64_slots_are_refused_with_the_limit_in_the_message():
    mix = _bare().enable_moe_batch().enable_moe_fp8()
    for B in (65, 70, 128):
        with pytest.raises(NotImplementedError, match="at most 64 sequences"):
            mix._ensure_batch(B)
    mix._bb = dict(B=128, moe={})                                  # slots of a 16-bit batch left over: still refused
    with pytest.raises(NotImplementedError, match="at most 64 sequences"):
        mix._ensure_batch(100)
    assert mix._ensure_batch(64)["B"] == 128                       # (64 and fewer reach the slot buffers)
    assert mix.MOE_FP8_ROWS == 64 and mix.MOE_GEMM_BATCH == 5 and mix.MOE_SKINNY_ROWS == 0      # the 16-bit regimes are untouched
    mix.enable_moe_fp8(False)
    assert mix._ensure_batch(100)["B"] == 128


def test_model_switch_passes_through_and_a_dense_decoder_refuses():
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.decoder import HipMistralDecoder
    model = object.__new__(VideoLLaMA2Hip)
    model.__dict__["decoder"] = _bare()
    assert model.enable_moe_fp8() is model and model.decoder.moe_fp8 is True
    model.enable_moe_fp8(False)
    assert model.decoder.moe_fp8 is False
    model.__dict__["decoder"] = object.__new__(HipMistralDecoder)
    with pytest.raises(NotImplementedError, match="enable_moe_fp8: the decoder is dense"):
        model.enable_moe_fp8()


def test_entry_points_refuse_what_the_kernels_cannot_take_before_launching():
    """Every check runs before every launch, so the pointers are never read and no GPU is needed."""
    _lib, lib = _lib_built()
    p = ctypes.c_void_p(4096)
    err = lambda: lib.vl2_last_error_string()
    N, K, I, S, k, E = 1024, 256, 512, 4, 2, 8
    # ---- vl2_moe_gemv_fp8(q, q_stride, ldq, scale, s_stride, x, ids, wts, res, y, E, k, N, K, eps, flags, stream)
    names = ["q", "q_stride", "ldq", "scale", "s_stride", "x", "ids", "wts", "res", "y", "E", "k", "N", "K", "eps", "flags", "stream"]
    gu = [p, N * K, K, p, N, p, p, None, None, p, E, k, N, K, 1e-5, 1, None]
    dn = [p, K * I, I, p, K, p, p, p, p, p, E, k, K, I, 1e-5, 0, None]

    def solo(base, **over):
        a = list(base)
        for key, v in over.items():
            a[names.index(key)] = v
        return lib.vl2_moe_gemv_fp8(*a)
    assert solo(gu, q=None) == -1 and b"null q" in err()
    assert solo(gu, scale=None) == -1 and b"null scale" in err()
    assert solo(gu, ids=None) == -1
    assert solo(gu, N=1023) == -2 and b"N even" in err()
    assert solo(gu, N=1022) == -2 and b"N%64==0" in err()
    assert solo(gu, K=248) == -2 and b"K%16==0" in err()
    assert solo(gu, K=32720, ldq=32720, q_stride=N * 32720) == -2 and b"K<=32704" in err()
    assert solo(dn, K=32720, ldq=32720, q_stride=K * 32720, k=1) == -2 and b"K<=32704" in err()
    assert solo(gu, ldq=K - 16) == -2 and solo(gu, q_stride=N * K - 16) == -2 and solo(gu, s_stride=N - 1) == -2
    assert solo(gu, wts=p) == -2 and solo(gu, res=p) == -2
    assert solo(gu, E=65) == -3 and solo(gu, k=5) == -3 and solo(gu, flags=3) == -3
    assert solo(dn, wts=None) == -1 and b"routing weights" in err()
    assert solo(dn, k=4, K=X8.DOWN8_K_REFUSED, ldq=X8.DOWN8_K_REFUSED, q_stride=K * X8.DOWN8_K_REFUSED) == -2 and b"fit the LDS" in err()
    # ---- vl2_moe_gemv_batched_fp8(q, q_stride, ldq, scale, s_stride, x, ldx, ids, wts, res, ldres, y, ldy, S, E, k, N, K, eps, flags, stream)
    bnames = ["q", "q_stride", "ldq", "scale", "s_stride", "x", "ldx", "ids", "wts", "res", "ldres", "y", "ldy", "S", "E", "k", "N", "K", "eps", "flags", "stream"]
    bgu = [p, N * K, K, p, N, p, K, p, None, None, 0, p, N // 2, S, E, k, N, K, 1e-5, 1, None]
    bdn = [p, K * I, I, p, K, p, I, p, p, p, K, p, K, S, E, k, K, I, 1e-5, 0, None]

    def rows(base, **over):
        a = list(base)
        for key, v in over.items():
            a[bnames.index(key)] = v
        return lib.vl2_moe_gemv_batched_fp8(*a)
    assert rows(bgu, ldx=K - 8) == -2 and rows(bgu, ldy=N // 2 - 8) == -2 and rows(bgu, S=0) == -1 and rows(bgu, S=65536) == -2
    assert rows(bgu, N=1023) == -2 and b"N even" in err()
    assert rows(bgu, K=248) == -2 and b"K%16==0" in err()
    assert rows(bdn, ldx=I + 16) == -2 and b"without a gap" in err()
    assert rows(bdn, ldy=K - 8) == -2 and rows(bdn, ldres=K - 8) == -2
    assert rows(bdn, k=4, K=X8.DOWN8_K_REFUSED, ldq=X8.DOWN8_K_REFUSED, ldx=X8.DOWN8_K_REFUSED, q_stride=K * X8.DOWN8_K_REFUSED) == -2 and b"fit the LDS" in err()
    # ---- vl2_moe_gemm_skinny_fp8(A, lda, a_rows, rowmap, q, q_stride, ldq, scale, s_stride, C, ldc, counts, offs, S, k, E, N, K, flags, part, part_bytes, stream)
    need = lib.vl2_moe_gemm_skinny_part_bytes(8, k, N, K)
    snames = ["A", "lda", "a_rows", "rowmap", "q", "q_stride", "ldq", "scale", "s_stride", "C", "ldc", "counts", "offs", "S", "k", "E", "N", "K", "flags",
              "part", "part_bytes", "stream"]
    good = [p, K, 8, p, p, N * K, K, p, N, p, N // 2, p, p, 8, k, E, N, K, 1, p, need, None]

    def skinny(**over):
        a = list(good)
        for key, v in over.items():
            a[snames.index(key)] = v
        return lib.vl2_moe_gemm_skinny_fp8(*a)
    assert skinny(S=65, a_rows=65) == -2 and b"S<=64" in err()
    assert skinny(N=1000) == -2 and b"N%64==0" in err()
    assert skinny(N=960, q_stride=960 * K, s_stride=960) == -2 and b"N%128==0 with SWIGLU" in err()
    assert skinny(K=240) == -2 and b"K%32==0" in err()
    assert skinny(K=32736, lda=32736, ldq=32736, q_stride=N * 32736) == -2 and b"K<=32704" in err()
    assert skinny(part_bytes=need - 4) == -1 and b"partial buffer too small" in err()
    assert skinny(part=None) == -1 and skinny(q=None) == -1 and skinny(scale=None) == -1 and skinny(counts=None) == -1 and skinny(offs=None) == -1
    assert skinny(E=65) == -3 and skinny(k=5) == -3 and skinny(flags=2) == -3
    assert skinny(lda=K - 8) == -2 and skinny(ldq=K - 16) == -2 and skinny(q_stride=N * K - 16) == -2 and skinny(s_stride=N - 1) == -2
    assert skinny(ldc=N // 2 - 4) == -2
    assert skinny(a_rows=7) == -2 and b"A has 7 rows, need 8" in err()


# ---------------------------------------------------------------------------------------------------------------- the reference alone
def test_every_exact_case_survives_the_oracles_quantiser():
    """Integers in [-15, 15] have at most 4 significant bits; under the row-scale rule they become q = w 2^s, s >= 4, exact in e4m3fn whatever
    power of two multiplies the row.  Asserted for EVERY case the GPU test runs (none dropped), on oracle/fp8_oracle.py alone."""
    rows = X8.down8_table()
    assert len(rows) >= 40
    assert {r.k for r in rows} == {1, 2, 3, 4} and {r.N for r in rows} == set(X8.DOWN8_N) and {r.S for r in rows if r.batched} == {1, 2, 5}
    assert {r.K for r in rows} == set(X8.DOWN8_K) | {X8.DOWN8_K_LDS} and {r.res for r in rows} == {True, False}
    assert 4 * X8.DOWN8_K_LDS * 2 == 160 * 1024 and X8.DOWN8_K_REFUSED == X8.DOWN8_K_LDS + 16
    for r in rows:
        c = X8.Down8Case(r)
        assert X8.survives(c.wi), c.coords()
        q = X8.quant_ints(c.wi)
        assert bool((q == q.round()).all()) and float(q.abs().max()) <= 448, c.coords()
        # q = w 2^s with s >= 4: the quantised row is a multiple of 16 (a zero row aside)
        assert bool((q % 16 == 0).all()), c.coords()
    c = X8.Down8Case.order_case8()
    assert X8.survives(c.wi)
    for (E, k, N, K) in X8.GU8_CASES:
        for S, batched in ((1, False), (X8.GU8_ROWS_S, True)):
            assert X8.survives(X8.GateUp8Case(S, E, k, N, K, batched).wi), (E, k, N, K, S)
    assert {c[0] for c in X8.GU8_CASES} == {4, 64} and {c[1] for c in X8.GU8_CASES} == {1, 2, 4} and {c[2] for c in X8.GU8_CASES} == {64, 192}
    assert {c[3] for c in X8.GU8_CASES} == {16, 1040, 4096, 4112, 8192, 8208}
    for name, (nb, counts) in X8.SKINNY8_CASES.items():
        assert sum(counts) == 2 * nb and max(counts) <= nb, name
    assert {c for _, cs in X8.SKINNY8_CASES.values() for c in cs} >= {0, 1, 16, 17, 33, 64}
    assert X8.survives(X8.skinny8_stack(8, 1024, 256, 1)) and X8.survives(X8.skinny8_stack(8, 256, 512, 2))
    # a value with 5 significant bits does NOT survive: the check can fail
    bad = torch.full((1, 2, 16), 17.0, dtype=torch.float64)
    assert not X8.survives(bad)


def test_the_exact_rounding_helper_against_known_answers():
    from fractions import Fraction
    assert X8.round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == 1                                   # a tie: to even
    assert X8.round_f32(Fraction(1) + Fraction(3, 2 ** 24)) == Fraction(1) + Fraction(2, 2 ** 23)  # a tie: to even, upwards
    assert X8.round_f32(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 40)) == Fraction(1) + Fraction(1, 2 ** 23)
    assert X8.round_f32(Fraction(-3, 7)) == Fraction(float(torch.tensor(-3.0 / 7.0, dtype=torch.float64).float()))
    g = torch.Generator().manual_seed(1)
    for v in (torch.randn(200, generator=g, dtype=torch.float64) * 1e3).tolist():
        assert float(X8.round_f32(Fraction(v))) == float(torch.tensor(v, dtype=torch.float64).float())
    # the order case through the chain: slot order gives 1.0078125 after the bf16 store, the reverse order 1.0
    c = X8.Down8Case.order_case8()
    d, w = c.dots[0, :, 0].tolist(), c.wts[0].tolist()
    assert torch.tensor(X8.fma_chain(w, d, None)).bfloat16().item() == 1.0078125
    assert torch.tensor(X8.fma_chain(w[::-1], d[::-1], None)).bfloat16().item() == 1.0
