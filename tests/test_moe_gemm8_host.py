"""The tiled W8A16 grouped GEMM on the fp8 expert stacks, host side: the export and its signature table, every refusal of
vl2_moe_gemm_fp8 (before any launch), the exactness of every input tests/test_gpu_moe_gemm8.py runs, and the decoder's `tiled` keyword -- what it
admits, what it leaves exactly as it was, and the regime chosen per batch size.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

from tests import decode_exact as D
from tests import moe_exact as X
from tests import moe_fp8_exact as X8
from tests import moe_gemm8_exact as M
from tests.test_moe_fp8_host import _bare, _lib_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vl2_moe_gemm_fp8"


def test_header_exports_and_the_signature_table_agree_and_mirror_the_16_bit_entry():
    _lib, lib = _lib_built()
    assert lib.vl2_version() == 7
    assert tuple(_lib.MOE_FP8_TILED_SIGNATURES) == (NAME,)
    assert tuple(_lib.MOE_FP8_SIGNATURES) == ("vl2_moe_gemv_fp8", "vl2_moe_gemv_batched_fp8", "vl2_moe_gemm_skinny_fp8")      # unchanged
    assert NAME in _lib.EXPORTS and hasattr(lib, NAME)
    for table in (_lib.SIGNATURES, _lib.MOE_SIGNATURES, _lib.MOE_BATCH_SIGNATURES, _lib.FP8_BATCH_SIGNATURES, _lib.MOE_FP8_SIGNATURES):
        assert NAME not in table                                                                # the emulator's symbol set is unchanged
    sig = _lib.MOE_FP8_TILED_SIGNATURES[NAME]
    assert getattr(lib, NAME).argtypes == sig and getattr(lib, NAME).restype is ctypes.c_int32
    header = open(os.path.join(ROOT, "include", "vl2hip.h")).read()
    m = re.search(r"int32_t\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header)
    assert m
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == len(sig)
    for p, c in zip(params, sig):
        want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if p.startswith("int64_t") else ctypes.c_float if p.startswith("float") else ctypes.c_int32
        assert c is want, (p, c)
    base = _lib.MOE_SIGNATURES["vl2_moe_gemm"]
    assert sig == base[:5] + [ctypes.c_void_p, ctypes.c_int64] + base[5:]
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["A", "lda", "q", "q_stride", "ldq", "scale", "s_stride", "C", "ldc", "row_norm", "eps", "counts", "offs", "S", "k", "E", "P", "N",
                     "K", "flags", "stream"]
    src = open(os.path.join(ROOT, "videollama2_amd", "csrc", "k_moe_gemm8.h")).read()
    assert int(re.search(r"#define MOE8_STAGES (\d+)", src).group(1)) == M.RING
    assert {64 * (M.RING - 1), 64 * M.RING, 64 * (M.RING + 1)} <= set(M.K8_ALL)                  # at, one below and one above the ring's depth


def test_the_entry_refuses_what_the_kernel_cannot_take_before_launching():
    """Every check runs before the launch, so the pointers are never read and no GPU is needed."""
    _lib, lib = _lib_built()
    p = ctypes.c_void_p(4096)
    err = lambda: lib.vl2_last_error_string()
    N, K, S, k, E = 256, 192, 8, 2, 8
    P = X.moe_rows(S, k, E)
    names = ["A", "lda", "q", "q_stride", "ldq", "scale", "s_stride", "C", "ldc", "row_norm", "eps", "counts", "offs", "S", "k", "E", "P", "N", "K",
             "flags", "stream"]
    good = [p, K, p, N * K, K, p, N, p, N, None, 0.0, p, p, S, k, E, P, N, K, 0, None]

    def call(**over):
        a = list(good)
        for key, v in over.items():
            a[names.index(key)] = v
        return lib.vl2_moe_gemm_fp8(*a)

    def refused(code, **over):
        r = call(**over)
        assert r == code and NAME.encode() in err(), (over, r, err())
        return err()
    assert b"null q" in refused(-1, q=None) and b"null scale" in refused(-1, scale=None)
    for key in ("A", "C", "counts", "offs"):
        refused(-1, **{key: None})
    for key in ("S", "k", "E", "N", "K"):
        refused(-1, **{key: 0})
    refused(-3, E=65) and refused(-3, k=5) and refused(-3, k=3, E=2)
    assert b"N%128==0" in refused(-2, N=192, q_stride=192 * K, s_stride=192)
    assert b"K%64==0" in refused(-2, K=160, lda=160, ldq=160)
    refused(-2, lda=K - 8) and refused(-2, lda=K + 4) and refused(-2, ldc=N + 4)
    refused(-2, A=ctypes.c_void_p(4104)) and refused(-2, C=ctypes.c_void_p(4104)) and refused(-2, row_norm=ctypes.c_void_p(4100))
    # restated for bytes
    assert b"ldq%16==0" in refused(-2, ldq=K + 8)
    refused(-2, ldq=K - 16)
    refused(-2, q_stride=N * K + 8)
    refused(-2, q_stride=N * K - 16)
    refused(-2, q=ctypes.c_void_p(4104))
    assert b"scale rows" in refused(-2, scale=ctypes.c_void_p(4104))
    refused(-2, s_stride=N + 2) and refused(-2, s_stride=N - 4)
    assert b"must be a multiple of 128" in refused(-2, P=P - 128)
    refused(-2, P=P + 64)
    big = 1 << 24                                                         # 127 * 2^24 + K >= 2^30: the 32-bit buffer offsets
    assert b"32-bit buffer offsets" in refused(-2, ldq=big, q_stride=N * big)
    assert b"32-bit buffer offsets" in refused(-2, lda=big)
    assert b"flags other than VL2_GEMM_SWIGLU" in refused(-3, flags=2)
    refused(-3, flags=3)
    # the strided layout of the exact cases is accepted by every check: the call reaches the launch (not tried here: no device)
    assert (K + 16) % 16 == 0 and ((N + 1) * (K + 16)) % 16 == 0 and (N + 4) % 4 == 0


# ---------------------------------------------------------------------------------------------------------------- the reference alone
def test_every_case_survives_the_oracles_quantiser_and_passes_its_guard():
    rows = M.gemm8_table()
    assert len(rows) == 30
    for E in (2, 8, 64):
        rs = [r for r in rows if r.E == E and not r.shrink]
        assert {r.counts[0] for r in rs} == {r.counts[-1] for r in rs} == set(X.GEMM_COUNTS)
        if E > 2:
            assert {c for r in rs for c in r.counts[1:-1]} == set(X.GEMM_COUNTS)
    assert {r.N for r in rows} == {128, 256, 384} and {r.K for r in rows} == set(M.K8_ALL) and {r.epi for r in rows} == set(X.MOE_EPIS)
    assert {(r.N, r.epi) for r in rows if r.E == 8 and not r.shrink} == {(n, e) for n in (128, 256, 384) for e in X.MOE_EPIS}
    assert {r.epi for r in rows if r.shrink} == set(X.MOE_EPIS)
    grids, fit16 = set(), []
    for r in rows:
        c = M.Gemm8Case(r)                                                  # (its constructor asserts the guards)
        assert X8.survives(c.wi), c.coords()
        q = X8.quant_ints(c.wi)
        assert bool((q == q.round()).all()) and float(q.abs().max()) <= 448 and bool((q % 16 == 0).all()), c.coords()
        assert c.bound < 2.0 ** 24 and c.ibound < 2.0 ** 24
        assert c.S * c.k <= X.MOE_SCAN_MAX and c.P % X.MOE_BM == 0 and c.P >= c.S * c.k + c.E * (X.MOE_BM - 1) and int(c.offs[-1]) <= c.P
        # the poisoned storages: NaN bytes / NaN floats everywhere outside the views
        qs, ss = c.store["q"], c.store["scale"]
        assert bool((qs[:, c.N:] == 0x7F).all()) and bool((qs[:, :, c.K:] == 0x7F).all()) and bool(ss[:, c.N:].isnan().all())
        assert qs.stride(1) == c.K + 16 and qs.stride(0) == (c.N + 1) * (c.K + 16) and ss.stride(0) == c.N + 4
        # neighbouring rows, the gate / up pair and neighbouring experts carry different scales
        sc = ss[:, :c.N]
        lead = (c.wi / M.col_powers(c.E, c.N)[:, :, None]).abs().amax(2) == 15      # rows that hold a +-15: scale = 2^(n % 5 + e % 3 - 4)
        assert torch.equal(sc[lead], (M.col_powers(c.E, c.N) / 16.0).float()[lead])
        n = torch.arange(c.N - 32)
        both = lead[:, n] & lead[:, n + 32]
        assert bool((sc[:, n][both] != sc[:, n + 32][both]).all()) and bool(both.any())
        if r.E < 64:
            grids.add(c.grid % 8 == 0)
        fit16.append(M.fits_fp16(c))
    assert grids == {True, False}, "xcd_remap: workgroup counts that are and are not multiples of 8"
    assert sum(fit16) >= 8 and {r.epi for r, f in zip(rows, fit16) if f} == set(X.MOE_EPIS)
    bad = torch.full((1, 2, 64), 17.0, dtype=torch.float64)               # 5 significant bits do NOT survive: the check can fail
    assert not X8.survives(bad)


def test_the_reference_alone_stays_inside_the_swiglu_cap(capsys):
    """torch fp32 on the CPU against RNE of fp64: moe_exact._check_rows's cap, unchanged."""
    nd = tot = 0
    for r in M.gemm8_table():
        c = M.Gemm8Case(r)
        if not c.swiglu or not c.R:
            continue
        y32 = X._epilogue(c.acc.float(), c.rs_live, True, torch.float32)
        d = D.ulp_distance(y32.bfloat16(), c.ref.float().bfloat16())
        assert int(d.max()) <= 1 and int((d > 0).sum()) <= max(1, c.R * c.n_out // 100), c.coords()
        nd, tot = nd + int((d > 0).sum()), tot + d.numel()
    with capsys.disabled():
        print(f"\nreference alone (torch fp32 against fp64), SwiGLU of the fp8 table: {nd} of {tot} outputs one step off")


# ---------------------------------------------------------------------------------------------------------------- the decoder
def test_without_the_keyword_nothing_changes():
    mix = _bare().enable_moe_batch().enable_moe_fp8()
    assert mix.moe_fp8 is True and mix.moe_fp8_tiled is False
    assert mix.MOE_FP8_ROWS == 64 and mix.MOE_GEMM_BATCH == 5 and mix.MOE_SKINNY_ROWS == 0 and 5 <= mix.MOE_FP8_TILED_FROM <= 65
    for B in (65, 70, 128):
        with pytest.raises(NotImplementedError, match="at most 64 sequences, the grouped skinny-M GEMM's limit \\(no tiled W8A16 grouped GEMM is built\\)"):
            mix._ensure_batch(B)
    mix.k, mix.eps = 2, 1e-5
    with pytest.raises(NotImplementedError, match="a batched step takes at most 64 sequences, got 65"):
        mix._token_block_batched_fp8({}, {}, None, None, 65, {}, None, None)
    assert _bare().moe_fp8_tiled is False


def test_tiled_admits_more_than_64_slots():
    mix = _bare().enable_moe_batch().enable_moe_fp8(tiled=True)
    assert mix.moe_fp8 is True and mix.moe_fp8_tiled is True
    mix._bb = dict(B=128, moe={})
    for B in (65, 70, 128):
        assert mix._ensure_batch(B)["B"] == 128
    mix.enable_moe_fp8(tiled=False)
    assert mix.moe_fp8 is True and mix.moe_fp8_tiled is False
    with pytest.raises(NotImplementedError, match="at most 64 sequences"):
        mix._ensure_batch(65)
    assert mix.enable_moe_fp8(False, tiled=True).moe_fp8_tiled is False          # (tiled means nothing with the switch off)
    assert mix._ensure_batch(100)["B"] == 128


def test_toggling_tiled_drops_the_graphs_bumps_the_epoch_and_is_refused_while_busy():
    mix = _bare()
    mix.cache_epoch = 3
    for tiled in (True, False, True):
        mix._batch_graphs, mix.graph, mix._graph_sample = {(4, False): object()}, object(), (object(), object())
        assert mix.enable_moe_fp8(tiled=tiled) is mix and mix.moe_fp8_tiled is tiled
        assert mix._batch_graphs == {} and mix.graph is None and mix._graph_sample == (None, None)
    assert mix.cache_epoch == 6
    copies = mix.w8moe
    assert mix.enable_moe_fp8(tiled=False).w8moe is copies and mix.enable_moe_fp8(tiled=True).w8moe is copies      # the copies are made once

    class Busy:
        n = 2

        def in_flight(self):
            return self.n
    mix._bb_busy = Busy()
    for tiled in (False, True):
        with pytest.raises(RuntimeError, match="enable_moe_fp8: a ContinuousBatcher holds requests in flight"):
            mix.enable_moe_fp8(tiled=tiled)
    assert mix.moe_fp8_tiled is True and mix.cache_epoch == 8
    mix._bb_busy.n = 0
    assert mix.enable_moe_fp8(tiled=False).moe_fp8_tiled is False


def _recorded(monkeypatch, mix, nb):
    """The ops.moe_* calls of one fp8 batched block of nb rows, by name."""
    from videollama2_amd import decoder as dec
    calls = []

    def rec(name, ret=None):
        def f(*a, **kw):
            calls.append((name, kw))
            return ret() if callable(ret) else ret
        return f
    route = lambda: dict(xg="xg", rn="rn", ids="route_ids", wts="route_wts")
    for name in ("moe_route_rows", "moe_gemv_batched_fp8", "moe_gemm_skinny_fp8", "moe_gemm_fp8", "moe_combine", "moe_gemm", "moe_gemm_skinny", "moe_gemv_batched"):
        monkeypatch.setattr(dec.ops, name, rec(name, "t"))
    monkeypatch.setattr(dec.ops, "moe_route", rec("moe_route", route))
    monkeypatch.setattr(dec.ops, "rmsnorm", rec("rmsnorm", "h"))
    big = torch.zeros(4)
    m = dict(a=big, y=big, h=big, gather=big, inv=big, counts=big, offs=big, part=big)
    w8 = dict(wgu=("qgu", "sgu"), wd=("qd", "sd"))
    got = mix._token_block_batched_fp8(w8, dict(wr="wr"), "x", "x1", nb, m, "ids", "wts")
    return [n for n, _ in calls], calls, got


ROWS = ["moe_route_rows", "moe_gemv_batched_fp8", "moe_gemv_batched_fp8"]
SKINNY = ["moe_route_rows", "rmsnorm", "moe_gemm_skinny_fp8", "moe_gemm_skinny_fp8", "moe_combine"]
TILED = ["moe_route", "moe_gemm_fp8", "moe_gemm_fp8", "moe_combine"]


@pytest.mark.parametrize("tiled_from", (5, 65))
def test_the_regime_chosen_per_batch_size(monkeypatch, tiled_from):
    mix = _bare().enable_moe_batch().enable_moe_fp8(tiled=True)
    mix.k, mix.eps, mix.w["ones"] = 2, 1e-5, "ones"
    mix.MOE_FP8_TILED_FROM = tiled_from
    for nb in (1, 2, 4):
        assert _recorded(monkeypatch, mix, nb)[0] == ROWS, nb
    for nb in (5, 8, 33, 64):
        names, calls, got = _recorded(monkeypatch, mix, nb)
        assert names == (TILED if nb >= tiled_from else SKINNY), nb
        assert got == (("route_ids", "route_wts") if nb >= tiled_from else ("ids", "wts"))
    for nb in (65, 70, 128, 1000):                                        # any nb from MOE_FP8_TILED_FROM on
        names, calls, got = _recorded(monkeypatch, mix, nb)
        assert names == TILED and got == ("route_ids", "route_wts"), nb
        gu, dn = calls[1][1], calls[2][1]
        assert gu == dict(swiglu=True, row_norm="rn", eps=1e-5) and dn == {}
    # without the keyword the tiled form is never chosen, whatever the constant says
    mix.enable_moe_fp8(tiled=False)
    for nb in (5, 64):
        assert _recorded(monkeypatch, mix, nb)[0] == SKINNY
    with pytest.raises(NotImplementedError, match="at most 64 sequences, got 65"):
        _recorded(monkeypatch, mix, 65)


def test_the_tiled_block_hands_the_fp8_stacks_to_both_products(monkeypatch):
    from videollama2_amd import decoder as dec
    mix = _bare().enable_moe_batch().enable_moe_fp8(tiled=True)
    mix.k, mix.eps, mix.MOE_FP8_TILED_FROM = 2, 1e-5, 5
    seen = []
    monkeypatch.setattr(dec.ops, "moe_route", lambda x, wr, k, eps: seen.append(("route", x, wr, k)) or dict(xg="xg", rn="rn", ids="i", wts="w"))
    monkeypatch.setattr(dec.ops, "moe_gemm_fp8", lambda a, q, s, r, S, k, **kw: seen.append(("gemm", a, q, s, S, k)) or "a" + str(len(seen)))
    monkeypatch.setattr(dec.ops, "moe_combine", lambda x1, y, r, eps, out=None: seen.append(("combine", x1, y, out)))
    mix._token_block_batched_fp8(dict(wgu=("qgu", "sgu"), wd=("qd", "sd")), dict(wr="wr"), "x", "x1", 70, {}, None, None)
    assert seen == [("route", "x1", "wr", 2), ("gemm", "xg", "qgu", "sgu", 70, 2), ("gemm", "a2", "qd", "sd", 70, 2), ("combine", "x1", "a3", "x")]


def test_model_switch_passes_the_keyword_through_and_a_dense_decoder_refuses():
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.decoder import HipMistralDecoder
    model = object.__new__(VideoLLaMA2Hip)
    model.__dict__["decoder"] = _bare()
    assert model.enable_moe_fp8(tiled=True) is model and model.decoder.moe_fp8 is True and model.decoder.moe_fp8_tiled is True
    assert model.enable_moe_fp8().decoder.moe_fp8_tiled is False and model.decoder.moe_fp8 is True
    model.enable_moe_fp8(False)
    assert model.decoder.moe_fp8 is False
    model.__dict__["decoder"] = object.__new__(HipMistralDecoder)
    with pytest.raises(NotImplementedError, match="enable_moe_fp8: the decoder is dense"):
        model.enable_moe_fp8(tiled=True)
