"""The tiled W4A16 grouped GEMM on the MXFP4 expert stacks, host side: the export and its signature table, every refusal
of vl2_moe_gemm_mxfp4 (before any launch), the exactness of every input tests/test_gpu_moe_gemm4.py runs, and the decoder's `tiled` keyword --
what it admits, what it leaves exactly as it was, and the regime chosen per batch size.  No GPU needed."""
import ctypes
import os
import re

import pytest
import torch

from tests import decode_exact as D
from tests import moe_exact as X
from tests import moe_gemm4_exact as M
from tests import moe_mxfp4_exact as X4
from tests.test_moe_mxfp4_host import _bare, _lib_built

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vl2_moe_gemm_mxfp4"
ARGS = ["A", "lda", "q", "q_stride", "ldq", "scale", "s_stride", "lds", "C", "ldc", "row_norm", "eps", "counts", "offs", "S", "k", "E", "P", "N", "K",
        "flags", "stream"]


def test_header_exports_and_the_signature_table_agree_and_mirror_the_16_bit_entry():
    _lib, lib = _lib_built()
    assert lib.vl2_version() == 7
    assert tuple(_lib.MOE_MXFP4_TILED_SIGNATURES) == (NAME,)
    assert tuple(_lib.MOE_MXFP4_SIGNATURES) == ("vl2_moe_gemv_mxfp4", "vl2_moe_gemv_batched_mxfp4", "vl2_moe_gemm_skinny_mxfp4")      # unchanged
    assert tuple(_lib.MOE_FP8_SIGNATURES) == ("vl2_moe_gemv_fp8", "vl2_moe_gemv_batched_fp8", "vl2_moe_gemm_skinny_fp8")              # unchanged
    assert tuple(_lib.MOE_FP8_TILED_SIGNATURES) == ("vl2_moe_gemm_fp8",)                                                             # unchanged
    assert NAME in _lib.EXPORTS and hasattr(lib, NAME)
    for table in (_lib.SIGNATURES, _lib.MOE_SIGNATURES, _lib.MOE_BATCH_SIGNATURES, _lib.FP8_BATCH_SIGNATURES, _lib.MOE_FP8_SIGNATURES,
                  _lib.MOE_FP8_TILED_SIGNATURES, _lib.MOE_MXFP4_SIGNATURES, _lib.MXFP4_SIGNATURES):
        assert NAME not in table                                                                # the emulator's symbol set is unchanged
    sig = _lib.MOE_MXFP4_TILED_SIGNATURES[NAME]
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
    assert sig == base[:5] + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32] + base[5:]
    fp8 = _lib.MOE_FP8_TILED_SIGNATURES["vl2_moe_gemm_fp8"]
    assert sig == fp8[:7] + [ctypes.c_int32] + fp8[7:]                                          # vl2_moe_gemm_fp8's list with lds after s_stride
    assert [p.split()[-1].lstrip("*") for p in params] == ARGS
    src = open(os.path.join(ROOT, "videollama2_amd", "csrc", "k_moe_gemm4.h")).read()
    assert int(re.search(r"#define MOE4_STAGES (\d+)", src).group(1)) == M.RING
    stage = int(re.search(r"#define MOE4_STAGE_BYTES (\d+)", src).group(1))
    assert stage % 16 == 0 and M.RING * stage <= 160 * 1024 and stage >= 16384 + 4096 + 256
    assert {64 * (M.RING - 2), 64 * M.RING, 64 * (M.RING + 1), 64 * 17} <= set(M.K4_ALL) and 64 in M.K4_ALL      # below, at and above the ring's depth


def test_the_entry_refuses_what_the_kernel_cannot_take_before_launching():
    """Every check runs before the launch, so the pointers are never read and no GPU is needed."""
    _lib, lib = _lib_built()
    p = ctypes.c_void_p(4096)
    err = lambda: lib.vl2_last_error_string()
    N, K, S, k, E = 256, 192, 8, 2, 8
    P = X.moe_rows(S, k, E)
    good = [p, K, p, N * (K // 2), K // 2, p, N * (K // 32), K // 32, p, N, None, 0.0, p, p, S, k, E, P, N, K, 0, None]
    assert len(good) == len(ARGS)

    def call(**over):
        a = list(good)
        for key, v in over.items():
            a[ARGS.index(key)] = v
        return lib.vl2_moe_gemm_mxfp4(*a)

    def refused(code, **over):
        r = call(**over)
        assert r == code and NAME.encode() + b":" in err(), (over, r, err())
        return err()
    assert b"null q" in refused(-1, q=None) and b"null scale" in refused(-1, scale=None)
    for key in ("A", "C", "counts", "offs"):
        refused(-1, **{key: None})
    for key in ("S", "k", "E", "N", "K"):
        refused(-1, **{key: 0})
    refused(-3, E=65) and refused(-3, k=5) and refused(-3, k=3, E=2)
    assert b"N%128==0" in refused(-2, N=192, q_stride=192 * (K // 2), s_stride=192 * (K // 32))
    assert b"K%64==0" in refused(-2, K=160, lda=160, ldq=80, lds=5)
    assert b"K%64==0" in refused(-2, K=96, lda=96)                                  # K % 32 == 0 is not enough: a K-tile is two scale blocks
    refused(-2, lda=K - 8) and refused(-2, lda=K + 4) and refused(-2, ldc=N + 4)
    refused(-2, A=ctypes.c_void_p(4104)) and refused(-2, C=ctypes.c_void_p(4104)) and refused(-2, row_norm=ctypes.c_void_p(4100))
    # restated for codes and scale bytes
    assert b"ldq%16==0" in refused(-2, ldq=K // 2 + 8, q_stride=N * (K // 2 + 8))
    assert b"ldq >= K/2" in refused(-2, ldq=K // 2 - 16)
    assert b"lds >= K/32" in refused(-2, lds=K // 32 - 1)
    refused(-2, q_stride=N * (K // 2) + 8)
    refused(-2, q_stride=N * (K // 2) - 16)
    assert b"s_stride >= N*lds" in refused(-2, s_stride=N * (K // 32) - 1)
    refused(-2, q=ctypes.c_void_p(4104))
    assert b"must be a multiple of 128" in refused(-2, P=P - 128)
    refused(-2, P=P + 64)
    big = 1 << 24                                                         # 127 * 2^24 + ... >= 2^30: the 32-bit buffer offsets
    assert b"32-bit buffer offsets" in refused(-2, ldq=big, q_stride=N * big)
    assert b"32-bit buffer offsets" in refused(-2, lds=big, s_stride=N * big)
    assert b"32-bit buffer offsets" in refused(-2, lda=big)
    assert b"flags other than VL2_GEMM_SWIGLU" in refused(-3, flags=2)
    refused(-3, flags=3)
    # the strided layout of the exact cases passes every rule above: ldq = K / 2 + 16, and NO alignment rule for scale, lds or s_stride (odd
    # values of all three are what tests/moe_gemm4_exact.py lays out and tests/test_gpu_moe_gemm4.py launches)
    assert (K // 2 + 16) % 16 == 0 and ((N + 1) * (K // 2 + 16)) % 16 == 0 and (K // 32 + 3) % 2 == 1


# ---------------------------------------------------------------------------------------------------------------- the reference alone
def test_every_case_survives_the_oracles_quantiser_and_passes_its_guard():
    rows = M.gemm4_table()
    assert len(rows) == 30
    for E in (2, 8, 64):
        rs = [r for r in rows if r.E == E and not r.shrink]
        assert {r.counts[0] for r in rs} == {r.counts[-1] for r in rs} == set(X.GEMM_COUNTS)
        if E > 2:
            assert {c for r in rs for c in r.counts[1:-1]} == set(X.GEMM_COUNTS)
    assert {r.N for r in rows} == {128, 256, 384} and {r.K for r in rows} == set(M.K4_ALL) and {r.epi for r in rows} == set(X.MOE_EPIS)
    assert {(r.N, r.epi) for r in rows if r.E == 8 and not r.shrink} == {(n, e) for n in (128, 256, 384) for e in X.MOE_EPIS}
    assert {r.epi for r in rows if r.shrink} == set(X.MOE_EPIS)
    grids, fit16, worst = set(), [], 0.0
    for r in rows:
        c = M.Gemm4Case(r)                                                  # (its constructor asserts the guards)
        assert X4.survives(c.wi), c.coords()
        assert c.bound < 2.0 ** 24
        worst = max(worst, c.bound)
        assert c.S * c.k <= X.MOE_SCAN_MAX and c.P % X.MOE_BM == 0 and c.P >= c.S * c.k + c.E * (X.MOE_BM - 1) and int(c.offs[-1]) <= c.P
        # the rule: every value a normal half, every non-zero block holds a 4 or a 6 (times its power), one zero block and one zero row
        nz = c.wi[c.wi != 0].abs()
        assert float(nz.min()) >= 2.0 ** -14 and float(nz.max()) <= 24.0
        blocks = c.wi.view(c.E, c.N, c.K // 32, 32).abs()
        p = X4.block_powers(c.E, c.N, c.K).double()
        lead = blocks.amax(3) / torch.exp2(p)
        assert bool(((lead == 4) | (lead == 6) | (lead == 0)).all()) and bool((lead == 0).any())
        if c.K >= 64:
            assert bool((blocks[0, 0, -1] == 0).all())
        assert bool((c.wi[c.E - 1, 1] == 0).all())
        # the scale bytes ARE 127 + p where the block is not zero: p differs between the two blocks of a K-tile, neighbouring rows, the gate
        # and the up row of a SwiGLU pair and neighbouring experts
        qs, ss = c.store["q"], c.store["s"]
        sb = ss[:, :c.N, :c.K // 32]
        assert torch.equal(sb[lead != 0].long(), (127 + p.long())[lead != 0])
        assert bool((p[:, :, 0::2] != p[:, :, 1::2]).all()) and bool((p[:, 1:] != p[:, :-1]).all()) and bool((p[:, 32:] != p[:, :-32]).all())
        assert bool((p[1:] != p[:-1]).all())
        # the poisoned storages: non-zero codes / NaN scale bytes everywhere outside the views, odd scale strides
        assert bool((qs[:, c.N:] == 0x77).all()) and bool((qs[:, :, c.K // 2:] == 0x77).all())
        assert bool((ss[:, c.N:] == 0xFF).all()) and bool((ss[:, :, c.K // 32:] == 0xFF).all())
        assert qs.stride(1) == c.K // 2 + 16 and qs.stride(0) == (c.N + 1) * (c.K // 2 + 16)
        assert ss.stride(1) == c.K // 32 + 3 and ss.stride(0) == (c.N + 1) * (c.K // 32 + 3)
        if r.E < 64:
            grids.add(c.grid % 8 == 0)
        fit16.append(M.fits_fp16(c))
    assert grids == {True, False}, "xcd_remap: workgroup counts that are and are not multiples of 8"
    assert sum(fit16) >= 8 and {r.epi for r, f in zip(rows, fit16) if f} == set(X.MOE_EPIS)
    assert worst < 2.0 ** 24
    bad = torch.full((1, 2, 64), 5.0, dtype=torch.float64)                # 5 is not on the grid at exponent 0: the check can fail
    assert not X4.survives(bad)


def test_the_reference_alone_stays_inside_the_swiglu_cap(capsys):
    """torch fp32 on the CPU against RNE of fp64: moe_exact._check_rows's cap, unchanged.  Measured: 22 of 3753600 outputs one step off."""
    nd = tot = 0
    for r in M.gemm4_table():
        c = M.Gemm4Case(r)
        if not c.swiglu or not c.R:
            continue
        y32 = X._epilogue(c.acc.float(), c.rs_live, True, torch.float32)
        d = D.ulp_distance(y32.bfloat16(), c.ref.float().bfloat16())
        assert int(d.max()) <= 1 and int((d > 0).sum()) <= max(1, c.R * c.n_out // 100), c.coords()
        nd, tot = nd + int((d > 0).sum()), tot + d.numel()
    with capsys.disabled():
        print(f"\nreference alone (torch fp32 against fp64), SwiGLU of the MXFP4 table: {nd} of {tot} outputs one step off")


# ---------------------------------------------------------------------------------------------------------------- the decoder
LIMIT = "at most 64 sequences, the grouped skinny-M GEMM's limit \\(no tiled W4A16 grouped GEMM is built\\)"


def test_without_the_keyword_nothing_changes():
    mix = _bare().enable_moe_batch().enable_moe_mxfp4()
    assert mix.moe_mxfp4 is True and mix.moe_mxfp4_tiled is False
    assert mix.MOE_MXFP4_ROWS == 64 and mix.MOE_GEMM_BATCH == 5 and mix.MOE_SKINNY_ROWS == 0 and 5 <= mix.MOE_MXFP4_TILED_FROM <= 65
    for B in (65, 70, 128):
        with pytest.raises(NotImplementedError, match=LIMIT):
            mix._ensure_batch(B)
    mix.k, mix.eps = 2, 1e-5
    with pytest.raises(NotImplementedError, match=LIMIT + "; got 65"):
        mix._token_block_batched_mxfp4({}, {}, None, None, 65, {}, None, None)
    assert _bare().moe_mxfp4_tiled is False


def test_tiled_admits_more_than_64_slots():
    mix = _bare().enable_moe_batch().enable_moe_mxfp4(tiled=True)
    assert mix.moe_mxfp4 is True and mix.moe_mxfp4_tiled is True
    mix._bb = dict(B=128, moe={})
    for B in (65, 70, 128):
        assert mix._ensure_batch(B)["B"] == 128
    mix.enable_moe_mxfp4(tiled=False)
    assert mix.moe_mxfp4 is True and mix.moe_mxfp4_tiled is False
    with pytest.raises(NotImplementedError, match=LIMIT):
        mix._ensure_batch(65)
    assert mix.enable_moe_mxfp4(False, tiled=True).moe_mxfp4_tiled is False      # (tiled means nothing with the switch off)
    assert mix._ensure_batch(100)["B"] == 128


def test_toggling_tiled_drops_the_graphs_bumps_the_epoch_and_is_refused_while_busy():
    mix = _bare()
    mix.cache_epoch = 3
    for tiled in (True, False, True):
        mix._batch_graphs, mix.graph, mix._graph_sample = {(4, False): object()}, object(), (object(), object())
        assert mix.enable_moe_mxfp4(tiled=tiled) is mix and mix.moe_mxfp4_tiled is tiled
        assert mix._batch_graphs == {} and mix.graph is None and mix._graph_sample == (None, None)
    assert mix.cache_epoch == 6
    copies = mix.w4moe
    assert mix.enable_moe_mxfp4(tiled=False).w4moe is copies and mix.enable_moe_mxfp4(tiled=True).w4moe is copies      # the copies are made once

    class Busy:
        n = 2

        def in_flight(self):
            return self.n
    mix._bb_busy = Busy()
    for tiled in (False, True):
        with pytest.raises(RuntimeError, match="enable_moe_mxfp4: a ContinuousBatcher holds requests in flight"):
            mix.enable_moe_mxfp4(tiled=tiled)
    assert mix.moe_mxfp4_tiled is True and mix.cache_epoch == 8
    mix._bb_busy.n = 0
    assert mix.enable_moe_mxfp4(tiled=False).moe_mxfp4_tiled is False


def test_the_two_expert_formats_still_refuse_each_other_with_tiled():
    mix = _bare().enable_moe_mxfp4(tiled=True)
    for kw in (dict(), dict(tiled=True)):
        with pytest.raises(ValueError, match="MXFP4 expert weights are on: call enable_moe_mxfp4\\(False\\) before enable_moe_fp8\\(\\)"):
            mix.enable_moe_fp8(**kw)
    assert mix.moe_mxfp4_tiled is True and mix.moe_fp8 is False
    mix.enable_moe_mxfp4(False).enable_moe_fp8(tiled=True)
    for kw in (dict(), dict(tiled=True)):
        with pytest.raises(ValueError, match="fp8 expert weights are on: call enable_moe_fp8\\(False\\) before enable_moe_mxfp4\\(\\)"):
            mix.enable_moe_mxfp4(**kw)
    assert mix.moe_fp8_tiled is True and mix.moe_mxfp4 is False and mix.moe_mxfp4_tiled is False


def _recorded(monkeypatch, mix, nb):
    """The ops.moe_* calls of one MXFP4 batched block of nb rows, by name."""
    from videollama2_amd import decoder as dec
    calls = []

    def rec(name, ret=None):
        def f(*a, **kw):
            calls.append((name, kw))
            return ret() if callable(ret) else ret
        return f
    route = lambda: dict(xg="xg", rn="rn", ids="route_ids", wts="route_wts")
    for name in ("moe_route_rows", "moe_gemv_batched_mxfp4", "moe_gemm_skinny_mxfp4", "moe_gemm_mxfp4", "moe_combine", "moe_gemm", "moe_gemm_skinny",
                 "moe_gemv_batched", "moe_gemm_fp8", "moe_gemm_skinny_fp8"):
        monkeypatch.setattr(dec.ops, name, rec(name, "t"))
    monkeypatch.setattr(dec.ops, "moe_route", rec("moe_route", route))
    monkeypatch.setattr(dec.ops, "rmsnorm", rec("rmsnorm", "h"))
    big = torch.zeros(4)
    m = dict(a=big, y=big, h=big, gather=big, inv=big, counts=big, offs=big, part=big)
    w4 = dict(wgu=("qgu", "sgu"), wd=("qd", "sd"))
    got = mix._token_block_batched_mxfp4(w4, dict(wr="wr"), "x", "x1", nb, m, "ids", "wts")
    return [n for n, _ in calls], calls, got


ROWS = ["moe_route_rows", "moe_gemv_batched_mxfp4", "moe_gemv_batched_mxfp4"]
SKINNY = ["moe_route_rows", "rmsnorm", "moe_gemm_skinny_mxfp4", "moe_gemm_skinny_mxfp4", "moe_combine"]
TILED = ["moe_route", "moe_gemm_mxfp4", "moe_gemm_mxfp4", "moe_combine"]


@pytest.mark.parametrize("tiled_from", (5, 65))
def test_the_regime_chosen_per_batch_size(monkeypatch, tiled_from):
    mix = _bare().enable_moe_batch().enable_moe_mxfp4(tiled=True)
    mix.k, mix.eps, mix.w["ones"] = 2, 1e-5, "ones"
    mix.MOE_MXFP4_TILED_FROM = tiled_from
    for nb in (1, 2, 4):
        names, calls, got = _recorded(monkeypatch, mix, nb)
        assert names == ROWS and got == ("ids", "wts"), nb
    for nb in (5, 8, 33, 64):
        names, calls, got = _recorded(monkeypatch, mix, nb)
        assert names == (TILED if nb >= tiled_from else SKINNY), nb
        assert got == (("route_ids", "route_wts") if nb >= tiled_from else ("ids", "wts"))
    for nb in (65, 70, 128, 1000):                                        # any nb from MOE_MXFP4_TILED_FROM on
        names, calls, got = _recorded(monkeypatch, mix, nb)
        assert names == TILED and got == ("route_ids", "route_wts"), nb
        gu, dn = calls[1][1], calls[2][1]
        assert gu == dict(swiglu=True, row_norm="rn", eps=1e-5) and dn == {}
    # without the keyword the tiled form is never chosen, whatever the constant says
    mix.enable_moe_mxfp4(tiled=False)
    for nb in (5, 64):
        assert _recorded(monkeypatch, mix, nb)[0] == SKINNY
    with pytest.raises(NotImplementedError, match=LIMIT + "; got 65"):
        _recorded(monkeypatch, mix, 65)


def test_the_tiled_block_hands_the_mxfp4_stacks_to_both_products(monkeypatch):
    from videollama2_amd import decoder as dec
    mix = _bare().enable_moe_batch().enable_moe_mxfp4(tiled=True)
    mix.k, mix.eps, mix.MOE_MXFP4_TILED_FROM = 2, 1e-5, 5
    seen = []
    monkeypatch.setattr(dec.ops, "moe_route", lambda x, wr, k, eps: seen.append(("route", x, wr, k)) or dict(xg="xg", rn="rn", ids="i", wts="w"))
    monkeypatch.setattr(dec.ops, "moe_gemm_mxfp4", lambda a, q, s, r, S, k, **kw: seen.append(("gemm", a, q, s, S, k)) or "a" + str(len(seen)))
    monkeypatch.setattr(dec.ops, "moe_combine", lambda x1, y, r, eps, out=None: seen.append(("combine", x1, y, out)))
    got = mix._token_block_batched_mxfp4(dict(wgu=("qgu", "sgu"), wd=("qd", "sd")), dict(wr="wr"), "x", "x1", 70, {}, None, None)
    assert seen == [("route", "x1", "wr", 2), ("gemm", "xg", "qgu", "sgu", 70, 2), ("gemm", "a2", "qd", "sd", 70, 2), ("combine", "x1", "a3", "x")]
    assert got == ("i", "w")


def test_the_op_takes_strides_from_the_tensors(monkeypatch):
    """ops.moe_gemm_mxfp4 on strided views: q_stride / ldq / s_stride / lds are the views' strides in bytes."""
    from videollama2_amd import _lib, ops
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: seen.append((name, a)))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_chk", lambda t, dtype, name: None)         # (the device / dtype check: host tensors stand in here)
    E, N, K, P = 2, 128, 128, 256
    qs, ss = torch.zeros((E, N + 1, K // 2 + 16), dtype=torch.uint8), torch.zeros((E, N + 1, K // 32 + 3), dtype=torch.uint8)
    a = torch.zeros((P, K), dtype=_lib.elem_dtype())
    route = dict(counts=torch.zeros(E, dtype=torch.int32), offs=torch.zeros(E + 1, dtype=torch.int32))
    out = ops.moe_gemm_mxfp4(a, qs[:, :N, :K // 2], ss[:, :N, :K // 32], route, 3, 2, swiglu=True)
    assert out.shape == (P, N // 2)
    (name, args), = seen
    assert name == NAME and args[1] == K and args[3:5] == ((N + 1) * (K // 2 + 16), K // 2 + 16) and args[6:8] == ((N + 1) * (K // 32 + 3), K // 32 + 3)
    assert len(args) == len(ARGS) and args[14:22] == (3, 2, E, P, N, K, 1, None)
    with pytest.raises(ValueError, match="moe_gemm_mxfp4: need q \\[E, N, K / 2\\] bytes"):
        ops.moe_gemm_mxfp4(a, qs[:, :N, :K // 2], ss[:, :N, :K // 32 + 1], route, 3, 2)


def test_model_switch_passes_the_keyword_through_and_a_dense_decoder_refuses():
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.decoder import HipMistralDecoder
    model = object.__new__(VideoLLaMA2Hip)
    model.__dict__["decoder"] = _bare()
    assert model.enable_moe_mxfp4(tiled=True) is model and model.decoder.moe_mxfp4 is True and model.decoder.moe_mxfp4_tiled is True
    assert model.enable_moe_mxfp4().decoder.moe_mxfp4_tiled is False and model.decoder.moe_mxfp4 is True
    model.enable_moe_mxfp4(False)
    assert model.decoder.moe_mxfp4 is False
    model.__dict__["decoder"] = object.__new__(HipMistralDecoder)
    with pytest.raises(NotImplementedError, match="enable_moe_mxfp4: the decoder is dense"):
        model.enable_moe_mxfp4(tiled=True)
