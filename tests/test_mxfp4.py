"""MXFP4 decode weights, everything that needs no GPU: the format's definition (tests/mxfp4_oracle.py) against the OCP MX v1.0 tables and PyTorch's
E8M0 type, the four entry points' place in the export tables, their argument checks (no launch), and the decoder switch's refusals."""
import ctypes
import math

import pytest
import torch

from oracle import vl2_oracle as O
from tests import mxfp4_oracle as M4
from tests.emu.backend import emulated_backend

NAMES = ("vl2_pack_quant_mxfp4", "vl2_gemv_mxfp4", "vl2_gemv_batched_mxfp4", "vl2_gemm_skinny_mxfp4")


def test_e2m1_codes_decode_encode_and_ties():
    table = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    for c in range(16):
        v = M4.e2m1_decode(c)
        assert abs(v) == table[c & 7] and (math.copysign(1.0, v) < 0) == bool(c & 8)
        assert M4.e2m1_encode(v) == c
    ties = [(0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0), (6.0001, 6.0), (7.9, 6.0), (1e9, 6.0)]
    for x, want in ties:
        for sgn in (1.0, -1.0):
            assert M4.e2m1_decode(M4.e2m1_encode(sgn * x)) == sgn * want, (x, sgn)
    # the vectorised encoder is the scalar one
    g = torch.Generator().manual_seed(0)
    v = torch.cat([torch.randn(4096, generator=g, dtype=torch.float64) * 3, torch.tensor([s * x for x, _ in ties for s in (1.0, -1.0)], dtype=torch.float64),
                   torch.tensor([0.0, -0.0, 0.2499, 0.2501], dtype=torch.float64)])
    assert M4.encode_tensor(v).tolist() == [M4.e2m1_encode(float(t)) for t in v]


def test_scale_bytes_are_e8m0_of_the_floor_rule():
    sub = float(torch.tensor(2.0 ** -130).bfloat16())                       # a bf16 denormal
    assert 0 < sub < 2.0 ** -126
    amax = [0.0, sub, 4.0, 5.9, 6.0, 7.99, 8.0, 2.0 ** -20, 1e30]
    want_e = [0, -127, 0, 0, 0, 0, 1, -22, 97]
    w = torch.zeros(len(amax), 32, dtype=torch.float64)
    w[:, 7] = torch.tensor(amax, dtype=torch.float64)
    w[:, 9] = -0.5 * w[:, 7]
    q, s = M4.quant_blocks(w)
    assert (s[:, 0].int() - 127).tolist() == want_e
    assert 0xFF not in s.tolist()
    e8 = torch.exp2(torch.tensor(want_e, dtype=torch.float32)).to(torch.float8_e8m0fnu).view(torch.uint8)
    assert torch.equal(s[:, 0], e8)
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(64, 4096, generator=g) * 0.02).bfloat16()
    w[3, 64:96] = 0
    q, s = M4.quant_blocks(w)
    am = w.float().view(64, -1, 32).abs().amax(dim=2).double()
    sc = torch.exp2(s.double() - 127)
    nz = am > 0
    assert bool(((4 * sc <= am) & (am < 8 * sc))[nz].all())
    assert int(s[3, 2]) == 127                                              # the zero block: e = 0
    assert torch.equal(s, torch.exp2(s.float() - 127).to(torch.float8_e8m0fnu).view(torch.uint8))


def test_dequant_of_quant_is_within_half_a_step_and_idempotent():
    g = torch.Generator().manual_seed(2)
    w = torch.cat([(torch.randn(32, 2048, generator=g) * 0.02), torch.distributions.StudentT(4.0).sample((32, 2048)) * 0.02]).bfloat16()
    q, s = M4.quant_blocks(w)
    d = M4.dequant(q, s).double()
    sc = torch.exp2(s.double() - 127).repeat_interleave(32, dim=1)
    a = w.double().abs() / sc
    # the E2M1 step at |v|: 0.5 below 2, 1 in [2, 4), 2 in [4, 6]
    step = torch.where(a < 2, torch.full_like(a, 0.5), torch.where(a < 4, torch.ones_like(a), torch.full_like(a, 2.0)))
    inside = a < 6
    assert bool((((d - w.double()).abs() / sc)[inside] <= step[inside] / 2).all())
    assert bool((d.abs()[~inside] == 6 * sc[~inside]).all()) and bool((torch.sign(d) == torch.sign(w.double()))[~inside].all())
    q2, s2 = M4.quant_blocks(d)
    assert torch.equal(q2, q) and torch.equal(s2, s)
    # byte order: k = 2j in bits 3:0
    w1 = torch.zeros(1, 32)
    w1[0, 0], w1[0, 1] = 6.0, -1.0
    q1, _ = M4.quant_blocks(w1)
    assert int(q1[0, 0]) == (0xA << 4 | 0x7)
    # the fp64 gemv multiplies by exactly these dequantised weights
    x = torch.randn(2048, generator=g).bfloat16()
    assert torch.equal(M4.gemv(q, s, x), d @ x.double())


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.vl2_last_error_string().decode()


def test_mxfp4_entry_points_are_exported_and_bound_apart_from_the_emulated_table(lib):
    from videollama2_amd import _lib
    plain = ctypes.CDLL(_lib.LIB_PATH)
    assert set(_lib.MXFP4_SIGNATURES) == set(NAMES)
    for name in NAMES:
        assert hasattr(plain, name), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.MXFP4_SIGNATURES[name]
    assert not set(_lib.MXFP4_SIGNATURES) & set(_lib.SIGNATURES)                # the emulator's symbol set is unchanged
    assert lib.vl2_version() == 7


def test_mxfp4_entry_points_refuse_bad_arguments_before_launching(lib):
    from videollama2_amd.ops import GEMM_OUT_F32, GEMM_SWIGLU
    p = ctypes.c_void_p(4096)                                       # stand-in device pointers: every case fails its checks first
    ws, wsb = ctypes.c_void_p(1 << 20), 64 << 20

    def quant(N=64, K=4096, w=p, q=p, s=p):
        return lib.vl2_pack_quant_mxfp4(w, N, K, K, q, s, K // 32, None)

    for kw, rc, msg in [(dict(K=4096 + 16), -2, "K%32==0"), (dict(q=None), -1, "null q"), (dict(s=None), -1, "null scale"), (dict(w=None), -1, "null w")]:
        assert quant(**kw) == rc and msg in _err(lib), (kw, _err(lib))

    def skinny(M=16, N=4096, K=4096, scale=p, bias=None, flags=0, ws=ws, wsb=wsb, q=p):
        return lib.vl2_gemm_skinny_mxfp4(p, q, scale, K // 32, p, bias, None, M, N, K, K, K // 2, N, 0, flags, ws, wsb, None)

    cases = [(dict(M=65), -2, "M<=64"), (dict(N=4096 + 32), -2, "N%64==0"), (dict(K=4096 + 16), -2, "K%32==0"),
             (dict(ws=None), -1, "workspace"), (dict(wsb=1024), -1, "workspace too small"), (dict(scale=None), -1, "null scale"),
             (dict(q=None), -1, "null q"), (dict(bias=p, flags=GEMM_SWIGLU), -3, "SWIGLU excludes bias"),
             (dict(flags=GEMM_SWIGLU | GEMM_OUT_F32), -3, "SWIGLU excludes bias / f32")]
    for kw, rc, msg in cases:
        assert skinny(**kw) == rc, (kw, _err(lib))
        assert msg in _err(lib), (kw, _err(lib))
    need16 = 16 * 16 * 4096 * 4                                     # ks = 16 at N = K = 4096, Mp = 16: the split is never shrunk to fit
    assert skinny(M=64, wsb=need16) == -1 and "workspace too small" in _err(lib)

    def gemv_b(MB=4, N=4096, K=4096, scale=p, bias=None, flags=0, q=p):
        n_out = N // 2 if flags & GEMM_SWIGLU else N
        return lib.vl2_gemv_batched_mxfp4(q, scale, K // 32, p, None, None, bias, p, MB, N, K, K // 2, K, n_out, 0, 1e-5, flags, None)

    def gemv_1(N=4096, K=4096, scale=p, bias=None, flags=0, q=p, MB=1):
        return lib.vl2_gemv_mxfp4(q, scale, K // 32, p, None, None, bias, p, N, K, K // 2, 1e-5, flags, None)

    cases = [(dict(scale=None), -1, "null scale"), (dict(q=None), -1, "null q"), (dict(K=4096 + 16), -2, "K%32==0"),
             (dict(K=32768), -2, "K<=32704"), (dict(N=4097), -2, "N even"), (dict(bias=p, flags=GEMM_SWIGLU), -3, "SWIGLU excludes bias"),
             (dict(flags=GEMM_SWIGLU | GEMM_OUT_F32), -3, "SWIGLU excludes bias / f32"), (dict(N=4096 + 32, flags=GEMM_SWIGLU), -2, "N%64==0")]
    for fn in (gemv_b, gemv_1):
        for kw, rc, msg in cases:
            assert fn(**kw) == rc, (fn.__name__, kw, _err(lib))
            assert msg in _err(lib) and fn.__name__.replace("gemv_b", "vl2_gemv_batched_mxfp4").replace("gemv_1", "vl2_gemv_mxfp4") in _err(lib)
    assert gemv_b(MB=0) == -1 and "empty shape" in _err(lib)


def test_enable_mxfp4_decode_refusals_come_before_any_library_call(golden_small, monkeypatch):
    from videollama2_amd import _lib
    from videollama2_amd.decoder import HipMistralDecoder, HipMixtralDecoder
    cfg = golden_small["cfg"]
    keep = lambda n: n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))
    with emulated_backend():
        dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, golden_small["seed"], round_bf16=True, only=keep), "cpu", max_seq_len=32)

        def no_call(name, *a):
            raise AssertionError(f"library call {name} before the refusal")
        monkeypatch.setattr(_lib, "call", no_call)
        assert dec.decode_format == "16bit" and hasattr(dec, "enable_mxfp4_decode")
        dec.tp = 2
        with pytest.raises(NotImplementedError, match="single-rank"):
            dec.enable_mxfp4_decode()
        dec.tp = 1
        dec.decode_fp8 = True                                        # as enable_fp8_decode() leaves it
        with pytest.raises(ValueError, match=r"enable_fp8_decode\(False\)"):
            dec.enable_mxfp4_decode()
        dec.decode_fp8, dec.decode_mxfp4 = False, True
        with pytest.raises(ValueError, match=r"enable_mxfp4_decode\(False\)"):
            dec.enable_fp8_decode()
        dec.decode_mxfp4 = False
        moe = HipMixtralDecoder.__new__(HipMixtralDecoder)           # the refusal needs no weights
        with pytest.raises(NotImplementedError, match="MXFP4"):
            moe.enable_mxfp4_decode()
        assert dec.decode_format == "16bit" and dec.cache_epoch == 0
