"""CPU-only functional check of the REAL host code and the REAL kernel sources: the kernel headers are compiled for
the host against tests/emu/hip_emu.h (fibers + emulated MFMA / LDS-DMA / shuffles), exported under the same C ABI,
and the unmodified videollama2_amd host layer runs the small config end to end against the reference goldens.
This guards kernel indexing logic (swizzles, fragment maps, edge rows) where no GPU exists; the `-m gpu` tests are
the parity tests proper."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import vl2_oracle as O
from tests.emu.backend import emulated_backend
from tests.util import TOL_BF16_OUT, TOL_F32_OUT, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    with emulated_backend() as lib:
        yield lib


def bf(*shape, scale=1.0, seed=0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape))) * scale).bfloat16()


def test_emu_gemm_variants(emu):
    from videollama2_amd import ops
    from videollama2_amd.weights import pack_gate_up
    M, N, K = 200, 256, 192
    a, w, bias, res = bf(M, K), bf(N, K), torch.randn(N), bf(M, N)
    assert rel(ops.gemm(a, w, out_f32=True), a.float() @ w.float().T) < TOL_F32_OUT
    y = F.linear(a.float(), w.float(), bias)
    assert rel(ops.gemm(a, w, bias=bias, res=res, act=ops.ACT_QGELU), y * torch.sigmoid(1.702 * y) + res.float()) < TOL_BF16_OUT
    assert rel(ops.gemm(a, w, bias=bias, act=ops.ACT_GELU), F.gelu(y)) < TOL_BF16_OUT
    wg, wu = bf(128, K), bf(128, K, seed=1)
    ref = F.silu(a.float() @ wg.float().T) * (a.float() @ wu.float().T)
    assert rel(ops.gemm(a, pack_gate_up(wg, wu), swiglu=True), ref) < TOL_BF16_OUT
    # patch-embed style row remap: groups of 16 rows -> 17-row frames, residual row = m % 16 + 1
    a2, w2, pos = bf(64, 128), bf(128, 128), bf(17, 128)
    out = torch.zeros(4 * 17, 128, dtype=torch.bfloat16)
    ops.gemm(a2, w2, res=pos, out=out, out_map=(16, 1, 1), res_map=(16, 1))
    ref = (a2.float() @ w2.float().T).view(4, 16, 128) + pos.float()[1:][None]
    assert rel(out.view(4, 17, 128)[:, 1:], ref) < TOL_BF16_OUT and out.view(4, 17, 128)[:, 0].abs().max() == 0


def test_emu_gemm_mixed_launch(emu):
    """k_gemm.h gemm_mix_bf16_kernel (the row-split GEMM as ONE launch: 256x256 ping-pong tiles on the leading rows, 8-wave 128x128 tiles
    on the tail; emulator knob 24): same bits as the 128x128 kernel, with and without a residual (LDS / C^T epilogue of the big part),
    SwiGLU, and a LayerNorm-carrying input whose statistics rows are shifted for the tail."""
    from videollama2_amd import ops
    from videollama2_amd.weights import pack_gate_up
    M, N, K = 300, 512, 128
    a, w, bias, res = bf(M, K), bf(N, K, scale=K ** -0.5), torch.randn(N), bf(M, N)
    wgu = pack_gate_up(bf(256, K, seed=3), bf(256, K, seed=4))
    st = ops.row_stats(a)
    try:
        ops.set_gemm_variant(1)
        refs = (ops.gemm(a, w, bias=bias, res=res, act=ops.ACT_QGELU), ops.gemm(a, w, bias=bias, act=ops.ACT_GELU), ops.gemm(a, wgu, swiglu=True),
                ops.gemm(a, w, norm=(ops.NORM_RMS, st, 1e-5, None)))
        st_ref = torch.zeros(M, N // 64, 2)
        ops.gemm(a, w, bias=bias, res=res, stats_out=st_ref)
        ops.set_gemm_variant(24)
        outs = (ops.gemm(a, w, bias=bias, res=res, act=ops.ACT_QGELU), ops.gemm(a, w, bias=bias, act=ops.ACT_GELU), ops.gemm(a, wgu, swiglu=True),
                ops.gemm(a, w, norm=(ops.NORM_RMS, st, 1e-5, None)))
        st_out = torch.zeros(M, N // 64, 2)
        ops.gemm(a, w, bias=bias, res=res, stats_out=st_out)
    finally:
        ops.set_gemm_variant(0)
    for i, (r, o) in enumerate(zip(refs, outs)):
        assert torch.equal(r, o), i
    assert torch.equal(st_ref, st_out)


def test_emu_norm_carrying_gemms(emu):
    """csrc/k_gemm.h "norm-carrying GEMMs": (1) the statistics a producer GEMM emits are bit-identical to `row_stats` of its
    stored output, whichever kernel ran it; (2) RMSNorm / LayerNorm computed in the consumer's epilogue from those statistics
    (weights.fold_norm) match the fp32 norm -> linear of HF MistralRMSNorm / nn.LayerNorm within one bf16 output rounding;
    (3) every kernel variant gives the same bits."""
    from videollama2_amd import ops
    from videollama2_amd.weights import fold_norm, pack_gate_up
    M, N, K = 200, 256, 192
    a, w, bias, res = bf(M, K), bf(N, K), torch.randn(N), bf(M, N, scale=2.0)
    st = torch.full((M, N // 64, 2), -7.0)
    x = ops.gemm(a, w, bias=bias, res=res, stats_out=st)                 # a residual-stream write, as out_proj / fc2 / o_proj / down
    assert torch.equal(st, ops.row_stats(x))
    xf = x.float()
    assert rel(st[..., 0].sum(1), xf.sum(1)) < 1e-5 and rel(st[..., 1].sum(1), (xf * xf).sum(1)) < 1e-5
    # consumers: x [M, 256] is the A operand now (K = 256)
    g, b = 1 + 0.3 * torch.randn(N), 0.2 * torch.randn(N)
    w2, c2 = bf(384, N, seed=3), torch.randn(384)
    eps = 1e-5
    h_rms = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * g.bfloat16().float()
    h_ln = F.layer_norm(xf, (N,), g.bfloat16().float(), b.bfloat16().float(), eps)
    wr, _, _ = fold_norm(w2, g)
    y_rms = ops.gemm(x, wr, bias=c2, norm=(ops.NORM_RMS, st, eps, None))
    assert rel(y_rms, F.linear(h_rms, w2.float(), c2)) < TOL_BF16_OUT
    wl, sl, tl = fold_norm(w2, g, b, c2)
    y_ln = ops.gemm(x, wl, bias=tl, act=ops.ACT_QGELU, norm=(ops.NORM_LN, st, eps, sl))
    ref = F.linear(h_ln, w2.float(), c2.bfloat16().float())
    assert rel(y_ln, ref * torch.sigmoid(1.702 * ref)) < TOL_BF16_OUT
    wg, wu = bf(128, N, seed=5), bf(128, N, seed=6)
    wgu, _, _ = fold_norm(pack_gate_up(wg, wu), g)
    y_sw = ops.gemm(x, wgu, swiglu=True, norm=(ops.NORM_RMS, st, eps, None))
    assert rel(y_sw, F.silu(h_rms @ wg.float().T) * (h_rms @ wu.float().T)) < TOL_BF16_OUT
    # a mean far from zero (LayerNorm's cancellation case: mean ~ 8 sigma) and every kernel variant
    x2 = (xf + 8.0 * xf.std()).bfloat16()
    st2 = ops.row_stats(x2)
    ref2 = F.linear(F.layer_norm(x2.float(), (N,), g.bfloat16().float(), b.bfloat16().float(), eps), w2.float(), c2.bfloat16().float())
    y2 = ops.gemm(x2, wl, bias=tl, norm=(ops.NORM_LN, st2, eps, sl))
    assert rel(y2, ref2) < TOL_BF16_OUT
    try:
        for v in (1, 4, 5, 8, 10, 12, 32, 256):                             # 10 = the 160-row tile (round 6): the 192-row tile without group 1's third row block
            ops.set_gemm_variant(v)
            stv = torch.zeros_like(st)
            assert torch.equal(ops.gemm(a, w, bias=bias, res=res, stats_out=stv), x) and torch.equal(stv, st), v
            assert torch.equal(ops.gemm(x2, wl, bias=tl, norm=(ops.NORM_LN, st2, eps, sl)), y2), v
            if v != 32:                                                    # the 64x64 small-M kernel has no SwiGLU form (10: falls back to the automatic choice)
                assert torch.equal(ops.gemm(x, wgu, swiglu=True, norm=(ops.NORM_RMS, st, eps, None)), y_sw), v
    finally:
        ops.set_gemm_variant(0)


def test_emu_gemm_producer_side_finalize_equals_the_launch(emu):
    """k_gemm.h gemm_rows_ticket (round 5): a statistics-producing GEMM leaves (mean, rstd) of its output rows in `row_norm_out` itself -- the
    workgroup that stores the last column tile of a row block reduces the block's partials.  On every tile shape (128x128, 128x256, 256x256,
    192x256, 224x128, 192x128, the 8-wave 128x128, the mixed launch) and both epilogue forms, ragged M: the same bits as
    row_norm_finalize(stats_out), LayerNorm and RMSNorm; the tickets come back zeroed (one block serves a stream of GEMMs); kernels without the
    epilogue (64x64 tiles, split-K) and VL2_GEMM_NO_TICKET get the launch appended by vl2_gemm -- same result."""
    from videollama2_amd import ops
    M, N, K = 700, 512, 256
    a, w, bias, res = bf(M, K), bf(N, K, scale=K ** -0.5), torch.randn(N), bf(M, N)
    try:
        for kind, eps in ((ops.NORM_LN, 1e-5), (ops.NORM_RMS, 1e-6)):
            ops.set_gemm_variant(1)
            st_ref = torch.zeros(M, N // 64, 2)
            y_ref = ops.gemm(a, w, bias=bias, res=res, stats_out=st_ref)
            rn_ref = ops.row_norm_finalize(st_ref, N, kind, eps)
            for v, use_res in ((1, True), (4, True), (4, False), (8, True), (8, False), (12, True), (12, False), (10, True), (10, False), (224, True), (192, True), (256, True),
                               (24, True), (24, False), (32, True), (0, True)):
                ops.set_gemm_variant(v)
                st, rn, tick = torch.zeros(M, N // 64, 2), torch.full((M, 2), -7.0), torch.zeros(M // 64 + 2, dtype=torch.int32)
                r = res if use_res else None
                y = ops.gemm(a, w, bias=bias, res=r, stats_out=st, norm_out=(kind, eps, rn, tick))
                if use_res:
                    assert torch.equal(y, y_ref) and torch.equal(st, st_ref), v
                    assert torch.equal(rn, rn_ref), (v, kind, (rn - rn_ref).abs().max())
                else:
                    assert torch.equal(rn, ops.row_norm_finalize(st, N, kind, eps)), (v, kind)
                assert int(tick.abs().sum()) == 0, f"variant {v}: tickets not re-armed"
            ops.set_gemm_variant(0)
            ops.set_stage_flags(ops.STAGE_NO_TICKET_OPS)                       # the launch appended by vl2_gemm (A/B form)
            st, rn, tick = torch.zeros(M, N // 64, 2), torch.zeros(M, 2), torch.zeros(M // 64 + 2, dtype=torch.int32)
            ops.gemm(a, w, bias=bias, res=res, stats_out=st, norm_out=(kind, eps, rn, tick))
            assert torch.equal(rn, rn_ref) and int(tick.abs().sum()) == 0
            ops.set_stage_flags(0)
            ops.set_splitk(True)                                            # split-K kernel: no ticket epilogue -> appended launch
            ops.set_gemm_variant(1)
            st, rn = torch.zeros(M, N // 64, 2), torch.zeros(M, 2)
            ops.gemm(a, w, bias=bias, res=res, stats_out=st, norm_out=(kind, eps, rn, tick))
            assert torch.equal(rn, ops.row_norm_finalize(st, N, kind, eps))
            ops.set_splitk(False)
    finally:
        ops.set_gemm_variant(0)
        ops.set_stage_flags(0)
        ops.set_splitk(False)


def test_emu_gemm_pingpong_variant(emu):
    from videollama2_amd import ops
    for K in (64, 128, 448):
        a, w = bf(300, K), bf(512, K)
        ref = ops.gemm(a, w, out_f32=True)
        try:
            for v in (4, 5, 8, 9, 256):                             # 9 = gemm8: the 256 x 256 tile on four waves (k_gemm8.h)
                ops.set_gemm_variant(v)
                assert torch.equal(ops.gemm(a, w, out_f32=True), ref)
        finally:
            ops.set_gemm_variant(0)
    # WEAVE4: the 256 x 256 / 192 x 256 bodies (and the mixed launch's big tiles) with the LDS-DMA of slab t+3 issued from the matrix phases
    for M, K in ((300, 64), (520, 192), (700, 576)):
        a, w, bias, res = bf(M, K), bf(512, K, scale=K ** -0.5), torch.randn(512), bf(M, 512)
        try:
            ops.set_gemm_variant(1)
            refs = (ops.gemm(a, w, bias=bias, res=res), ops.gemm(a, w, bias=bias, act=ops.ACT_QGELU))
            for v in (8, 12, 24):
                ops.set_gemm_variant(v)
                for fl in (ops.STAGE_WEAVE4, ops.STAGE_NO_WEAVE4, 0):             # woven everywhere | nowhere | the default (192-row tiles only)
                    ops.set_stage_flags(fl)
                    assert torch.equal(ops.gemm(a, w, bias=bias, res=res), refs[0]) and torch.equal(ops.gemm(a, w, bias=bias, act=ops.ACT_QGELU), refs[1]), (M, K, v, fl)
                ops.set_stage_flags(0)
        finally:
            ops.set_gemm_variant(0)
            ops.set_stage_flags(0)
    # gemm8 through every epilogue form: LDS patches (residual, statistics + producer-side finalize) and the register-resident C^T form (bias /
    # activation, SwiGLU, LayerNorm carried), ragged M, K from one slab to a full ring and beyond
    from videollama2_amd.weights import pack_gate_up
    for M, K in ((300, 64), (257, 192), (520, 576)):
        a, w, bias, res = bf(M, K), bf(512, K, scale=K ** -0.5), torch.randn(512), bf(M, 512)
        wgu = pack_gate_up(bf(256, K, seed=3), bf(256, K, seed=4))
        rn_in = ops.row_norm_finalize(ops.row_stats(a), K, ops.NORM_LN, 1e-5)
        outs = {}
        try:
            for v in (1, 9):
                ops.set_gemm_variant(v)
                st, rn, tick = torch.zeros(M, 8, 2), torch.zeros(M, 2), torch.zeros(M // 64 + 2, dtype=torch.int32)
                outs[v] = [ops.gemm(a, w, bias=bias, res=res, stats_out=st, norm_out=(ops.NORM_LN, 1e-5, rn, tick)), st, rn,
                           ops.gemm(a, w, bias=bias, act=ops.ACT_QGELU), ops.gemm(a, wgu, swiglu=True)]
                outs[v].append(ops.gemm(a, w, bias=bias, norm=(ops.NORM_LN, rn_in, 1e-5, torch.randn(512, generator=torch.Generator().manual_seed(1)))))
            assert all(torch.equal(x, y) for x, y in zip(outs[1], outs[9])), (M, K)
        finally:
            ops.set_gemm_variant(0)


def test_emu_gemm_mfma16_kernel(emu):
    """csrc/k_gemm9.h: the 256 x 256 ping-pong tile on v_mfma_f32_16x16x32_bf16 (variant 16 / VL2_GEMM_MFMA16 / STAGE_MFMA16).  The ONE kernel whose
    dot products associate differently from the family's ON THE GPU: held to the fp32 result at the family's tolerance, to the family's bits (emulator only),
    and to ITSELF across M (a row's bits do not depend on how many rows the call has) and across the ways of asking for it."""
    from videollama2_amd import ops
    from videollama2_amd.weights import fold_norm, pack_gate_up
    for M, K in ((300, 64), (257, 192), (520, 576)):                      # ragged M; K = 2 slabs (the ring never fills), 6, 18
        N = 512
        a, w, bias, res = bf(M, K), bf(N, K, scale=K ** -0.5), torch.randn(N), bf(M, N)
        wg, wu = bf(256, K, scale=K ** -0.5, seed=3), bf(256, K, scale=K ** -0.5, seed=4)
        g = 1 + 0.3 * torch.randn(K, generator=torch.Generator().manual_seed(5))
        wgu, _, _ = fold_norm(pack_gate_up(wg, wu), g)
        af = a.float()
        rn = ops.row_norm_finalize(ops.row_stats(a), K, ops.NORM_RMS, 1e-6)
        h = af * torch.rsqrt(af.pow(2).mean(-1, keepdim=True) + 1e-6) * g.bfloat16().float()
        fam = (ops.gemm(a, w, bias=bias, res=res), ops.gemm(a, wgu, swiglu=True, norm=(ops.NORM_RMS, rn, 1e-6, None)))
        try:
            ops.set_gemm_variant(16)
            y = ops.gemm(a, w, bias=bias, res=res)
            y_sw = ops.gemm(a, wgu, swiglu=True, norm=(ops.NORM_RMS, rn, 1e-6, None))
            assert rel(y, F.linear(af, w.float(), bias) + res.float()) < TOL_BF16_OUT, (M, K)
            assert rel(y_sw, F.silu(h @ wg.float().T) * (h @ wu.float().T)) < TOL_BF16_OUT, (M, K)
            # the emulated matrix instructions both sum their k in ascending order, so HERE the kernel must reproduce the family's bits exactly (an
            # indexing check stronger than any tolerance); on the GPU the two instructions associate differently (tests/test_gpu_ops.py holds the bound)
            assert torch.equal(y, fam[0]) and torch.equal(y_sw, fam[1]), (M, K)
            for v in (17, 18, 19, 20, 21, 22, 26):                          # lab forms (k_gemm9.h MODE 1 / 2 / 4 / 5 / 6: orders of the LDS-DMA issue; 3: register-staged slabs; 9: 64-deep phases)
                ops.set_gemm_variant(v)
                assert torch.equal(ops.gemm(a, w, bias=bias, res=res), y) and torch.equal(ops.gemm(a, wgu, swiglu=True, norm=(ops.NORM_RMS, rn, 1e-6, None)), y_sw), (M, K, v)
            # round 6: the other tiles of the 16 x 16 x 32 set (the decoder's o / down projections: residual + row statistics [+ producer-side finalize]): the
            # one-round 128 x 128 body (k_gemm9.h gemm_l8_16_body) and the fill-the-round tiles (k_gemm7.h gemm7_loop16), by the flag (auto) and on demand
            st_f, rn_f, tick = torch.zeros(M, N // 64, 2), torch.zeros(M, 2), torch.zeros(M // 64 + 2, dtype=torch.int32)
            ops.set_gemm_variant(1)
            y_f = ops.gemm(a, w, bias=bias, res=res, stats_out=st_f, norm_out=(ops.NORM_RMS, 1e-6, rn_f, tick))
            for v in (0, 256, 224, 192, 16, 26):
                ops.set_gemm_variant(v)
                st_v, rn_v = torch.zeros(M, N // 64, 2), torch.full((M, 2), -3.0)
                y_v = ops.gemm(a, w, bias=bias, res=res, stats_out=st_v, norm_out=(ops.NORM_RMS, 1e-6, rn_v, tick), mfma16=True)
                assert torch.equal(y_v, y_f) and torch.equal(st_v, st_f) and torch.equal(rn_v, rn_f) and int(tick.abs().sum()) == 0, (M, K, v)
            ops.set_gemm_variant(16)
            m1 = M - 130                                                    # fewer rows, other tile edge: the same bits row for row
            assert torch.equal(ops.gemm(a[:m1], w, bias=bias, res=res[:m1]), y[:m1])
            assert torch.equal(ops.gemm(a[:m1], wgu, swiglu=True, norm=(ops.NORM_RMS, rn[:m1], 1e-6, None)), y_sw[:m1])
            with pytest.raises(RuntimeError):                               # variant 16 is a demand: not built for activations / fp32 outputs
                ops.gemm(a, w, bias=bias, act=ops.ACT_QGELU)
            ops.set_gemm_variant(0)
            ops.set_stage_flags(ops.STAGE_MFMA16)                           # the session switch: SwiGLU GEMMs only
            assert torch.equal(ops.gemm(a, wgu, swiglu=True, norm=(ops.NORM_RMS, rn, 1e-6, None)), y_sw)
            assert torch.equal(ops.gemm(a, w, bias=bias, res=res), fam[0])
        finally:
            ops.set_gemm_variant(0)
            ops.set_stage_flags(0)


def test_emu_gemm_persistent_kernels_are_bit_identical(emu):
    """csrc/k_gemm6.h (persistent ping-pong GEMM; emulator knobs 60 = 256-row tiles, 61 = 192-row tiles, 62 = 192-row tiles with two
    accumulator sets and the previous tile's epilogue drained under the next tile's phases): three workgroups walk 6-15 tiles each across
    tile boundaries (ring never drained, epilogue vectors through the LDS aux block, last row tile shifted back to end at M): same bits
    as the one-tile-per-workgroup kernel for plain / bias + QuickGELU / LayerNorm- and RMSNorm-carrying / SwiGLU epilogues."""
    from videollama2_amd import ops
    from videollama2_amd.weights import pack_gate_up
    M, N, K = 700, 768, 512
    a, w, bias = bf(M, K), bf(N, K, scale=K ** -0.5), torch.randn(N)
    wgu = pack_gate_up(bf(384, K, seed=3, scale=K ** -0.5), bf(384, K, seed=4, scale=K ** -0.5))
    st = ops.row_norm_finalize(ops.row_stats(a), K, ops.NORM_LN, 1e-5)
    st_rms = ops.row_norm_finalize(ops.row_stats(a), K, ops.NORM_RMS, 1e-5)
    colsum = w.float().sum(1)

    def run():
        return (ops.gemm(a, w), ops.gemm(a, w, bias=bias, act=ops.ACT_QGELU),
                ops.gemm(a, w, bias=bias, norm=(ops.NORM_LN, st, 1e-5, colsum)),
                ops.gemm(a, w, bias=bias, act=ops.ACT_QGELU, norm=(ops.NORM_LN, st, 1e-5, colsum)),
                ops.gemm(a, w, norm=(ops.NORM_RMS, st_rms, 1e-5, None)),
                ops.gemm(a, wgu, swiglu=True), ops.gemm(a, wgu, swiglu=True, norm=(ops.NORM_RMS, st_rms, 1e-5, None)))
    try:
        ops.set_gemm_variant(8)
        refs = run()
        for v in (60, 61, 62, 70, 71, 80, 81):  # 70 / 71 = 60 / 61 with the tiles handed out through the counter block, 80 / 81 = the first tile too
            ops.set_gemm_variant(v)
            for i, (r, o) in enumerate(zip(refs, run())):
                assert torch.equal(r, o), (v, i, (r.float() - o.float()).abs().max().item())
    finally:
        ops.set_gemm_variant(0)


def test_emu_gemm_splitk_plain_and_gathered(emu):
    """Split-K form of the 128x128 kernel (emulator knob 116): partial tiles through the workspace, last arriver reduces in
    split order and re-arms the tile counter (second launch reuses the counters without a host reset)."""
    from videollama2_amd import ops
    from videollama2_amd.connector import conv3d_k2s2p1_index
    a, w, bias, res = bf(200, 768), bf(256, 768), torch.randn(256), bf(200, 256)
    ref = ops.gemm(a, w, bias=bias, res=res, act=ops.ACT_SILU)
    ref32 = ops.gemm(a, w, out_f32=True)
    T, H, C = 4, 4, 128
    pool, w3, b3 = bf(T * H * H, C), bf(128, 8 * C, scale=0.05), torch.randn(128)
    idx, _ = conv3d_k2s2p1_index(T, H, H, "cpu")
    zero = torch.zeros(C, dtype=torch.bfloat16)
    refg = ops.gemm(pool, w3, bias=b3, act=ops.ACT_SILU, gather=(idx, zero, C))
    try:
        ops.set_gemm_variant(116)
        for _ in range(2):
            assert rel(ops.gemm(a, w, bias=bias, res=res, act=ops.ACT_SILU), ref.float()) < 2e-3
            assert rel(ops.gemm(a, w, out_f32=True), ref32) < 1e-5
            assert rel(ops.gemm(pool, w3, bias=b3, act=ops.ACT_SILU, gather=(idx, zero, C)), refg.float()) < 2e-3
    finally:
        ops.set_gemm_variant(0)


def test_emu_gemm_small_m_kernel_is_bit_identical(emu):
    """64x64 small-M kernel (knob 32): same K order as the 128-wide kernels -> identical bits, plain and gathered, ragged M,
    K-tile counts below / at / above the ring depth."""
    from videollama2_amd import ops
    from videollama2_amd.connector import conv3d_k2s2p1_index
    for M, K in ((70, 64), (129, 128), (200, 192), (33, 448)):
        a, w, bias, res = bf(M, K), bf(256, K), torch.randn(256), bf(M, 256)
        ref = ops.gemm(a, w, bias=bias, res=res, act=ops.ACT_GELU)
        try:
            ops.set_gemm_variant(32)
            assert torch.equal(ops.gemm(a, w, bias=bias, res=res, act=ops.ACT_GELU), ref)
        finally:
            ops.set_gemm_variant(0)
    T, H, C = 4, 4, 128
    pool, w3, b3 = bf(T * H * H, C), bf(128, 8 * C, scale=0.05), torch.randn(128)
    idx, _ = conv3d_k2s2p1_index(T, H, H, "cpu")
    zero = torch.zeros(C, dtype=torch.bfloat16)
    refg = ops.gemm(pool, w3, bias=b3, act=ops.ACT_SILU, gather=(idx, zero, C))
    try:
        ops.set_gemm_variant(32)
        assert torch.equal(ops.gemm(pool, w3, bias=b3, act=ops.ACT_SILU, gather=(idx, zero, C)), refg)
    finally:
        ops.set_gemm_variant(0)


def test_emu_gemm_fill_round_kernel_is_bit_identical(emu):
    """csrc/k_gemm7.h (224 x 128 / 192 x 128 ping-pong tiles, knobs 224 / 192): two wave groups with DIFFERENT row ranges (2 x 2 and R1 x 1
    blocks), 44 / 40 LDS-DMA pieces per stage dealt over 8 waves, the shared fp32 image epilogue -- same K order and epilogue arithmetic as
    the 128 x 128 kernel, so the same bits: every epilogue the decoder's o / down projections and the connector use, ragged M over one
    and several row tiles, K-tile counts 1 / 2 / 3 / 7 (below, at and above the ring depth), fp32 output, the norm-carrying forms, gather."""
    from videollama2_amd import ops
    from videollama2_amd.connector import conv3d_k2s2p1_index
    for M, N, K in ((250, 256, 64), (225, 128, 128), (470, 128, 192), (193, 256, 448), (200, 128, 256)):
        a, w, bias, res = bf(M, K), bf(N, K), torch.randn(N), bf(M, N)
        st = torch.zeros((M, K // 64, 2), dtype=torch.float32)
        xs = bf(M, K)
        ops.row_stats(xs, out=st)
        colsum = w.float().sum(1)
        def run():
            so = torch.zeros((M, N // 64, 2), dtype=torch.float32)
            outs = (ops.gemm(a, w, bias=bias, res=res, act=ops.ACT_GELU), ops.gemm(a, w, bias=bias, act=ops.ACT_QGELU), ops.gemm(a, w, out_f32=True),
                    ops.gemm(a, w, res=res, stats_out=so), so)
            if K % 128 == 0:                                       # the statistics rows of a norm-carrying GEMM are read as 16-B vectors
                outs += (ops.gemm(xs, w, bias=bias, norm=(ops.NORM_LN, st, 1e-5, colsum)), ops.gemm(xs, w, norm=(ops.NORM_RMS, st, 1e-5, None)))
            return outs
        try:
            ops.set_gemm_variant(1)
            ref = run()
            for v in (224, 192, 225, 193):
                ops.set_gemm_variant(v)
                got = run()
                assert all(torch.equal(x, y) for x, y in zip(got, ref)), (M, N, K, v)
        finally:
            ops.set_gemm_variant(0)
    T, H, C = 4, 4, 128
    pool, w3, b3 = bf(T * H * H, C), bf(128, 8 * C, scale=0.05), torch.randn(128)
    idx, _ = conv3d_k2s2p1_index(T, H, H, "cpu")
    zero = torch.zeros(C, dtype=torch.bfloat16)
    try:
        ops.set_gemm_variant(1)
        refg = ops.gemm(pool, w3, bias=b3, act=ops.ACT_SILU, gather=(idx, zero, C))
        for v in (224, 192, 225, 193):
            ops.set_gemm_variant(v)
            assert torch.equal(ops.gemm(pool, w3, bias=b3, act=ops.ACT_SILU, gather=(idx, zero, C)), refg), v
    finally:
        ops.set_gemm_variant(0)


def test_emu_gemm_fp8_matrix_pipe_against_the_oracle(emu):
    """VL2_GEMM_FP8 (W8A8 on v_mfma_f32_32x32x64_f8f6f4; k_gemm.h gemm3 / gemm4 FP8, k_fp8.h quant_act_fp8_kernel) on the emulator: the
    activation quantiser bit for bit against oracle/fp8_oracle.py, the GEMM (all three tile shapes; plain, bias + SiLU, residual, SwiGLU,
    fp32 output) against gemm_w8a8 to fp32 summation order."""
    from oracle import fp8_oracle as F8
    from videollama2_amd import ops
    M, N, K = 200, 256, 256
    x, w, bias, res = bf(M, K), bf(N, K, scale=K ** -0.5), torch.randn(N), bf(M, N)
    x[3] = 0
    x[5, 7] = 300.0                                                # an outlier row: the other elements land in the subnormal codes
    qw, sw = ops.quant_fp8(w)
    for eps in (None, 1e-5):
        qa, tab = ops.quant_act_fp8(x, rms_eps=eps)
        qo, to = F8.quant_act_rows(x, rms_eps=eps)
        assert torch.equal(qa, qo) and rel(tab, to) < 1e-6 and torch.equal(tab[:, 0], to[:, 0])
        try:
            for v in (4, 8, 12):
                ops.set_gemm_variant(v)
                if v != 12:
                    assert rel(ops.gemm_fp8(qa, tab, qw, sw, out_f32=True), F8.gemm_w8a8(qa, tab, qw, sw)) < 1e-5, v
                assert rel(ops.gemm_fp8(qa, tab, qw, sw, bias=bias, act=ops.ACT_SILU), F8.gemm_w8a8(qa, tab, qw, sw, bias=bias, act="silu")) < TOL_BF16_OUT
                assert rel(ops.gemm_fp8(qa, tab, qw, sw, res=res), F8.gemm_w8a8(qa, tab, qw, sw, res=res)) < TOL_BF16_OUT
                assert rel(ops.gemm_fp8(qa, tab, qw, sw, swiglu=True), F8.gemm_w8a8(qa, tab, qw, sw, swiglu=True)) < TOL_BF16_OUT
        finally:
            ops.set_gemm_variant(0)


def test_emu_wide_rmsnorm_and_se_linear(emu):
    """The workgroup-per-row RMSNorm (C > 2048, several rows) and the K-split SE linear against torch."""
    from videollama2_amd import ops
    x, w = bf(5, 4096), 1 + 0.1 * torch.randn(4096)
    xf = x.float()
    ref = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5) * w
    assert rel(ops.rmsnorm(x, w, 1e-5), ref) < TOL_BF16_OUT
    g, wl, b = torch.randn(19, 4096), bf(24, 4096, scale=0.02), torch.randn(24)
    assert rel(ops.small_linear(g, wl, b, ops.ACT_SILU), F.silu(F.linear(g, wl.float(), b))) < 1e-5
    g2, wl2 = torch.randn(3, 1024), bf(40, 1024, scale=0.03)
    assert rel(ops.small_linear(g2, wl2, None, ops.ACT_SIGMOID), torch.sigmoid(F.linear(g2, wl2.float()))) < 1e-5


@pytest.mark.parametrize("Fr,H,W,C", [(2, 5, 13, 512), (1, 3, 6, 4096), (1, 2, 1, 256), (2, 3, 18, 512), (1, 2, 16, 4096), (1, 1, 17, 8192), (1, 2, 3, 8192)])
def test_emu_dwconv_ln_silu_odd_grids(emu, Fr, H, W, C):
    """Depthwise 3x3 + LayerNorm2d + SiLU on grids other than the square 24x24 / 13x13 of the workload: non-square, a single
    column, both row edges in every frame; W >= 16 takes the four-positions-per-workgroup kernel (18 = 4 groups + 2)."""
    import torch.nn.functional as F
    from videollama2_amd import ops
    x = bf(Fr * H * W, C)
    wt = (torch.randn(C, 1, 3, 3, generator=torch.Generator().manual_seed(3)) * 0.3).bfloat16().float()
    lnw, lnb = torch.randn(C, generator=torch.Generator().manual_seed(4)), torch.randn(C, generator=torch.Generator().manual_seed(5))
    y = ops.dwconv3x3_ln_silu(x, wt.view(C, 9).t().contiguous(), lnw, lnb, Fr, H, W)
    ref = F.conv2d(x.float().view(Fr, H, W, C).permute(0, 3, 1, 2), wt, padding=1, groups=C).permute(0, 2, 3, 1)
    ref = F.silu(F.layer_norm(ref, (C,), lnw, lnb, 1e-5)).reshape(Fr * H * W, C)
    assert rel(y, ref) < TOL_BF16_OUT


@pytest.mark.parametrize("Fr,H,W,C,rd", [(2, 5, 13, 512, 128), (1, 3, 6, 4096, 1024), (1, 2, 1, 256, 64), (2, 3, 18, 512, 48), (3, 24, 24, 128, 32), (1, 2, 3, 8192, 2048)])
def test_emu_dwconv_strip_squeeze_and_fused_excite(emu, Fr, H, W, C, rd):
    """The strip form of the depthwise kernel (taps in LDS, persistent teams, SE squeeze folded in) against the per-position forms, and the
    one-launch excite + scale against small_linear + se_scale.  24x24 is the s1 grid (64 teams per frame, 3 units each)."""
    from videollama2_amd import ops
    x = bf(Fr * H * W, C)
    wt = (torch.randn(C, 1, 3, 3, generator=torch.Generator().manual_seed(3)) * 0.3).bfloat16().float()
    lnw, lnb = torch.randn(C, generator=torch.Generator().manual_seed(4)), torch.randn(C, generator=torch.Generator().manual_seed(5))
    w9c = wt.view(C, 9).t().contiguous()
    y0 = ops.dwconv3x3_ln_silu(x, w9c, lnw, lnb, Fr, H, W)
    y, m = ops.dwconv3x3_ln_silu_mean(x, w9c, lnw, lnb, Fr, H, W)
    if W >= 16:
        assert torch.equal(y, y0)                     # same fmaf chain as the four-position kernel
    else:
        assert rel(y, y0) < 2e-3
    assert rel(m, y.float().view(Fr, H * W, C).mean(1)) < 1e-5
    if Fr > 1:                                        # a frame's bits do not depend on how many frames the launch holds
        y1, m1 = ops.dwconv3x3_ln_silu_mean(x[H * W:2 * H * W].contiguous(), w9c, lnw, lnb, 1, H, W)
        assert torch.equal(y1, y[H * W:2 * H * W]) and torch.equal(m1, m[1:2])
    w1, b1 = bf(rd, C, scale=C ** -0.5), torch.randn(rd) * 0.1
    w2, b2 = bf(C, rd, scale=rd ** -0.5), torch.randn(C) * 0.1
    g1 = ops.small_linear(m, w1, b1, ops.ACT_SILU)
    ya = ops.se_scale_(y.clone(), ops.small_linear(g1, w2, b2, ops.ACT_SIGMOID), Fr, H * W)
    yb = ops.se_excite_scale_(y.clone(), g1, w2, b2, Fr, H * W)
    gate = torch.sigmoid(F.linear(g1, w2.float(), b2))
    assert rel(yb.view(Fr, H * W, C), y.float().view(Fr, H * W, C) * gate[:, None, :]) < TOL_BF16_OUT
    assert rel(yb, ya) < 1e-3 and (yb != ya).float().mean() < 0.02      # the two differ only where a gate's last fp32 bit moves a bf16 rounding


def test_emu_attention_ragged_and_causal(emu):
    from videollama2_amd import ops
    B, H, N, D = 2, 2, 150, 64
    qkv = bf(B * N, 3 * H * D)
    o = torch.zeros(B * N, H * D, dtype=torch.bfloat16)
    st = (N * 3 * H * D, D, 3 * H * D)
    ops.attn_fwd(qkv, qkv[:, H * D:], qkv[:, 2 * H * D:], o, st, st, st, (N * H * D, D, H * D), B, H, N, N, 1, D ** -0.5, False, 0, D)
    q, k, v = [t.view(B, N, H, D).transpose(1, 2).float() for t in qkv.view(B * N, 3, H * D).unbind(1)]
    ref = (torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, -1) @ v).transpose(1, 2).reshape(B * N, H * D)
    assert rel(o, ref) < TOL_BF16_OUT
    S, nh, nkv, D, smax = 200, 4, 2, 128, 256
    q, kc, vc = bf(S, nh * D), bf(nkv, smax, D), bf(nkv, smax, D, seed=1)
    o = torch.zeros(S, nh * D, dtype=torch.bfloat16)
    args = ((0, D, nh * D), (0, smax * D, D), (0, smax * D, D), (0, D, nh * D), 1, nh)
    ops.attn_fwd(q, kc, vc, o, *args, S, S, nh // nkv, D ** -0.5, True, 0, D)
    qf = q.view(S, nh, D).transpose(0, 1).float()
    kf, vf = kc[:, :S].float().repeat_interleave(2, 0), vc[:, :S].float().repeat_interleave(2, 0)
    sc = (qf @ kf.transpose(1, 2) * D ** -0.5).masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
    ref = (torch.softmax(sc, -1) @ vf).transpose(0, 1).reshape(S, nh * D)
    assert rel(o, ref) < TOL_BF16_OUT
    # head_dim 96 (SigLIP's 72 zero-padded): non-causal, ragged N, real scale = 72^-0.5
    B, H, N, D = 1, 2, 150, 96
    qkv = bf(B * N, 3 * H * D)
    qkv.view(B * N, 3 * H, D)[:, :, 72:] = 0
    o = torch.zeros(B * N, H * D, dtype=torch.bfloat16)
    st = (N * 3 * H * D, D, 3 * H * D)
    ops.attn_fwd(qkv, qkv[:, H * D:], qkv[:, 2 * H * D:], o, st, st, st, (N * H * D, D, H * D), B, H, N, N, 1, 72 ** -0.5, False, 0, D)
    q9, k9, v9 = [t.view(B, N, H, D).transpose(1, 2).float() for t in qkv.view(B * N, 3, H * D).unbind(1)]
    ref96 = (torch.softmax(q9 @ k9.transpose(-1, -2) * 72 ** -0.5, -1) @ v9).transpose(1, 2).reshape(B * N, H * D)
    assert rel(o, ref96) < TOL_BF16_OUT and o.view(B * N, H, D)[:, :, 72:].abs().max() == 0
    S, nh, nkv, D, smax = 200, 4, 2, 128, 256
    o2 = torch.zeros(40, nh * D, dtype=torch.bfloat16)          # 40 new rows against 200 keys (chunked prefill form)
    ops.attn_fwd(q[160:].contiguous(), kc, vc, o2, *args, 40, S, nh // nkv, D ** -0.5, True, 160, D)
    assert rel(o2, ref[160:]) < TOL_BF16_OUT


def test_emu_attention_class_token_peel(emu):
    """csrc/k_attn2.h CLS = true (the automatic choice for full attention over 1 + 64 n tokens, head_dim 64 = the CLIP tower's 577): the
    class token's key as the initial online-softmax state, its query in a workgroup of its own, the tiles over the patch rows only.  Same
    result as the plain tiling (variant 3) and as torch; fused-qkv strides, several frames / heads, 1 + 64 / 1 + 192 / 1 + 576 tokens, a
    softmax spike ON the class key (its state must rescale) and on a patch key (the class state must be rescaled by a later tile)."""
    from videollama2_amd import ops
    D = 64
    try:
        for B, H, N in ((2, 2, 65), (1, 3, 193), (1, 2, 129), (2, 2, 577)):     # 129: the last query block is full -> an extra block for the class query
            qkv = bf(B * N, 3 * H * D, seed=N)
            qkv[5, :D] = 4.0
            qkv[0, H * D:H * D + D] = 4.0              # row 5's query loves the class key of frame 0 (head 0)
            qkv[9, :D] = -4.0
            qkv[N - 3, H * D:H * D + D] = -4.0         # row 9's query loves a late patch key
            st = (N * 3 * H * D, D, 3 * H * D)
            outs = {}
            for var in (3, 0):
                ops.set_attn_kv_groups(var)
                outs[var] = torch.zeros(B * N, H * D, dtype=torch.bfloat16)
                ops.attn_fwd(qkv, qkv[:, H * D:], qkv[:, 2 * H * D:], outs[var], st, st, st, (N * H * D, D, H * D), B, H, N, N, 1, D ** -0.5, False, 0, D)
            q, k, v = [t.view(B, N, H, D).transpose(1, 2).float() for t in qkv.view(B * N, 3, H * D).unbind(1)]
            ref = (torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, -1) @ v).transpose(1, 2).reshape(B * N, H * D)
            assert rel(outs[0], ref) < TOL_BF16_OUT and rel(outs[0], outs[3]) < 3e-3, (B, H, N)
            cls_rows = torch.arange(B) * N                                 # the class queries themselves (the one-row workgroups)
            assert rel(outs[0][cls_rows], ref[cls_rows]) < TOL_BF16_OUT, (B, H, N)
    finally:
        ops.set_attn_kv_groups(0)


def test_emu_attention_second_structure(emu):
    """csrc/k_attn2.h (vl2_attn_fwd variant 3): K/V tiles by LDS-DMA into a two-stage ring, V through transpose reads.  Same
    cases as the first structure -- ragged non-causal D = 64 out of a fused qkv buffer, causal GQA D = 128 from the KV cache,
    1..6 KV tiles (odd and even: both stages, both loop exits), chunked-prefill offset, a softmax spike -- against torch, and
    against the first structure (same arithmetic: equal up to fp32 summation order inside the MFMA chains)."""
    from videollama2_amd import ops

    def both(fn, shape):
        outs = []
        for var in (1, 3, 4):
            ops.set_attn_kv_groups(var)
            o = torch.zeros(shape, dtype=torch.bfloat16)
            fn(o)
            outs.append(o)
        # variant 4 = variant 3 with two key streams per query block (even / odd tiles, merged in fp32 through LDS): same tolerance
        # against torch is checked by the callers through o3; here: it agrees with the one-stream form to the rounding of P (each stream rounds exp2(s - its own running maximum) to 16 bits)
        assert rel(outs[2], outs[1]) < 3e-3, rel(outs[2], outs[1])
        both.last4 = outs[2]
        return outs[:2]

    try:
        for B, H, N, D in ((2, 2, 150, 64), (1, 1, 64, 64), (1, 3, 577, 64), (1, 2, 130, 128)):
            qkv = bf(B * N, 3 * H * D, seed=N)
            st = (N * 3 * H * D, D, 3 * H * D)
            o1, o3 = both(lambda o: ops.attn_fwd(qkv, qkv[:, H * D:], qkv[:, 2 * H * D:], o, st, st, st, (N * H * D, D, H * D), B, H, N, N, 1,
                                                 D ** -0.5, False, 0, D), (B * N, H * D))
            q, k, v = [t.view(B, N, H, D).transpose(1, 2).float() for t in qkv.view(B * N, 3, H * D).unbind(1)]
            ref = (torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5, -1) @ v).transpose(1, 2).reshape(B * N, H * D)
            assert rel(both.last4, ref) < TOL_BF16_OUT and rel(o3, ref) < TOL_BF16_OUT and rel(o3, o1) < 3e-3, (B, H, N, D)
        nh, nkv, D, smax = 4, 2, 128, 384
        for S in (60, 130, 200, 330):
            q, kc, vc = bf(S, nh * D, seed=S), bf(nkv, smax, D, seed=S + 1), bf(nkv, smax, D, seed=S + 2)
            args = ((0, D, nh * D), (0, smax * D, D), (0, smax * D, D), (0, D, nh * D), 1, nh)
            o1, o3 = both(lambda o: ops.attn_fwd(q, kc, vc, o, *args, S, S, nh // nkv, D ** -0.5, True, 0, D), (S, nh * D))
            qf = q.view(S, nh, D).transpose(0, 1).float()
            kf, vf = kc[:, :S].float().repeat_interleave(2, 0), vc[:, :S].float().repeat_interleave(2, 0)
            sc = (qf @ kf.transpose(1, 2) * D ** -0.5).masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
            ref = (torch.softmax(sc, -1) @ vf).transpose(0, 1).reshape(S, nh * D)
            assert rel(both.last4, ref) < TOL_BF16_OUT and rel(o3, ref) < TOL_BF16_OUT and rel(o3, o1) < 3e-3, S
            if S == 200:                                              # 40 new rows against 200 keys (chunked prefill form)
                _, o2 = both(lambda o: ops.attn_fwd(q[160:].contiguous(), kc, vc, o, *args, 40, S, nh // nkv, D ** -0.5, True, 160, D), (40, nh * D))
                assert rel(o2, ref[160:]) < TOL_BF16_OUT and rel(both.last4, ref[160:]) < TOL_BF16_OUT
        # causal D = 64 (not used by the models, built for completeness) and the rescale branch (guide rule 26)
        N, D = 300, 64
        qkv = bf(N, 3 * D, seed=7)
        qkv[17, :D] = 6.0
        qkv[250, D:2 * D] = 6.0
        st = (N * 3 * D, D, 3 * D)
        _, o3 = both(lambda o: ops.attn_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], o, st, st, st, (N * D, D, D), 1, 1, N, N, 1, D ** -0.5, False, 0, D), (N, D))
        q, k, v = [t.float() for t in qkv.view(N, 3, D).unbind(1)]
        ref = torch.softmax(q @ k.T * D ** -0.5, -1) @ v
        assert rel(both.last4, ref) < TOL_BF16_OUT and rel(o3, ref) < TOL_BF16_OUT and rel(o3[17], ref[17]) < 1e-2
        _, o3 = both(lambda o: ops.attn_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], o, st, st, st, (N * D, D, D), 1, 1, N, N, 1, D ** -0.5, True, 0, D), (N, D))
        sc = (q @ k.T * D ** -0.5).masked_fill(torch.triu(torch.ones(N, N, dtype=torch.bool), 1), float("-inf"))
        assert rel(o3, torch.softmax(sc, -1) @ v) < TOL_BF16_OUT and rel(both.last4, torch.softmax(sc, -1) @ v) < TOL_BF16_OUT
    finally:
        ops.set_attn_kv_groups(0)


def test_emu_causal_attention_kv_groups(emu):
    """Causal D=128 attention with one and with two KV groups per workgroup (the second group takes every other KV tile; the
    partial (m, l, O) are merged through LDS): 1, 3, 4 and 6 KV tiles, so that the second group has none / fewer / as many."""
    from videollama2_amd import ops
    nh, nkv, D, smax = 4, 2, 128, 384
    try:
        for S in (60, 130, 200, 330):
            q, kc, vc = bf(S, nh * D, seed=S), bf(nkv, smax, D, seed=S + 1), bf(nkv, smax, D, seed=S + 2)
            args = ((0, D, nh * D), (0, smax * D, D), (0, smax * D, D), (0, D, nh * D), 1, nh)
            qf = q.view(S, nh, D).transpose(0, 1).float()
            kf, vf = kc[:, :S].float().repeat_interleave(2, 0), vc[:, :S].float().repeat_interleave(2, 0)
            sc = (qf @ kf.transpose(1, 2) * D ** -0.5).masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
            ref = (torch.softmax(sc, -1) @ vf).transpose(0, 1).reshape(S, nh * D)
            outs = []
            for groups in (1, 2):
                ops.set_attn_kv_groups(groups)
                o = torch.zeros(S, nh * D, dtype=torch.bfloat16)
                ops.attn_fwd(q, kc, vc, o, *args, S, S, nh // nkv, D ** -0.5, True, 0, D)
                assert rel(o, ref) < TOL_BF16_OUT, (S, groups)
                outs.append(o)
            assert rel(outs[0], outs[1]) < 5e-3          # same math, partial sums merged in a different order
            # rows above the diagonal of the second group's first tile meet only masked keys there: whatever the rounding of
            # (-1e30 * scale), their weight must come out 0, never 2^(+residue) = inf
            for scale in (0.05, 0.0713, 0.1, 0.131):
                o = torch.zeros(S, nh * D, dtype=torch.bfloat16)
                ops.attn_fwd(q, kc, vc, o, *args, S, S, nh // nkv, scale, True, 0, D)
                sc2 = (qf @ kf.transpose(1, 2) * scale).masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
                ref2 = (torch.softmax(sc2, -1) @ vf).transpose(0, 1).reshape(S, nh * D)
                assert torch.isfinite(o.float()).all() and rel(o, ref2) < TOL_BF16_OUT, (S, scale)
    finally:
        ops.set_attn_kv_groups(0)


def test_emu_small_config_end_to_end_vs_reference_goldens(emu, golden_small):
    from videollama2_amd.model import VideoLLaMA2Hip
    g = golden_small
    cfg = g["cfg"]
    sd = O.seeded_state_dict(cfg, g["seed"])
    m = VideoLLaMA2Hip(cfg, sd, "cpu", max_seq_len=64)
    tower = m.vision_tower(g["frames"])
    assert rel(tower, g["tower_out"]) < 1.2e-2                       # reference's own bf16 floor here is ~1e-2
    out, st = m.mm_projector(tower.view(1, *tower.shape), return_stages=True)
    assert rel(st["s1"].permute(0, 3, 1, 2), g["stc_s1"]) < 2e-2
    assert rel(st["sampler"].permute(3, 0, 1, 2)[None], g["stc_sampler"]) < 2e-2
    assert rel(out, g["mm_features"]) < 2.5e-2
    ids = g["input_ids"][None]
    toks, logits = m.generate(ids, images=[(g["frames"], "video")], do_sample=False, max_new_tokens=3,
                              attention_mask=torch.ones_like(ids), return_logits=True)
    assert toks[0].tolist() == g["new_tokens"][:3].tolist()
    assert rel(logits, g["step_logits"][:3]) < 2.5e-2
    with pytest.raises(NotImplementedError):
        m.generate(ids, images=None, inputs_embeds=torch.zeros(1))
    with pytest.raises(ValueError, match="doesn't match model"):
        m.vision_tower(torch.zeros(1, 3, 28, 28))


def test_emu_v21_family_end_to_end_vs_reference_goldens(emu, golden_small_v21):
    """VideoLLaMA2.1 family (SigLIP tower with padded heads / MLP, unpadded v35 sampler, Qwen2 decoder with q/k/v bias and an
    odd GQA group) against goldens minted from the real reference."""
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.tower import HipSiglipVisionTower
    g = golden_small_v21
    cfg = g["cfg"]
    sd = O.seeded_state_dict(cfg, g["seed"])
    m = VideoLLaMA2Hip(cfg, sd, "cpu", max_seq_len=64)
    assert isinstance(m.vision_tower, HipSiglipVisionTower) and m.mm_projector.padding == 0
    assert m.vision_tower.w["hd"] == 32 and m.vision_tower.w["hdp"] == 64 and m.vision_tower.w["layers"][0]["w1"].shape[0] == 256
    tower = m.vision_tower(g["frames"])
    assert tuple(tower.shape) == tuple(g["tower_out"].shape) and rel(tower, g["tower_out"]) < 1.2e-2
    out, st = m.mm_projector(tower.view(1, *tower.shape), return_stages=True)
    assert rel(st["sampler"].permute(3, 0, 1, 2)[None], g["stc_sampler"]) < 2e-2
    assert rel(out, g["mm_features"]) < 2.5e-2
    ids = g["input_ids"][None]
    toks, logits = m.generate(ids, images=[(g["frames"], "video")], do_sample=False, max_new_tokens=3,
                              attention_mask=torch.ones_like(ids), return_logits=True)
    assert toks[0].tolist() == g["new_tokens"][:3].tolist()
    assert rel(logits, g["step_logits"][:3]) < 2.5e-2


@pytest.mark.parametrize("family", ["v2", "v21"])
def test_emu_drop_in_accelerate_reference_model(emu, golden_small, golden_small_v21, family):
    """The seam test: a live reference model (build container only; Videollama2MistralForCausalLM and the VideoLLaMA2.1
    Videollama2Qwen2ForCausalLM) re-routed by install.accelerate(); the reference's own `encode_images_or_videos` and
    `generate` entry points then run on the HIP host path (emulated kernels here)."""
    from oracle import ref_harness as RH
    if not RH.reference_available():
        pytest.skip("reference tree only exists in the build container")
    from videollama2_amd.install import accelerate
    g = golden_small if family == "v2" else golden_small_v21
    model, _ = RH.build_reference_model(g["cfg"])
    RH.reseed_weights(model, g["seed"])
    accelerate(model, device="cpu", max_seq_len=64)
    feats = model.encode_images_or_videos([(g["frames"], "video")])          # reference method, HIP modules underneath
    assert rel(feats, g["mm_features"]) < 2.5e-2
    ids = g["input_ids"][None]
    out = model.generate(ids, attention_mask=torch.ones_like(ids), images=[(g["frames"], "video")], do_sample=False,
                         max_new_tokens=2, use_cache=True, pad_token_id=0, eos_token_id=None)
    assert out[0].tolist() == g["new_tokens"][:2].tolist()


@pytest.mark.parametrize("family", ["v2", "v21"])
def test_emu_uint8_frame_ingest_matches_process_video(emu, golden_small, golden_small_v21, family):
    """uint8 ingest: raw uint8 [T,H,W,3] frames through `process_video_u8` + the in-register normalise of
    the patch-row kernel give the tower output of the fp32 `process_video` path (reciprocal instead of division: identical up
    to rare bf16 rounding ties)."""
    from videollama2_amd.mm_utils import process_video, process_video_u8
    from videollama2_amd.tower import (HipCLIPVisionTower, HipSiglipVisionTower, default_image_processor,
                                       default_siglip_image_processor)
    g = golden_small if family == "v2" else golden_small_v21
    cfg = g["cfg"]
    S = cfg["vision"]["image_size"]
    siglip = O.vision_family(cfg) == "siglip"
    proc = (default_siglip_image_processor if siglip else default_image_processor)(S)
    sd = O.seeded_state_dict(cfg, g["seed"], only=lambda n: "vision_tower" in n)
    tower = (HipSiglipVisionTower if siglip else HipCLIPVisionTower)(cfg, sd, "cpu", image_processor=proc)
    u8 = g["frames_u8"].numpy()
    ref_frames = process_video(u8, proc, aspect_ratio=None, num_frames=u8.shape[0])
    assert torch.allclose(ref_frames, g["frames"], atol=1e-6)                      # the mirror reproduces the reference's frames
    raw = process_video_u8(u8, proc, aspect_ratio=None, num_frames=u8.shape[0])
    assert raw.dtype == torch.uint8 and tuple(raw.shape) == (u8.shape[0], S, S, 3) and torch.equal(raw, g["frames_u8"])
    from videollama2_amd import ops
    P, kp = cfg["vision"]["patch_size"], tower.w["kp"]
    rows_f = ops.patchify(ref_frames, P, kp)                                      # fp32 frames -> bf16 patch rows
    rows_u = ops.patchify_u8(raw, P, kp, proc.rescale_factor, proc.image_mean, proc.image_std)
    same = (rows_f == rows_u).float().mean().item()
    ulp = (rows_f.float() - rows_u.float()).abs() / rows_f.float().abs().clamp_min(1e-3)
    assert same > 0.99 and ulp.max().item() <= 2 ** -7, (same, ulp.max().item())    # at most one bf16 ulp, on rounding ties only
    a = tower(ref_frames.bfloat16())
    b = tower(raw)
    assert b.dtype == torch.bfloat16 and a.shape == b.shape
    assert rel(b, a.float()) < 1e-2                                                # a few flipped input ulps -> bf16 noise floor
    odd = g["odd_u8"].numpy()                                                       # non-square, bicubic resize + crop on the host
    ro = process_video_u8([f for f in odd], proc, aspect_ratio=None, num_frames=4)
    fo = process_video([f for f in odd], proc, aspect_ratio=None, num_frames=4)
    assert tuple(ro.shape) == (4, S, S, 3)
    assert rel(tower(ro), tower(fo.bfloat16()).float()) < 2e-2


@pytest.mark.parametrize("family", ["v2", "v21"])
def test_emu_install_patches_factories_and_loader(emu, golden_small, golden_small_v21, family, tmp_path, monkeypatch):
    """install.install(): the reference's own FACTORIES return HIP modules and its loader returns the HIP model.
    (1) `Videollama2{Mistral,Qwen2}ForCausalLM(config)` built by the unmodified reference class after install(): its vision
        tower / projector come from the patched build_vision_tower / build_vision_projector, host the reference's state-dict keys
        (strict load of the seeded weights), hold no HF / timm module, and the reference's own encode_images_or_videos /
        generate reproduce the goldens (HF decoder on top of the HIP encoder).
    (2) `videollama2.model_init(checkpoint dir)` + `videollama2.mm_infer(...)` (videollama2/__init__.py:14-114, unmodified) on a
        synthetic safetensors checkpoint: `load_pretrained_model` gets the HIP model from the patched loader class."""
    from oracle import ref_harness as RH
    if not RH.reference_available():
        pytest.skip("reference tree only exists in the build container")
    import json
    from safetensors.torch import save_file
    from videollama2_amd import api, install
    from videollama2_amd.lazy import LazyHipSTCConnector, LazyHipVisionTower
    from videollama2_amd.model import VideoLLaMA2Hip
    g = golden_small if family == "v2" else golden_small_v21
    cfg = g["cfg"]
    ref = RH.import_reference()
    install.install(device="cpu", max_seq_len=160)
    try:
        # ---- (1) factories
        model, _ = RH.build_reference_model(cfg)
        inner = model.get_model()
        assert isinstance(inner.vision_tower, LazyHipVisionTower) and isinstance(inner.mm_projector, LazyHipSTCConnector)
        assert not any(type(m).__name__.startswith(("CLIPVision", "SiglipVision", "RegStage")) for m in model.modules())
        RH.reseed_weights(model, g["seed"])                                  # strict load: the keys are the reference's
        feats = model.encode_images_or_videos([(g["frames"], "video")])      # reference method, HIP modules underneath
        assert rel(feats, g["mm_features"]) < 2.5e-2
        assert inner.vision_tower.vision_tower is None and not list(inner.mm_projector.parameters())   # packed once, hosts released
        ids = g["input_ids"][None]
        out = model.generate(ids, attention_mask=torch.ones_like(ids), images=[(g["frames"], "video")], do_sample=False,
                             max_new_tokens=2, use_cache=True, pad_token_id=0, eos_token_id=None)
        assert out[0].tolist() == g["new_tokens"][:2].tolist()
        # ---- (2) loader: the reference's model_init / mm_infer on a synthetic checkpoint directory
        v, l = cfg["vision"], cfg["llm"]
        sd = {k: t.bfloat16().contiguous() for k, t in O.seeded_state_dict(cfg, g["seed"]).items()}
        save_file(sd, str(tmp_path / "model.safetensors"))
        hf = dict(model_type="videollama2_qwen2" if O.llm_family(cfg) == "qwen2" else "videollama2_mistral",
                  hidden_size=l["hidden_size"], intermediate_size=l["intermediate_size"], num_hidden_layers=l["num_hidden_layers"],
                  num_attention_heads=l["num_attention_heads"], num_key_value_heads=l["num_key_value_heads"], head_dim=l["head_dim"],
                  vocab_size=l["vocab_size"], rms_norm_eps=l["rms_norm_eps"], rope_theta=l["rope_theta"], num_frames=4,
                  mm_vision_tower="somewhere/" + ("siglip-synthetic" if O.vision_family(cfg) == "siglip" else "clip-synthetic"),
                  mm_projector_type=cfg.get("projector", "stc_connector"), mm_vision_select_layer=v["select_layer"])
        json.dump(hf, open(tmp_path / "config.json", "w"))
        json.dump({k: v[k] for k in v if k != "select_layer"}, open(tmp_path / "vision_config.json", "w"))
        tok = _ToyTokenizer(l["vocab_size"])
        import videollama2.model as vm
        monkeypatch.setattr(vm.AutoTokenizer, "from_pretrained", classmethod(lambda cls, *a, **k: tok))   # no tokenizer files on the box
        hip, processor, tok2 = ref.model_init(str(tmp_path), device_map={"": "cpu"})
        assert isinstance(hip, VideoLLaMA2Hip) and tok2 is tok and set(processor) == {"image", "video"}
        frames = processor["video"](g["frames_u8"].numpy())
        assert torch.allclose(frames, g["frames"], atol=1e-6)
        monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)          # mm_infer does tensor.half().cuda(): no GPU here
        text = ref.mm_infer(frames, "what happens in the clip ?", hip, tok, modal="video", max_new_tokens=4)
        mine = api.mm_infer(frames, "what happens in the clip ?", hip, tok, modal="video", max_new_tokens=4)
        assert len(text) > 0 and text == mine
    finally:
        install.uninstall()
    assert ref.model.encoder.build_vision_tower.__module__ == "videollama2.model.encoder"


from tests.util import ToyTokenizer as _ToyTokenizer, write_synthetic_checkpoint  # noqa: E402


@pytest.mark.parametrize("family", ["v2", "v21"])
def test_emu_standalone_model_init_and_mm_infer(emu, golden_small, golden_small_v21, family, tmp_path):
    """videollama2_amd.api: `model_init(local checkpoint dir)` + `mm_infer` (the reference's videollama2/__init__.py:14-114
    surface) on a synthetic safetensors checkpoint of each family."""
    import json
    from safetensors.torch import save_file
    from videollama2_amd import api
    g = golden_small if family == "v2" else golden_small_v21
    cfg = g["cfg"]
    v, l = cfg["vision"], cfg["llm"]
    sd = {k: t.bfloat16().contiguous() for k, t in O.seeded_state_dict(cfg, g["seed"]).items()}
    save_file(sd, str(tmp_path / "model.safetensors"))
    hf = dict(model_type="videollama2_qwen2" if O.llm_family(cfg) == "qwen2" else "videollama2_mistral",
              hidden_size=l["hidden_size"], intermediate_size=l["intermediate_size"], num_hidden_layers=l["num_hidden_layers"],
              num_attention_heads=l["num_attention_heads"], num_key_value_heads=l["num_key_value_heads"], head_dim=l["head_dim"],
              vocab_size=l["vocab_size"], rms_norm_eps=l["rms_norm_eps"], rope_theta=l["rope_theta"], num_frames=4,
              mm_vision_tower="somewhere/" + ("siglip-synthetic" if O.vision_family(cfg) == "siglip" else "clip-synthetic"),
              mm_projector_type=cfg.get("projector", "stc_connector"), mm_vision_select_layer=v["select_layer"])
    json.dump(hf, open(tmp_path / "config.json", "w"))
    json.dump({k: v[k] for k in v if k != "select_layer"}, open(tmp_path / "vision_config.json", "w"))
    got, _ = api.config_from_checkpoint(str(tmp_path))
    assert got["llm"] == {**l, "family": O.llm_family(cfg)} and got["projector"] == cfg.get("projector", "stc_connector")
    assert got["vision"] == {**v, "family": O.vision_family(cfg)}
    tok = _ToyTokenizer(l["vocab_size"])
    model, processor, tok2 = api.model_init(str(tmp_path), device="cpu", max_seq_len=160, tokenizer=tok)
    assert tok2.pad_token == "<unk>" and set(processor) == {"image", "video"}
    frames = processor["video"](g["frames_u8"].numpy())
    assert torch.allclose(frames, g["frames"], atol=1e-6)
    text = api.mm_infer(frames, "what happens in the clip ?", model, tok, modal="video", max_new_tokens=4)
    roles = [m["role"] for m in tok.prompts[-1]]
    assert roles == (["system", "user"] if family == "v2" else ["user"])            # __init__.py:72-83
    assert tok.prompts[-1][-1]["content"].startswith("<video>\n")
    prompt = tok.apply_chat_template(tok.prompts[-1])
    ids = api.tokenizer_multimodal_token(prompt, tok, "<video>", return_tensors="pt")[None]
    assert (ids == -201).sum().item() == 1
    ref = model.generate(ids, attention_mask=torch.ones_like(ids), images=[(frames.half(), "video")], do_sample=False,
                         max_new_tokens=4, eos_token_id=2)                        # mm_infer uploads tensor.half() (__init__.py:60)
    assert text == tok.batch_decode(ref)[0].strip() and len(text) > 0
    with pytest.raises(ValueError, match="Unsupported modal"):
        api.mm_infer(frames, "x", model, tok, modal="audio")


def test_emu_padded_batch_generate_and_forward_with_images(emu, golden_small):
    """arch.py:227-261 + videollama2_mistral.py:63-108 on the HIP host path: a RIGHT-PADDED batch of two video prompts of
    different lengths through `generate(inputs, attention_mask, images=[...])` gives each sequence the tokens it gets alone
    (finished rows padded with pad_token_id), `forward(input_ids, images=)` returns the logits of every position (golden
    prefill logits of the real reference), and the spliced mask / embeds follow the reference's layout; the reference's own
    batch-2 generate on the same images (tests/golden/reference_checks.pt) is the cross-check."""
    from videollama2_amd.model import VideoLLaMA2Hip
    g = golden_small
    cfg = g["cfg"]
    sd = O.seeded_state_dict(cfg, g["seed"])
    m = VideoLLaMA2Hip(cfg, sd, "cpu", max_seq_len=96)
    idsA = g["input_ids"]
    idsB = torch.cat([idsA[:3], idsA[6:]])                                   # three text tokens shorter, sentinel kept
    assert (idsB == -201).sum() == 1
    L = idsA.numel()
    batch = torch.zeros((2, L), dtype=torch.long)
    batch[0] = idsA
    batch[1, :idsB.numel()] = idsB
    mask = torch.ones_like(batch)
    mask[1, idsB.numel():] = 0
    fr2 = torch.flip(g["frames"], dims=[0]).contiguous()                      # a second, different video
    images = [(g["frames"], "video"), (fr2, "video")]
    _, m2, _, emb, _ = m.prepare_inputs_labels_for_multimodal(batch, mask, None, None, images)
    n_vis = O.n_visual_tokens(cfg["num_frames"], 4)
    assert tuple(emb.shape) == (2, L - 1 + n_vis, cfg["llm"]["hidden_size"]) and tuple(m2.shape) == tuple(emb.shape[:2])
    assert m2[0].all() and int(m2[1].sum()) == idsB.numel() - 1 + n_vis and not m2[1, -3:].any()
    assert rel(emb[0], g["inputs_embeds"]) < 2.5e-2
    alone = [m.generate(idsA[None], attention_mask=torch.ones(1, L, dtype=torch.long), images=images[:1], max_new_tokens=3)[0].tolist(),
             m.generate(idsB[None], attention_mask=torch.ones(1, idsB.numel(), dtype=torch.long), images=images[1:], max_new_tokens=3)[0].tolist()]
    assert alone[0] == g["new_tokens"][:3].tolist()
    out = m.generate(batch, attention_mask=mask, images=images, max_new_tokens=3, pad_token_id=0, do_sample=False)
    assert out.shape == (2, 3) and out.tolist() == alone
    eos = alone[1][0]                                                         # sequence 1 stops at its first token -> padded with pad_token_id
    out = m.generate(batch, attention_mask=mask, images=images, max_new_tokens=3, pad_token_id=0, eos_token_id=eos)
    assert out[1].tolist() == [eos, 0, 0] and (out[0].tolist() == alone[0] or eos in alone[0])
    res = m(input_ids=idsA[None], attention_mask=torch.ones(1, L, dtype=torch.long), images=images[:1])
    assert tuple(res.logits.shape) == (1, L - 1 + n_vis, cfg["llm"]["vocab_size"]) and rel(res.logits[0], g["prefill_logits"]) < 2.5e-2
    with pytest.raises(NotImplementedError):
        m(input_ids=idsA[None], images=images[:1], labels=idsA[None])
    bad = mask.clone()
    bad[1, 2] = 0
    with pytest.raises(NotImplementedError, match="right-padded"):
        m.generate(batch, attention_mask=bad, images=images, max_new_tokens=2)
    with pytest.raises(ValueError, match="media input"):
        m.generate(batch, attention_mask=mask, images=images[:1], max_new_tokens=2)
    # the reference's own batch-2 generate (equal lengths) on these images, minted by oracle/make_golden.py (mint_reference_checks)
    ref = torch.load(os.path.join(ROOT, "tests", "golden", "reference_checks.pt"), weights_only=False)["v2_batch2_flipped_tokens"]
    both = torch.stack([idsA, idsA])
    ours = m.generate(both, attention_mask=torch.ones_like(both), images=images, max_new_tokens=3, pad_token_id=0)
    assert ours.tolist() == ref


@pytest.mark.parametrize("family", ["v2", "v21"])
def test_emu_stage_level_entry_points_equal_the_per_operator_path(emu, golden_small, golden_small_v21, family):
    """include/vl2hip.h stage-level entry points (vl2_vit_forward, vl2_stc_forward, vl2_llm_prefill, vl2_llm_decode_step): the layer loops run
    inside the library; their results must be bit-identical to the per-operator host loops of tower.py / decoder.py (same kernels,
    same order), for both families, float and uint8 frames."""
    from videollama2_amd import ops
    from videollama2_amd.model import VideoLLaMA2Hip
    g = golden_small if family == "v2" else golden_small_v21
    cfg = g["cfg"]
    m = VideoLLaMA2Hip(cfg, O.seeded_state_dict(cfg, g["seed"]), "cpu", max_seq_len=64)
    try:
        outs = {}
        for stage in (True, False):
            ops.STAGE_ABI = stage
            tower = m.vision_tower(g["frames"])
            tower_u8 = m.vision_tower(g["frames_u8"])
            vis = m.mm_projector(tower.unsqueeze(0))
            logits = m.decoder.prefill(g["inputs_embeds"]).clone()
            m.decoder.state.copy_(torch.tensor([m.decoder.pos - 1, 0], dtype=torch.int32))
            steps = []
            for _ in range(3):
                if stage:
                    d, _, ws = m.decoder._stage_desc()
                    ops.llm_decode_step(d, m.decoder.logits, m.decoder.tok, m.decoder.state, m.decoder.hist, m.decoder.partial, ws)
                else:
                    ops.argmax(m.decoder.logits, m.decoder.tok, m.decoder.hist, 0, m.decoder.state)
                    m.decoder._decode_kernels(dyn=True)
                steps.append((int(m.decoder.tok), m.decoder.logits.clone()))
            outs[stage] = (tower, tower_u8, logits, steps, m.decoder.state.clone(), m.decoder.hist[:3].clone(), vis)
        a, b = outs[True], outs[False]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        assert [t for t, _ in a[3]] == [t for t, _ in b[3]]         # (the golden step-0 margin is 4e-3: tokens are only compared between the paths)
        assert all(torch.equal(x[1], y[1]) for x, y in zip(a[3], b[3])) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])
        assert torch.equal(a[6], b[6]) and rel(a[6][0], g["mm_features"]) < 2.5e-2
        assert rel(a[0], g["tower_out"]) < 1.2e-2
        ops.STAGE_ABI = True
        ops.set_stage_flags(ops.STAGE_ROW_TICKET)                  # producer-side finalize of the row statistics (k_gemm.h gemm_rows_ticket): same bits
        assert torch.equal(m.vision_tower(g["frames"]), a[0]) and torch.equal(m.decoder.prefill(g["inputs_embeds"]), a[2])
        ops.set_stage_flags(ops.STAGE_NO_MFMA16)                   # gate/up WITHOUT the default's 16 x 16 x 32 matrix instruction (k_gemm9.h): other last bits on the GPU,
        l16 = m.decoder.prefill(g["inputs_embeds"]).clone()        # but the SAME bits from the C++ layer loop and the per-operator loop
        ops.STAGE_ABI = False
        assert torch.equal(m.decoder.prefill(g["inputs_embeds"]), l16) and torch.equal(l16, a[2])   # (the emulated MFMAs sum k in order: here even the default's bits)
        ops.STAGE_ABI = True
        ops.set_stage_flags(0)
        from videollama2_amd._lib import Vl2HipError
        d, _, ws = m.decoder._stage_desc()
        with pytest.raises(Vl2HipError, match="exceeds the KV cache"):
            ops.llm_prefill(d, torch.zeros(65, cfg["llm"]["hidden_size"], dtype=torch.bfloat16), m.decoder.logits)
    finally:
        ops.STAGE_ABI = True
        ops.set_stage_flags(0)


def test_emu_fp8_prefill_stage_equals_the_per_operator_path(emu, golden_small):
    """VL2_STAGE_PREFILL_FP8 (vl2_llm_prefill with the projections on the fp8 matrix pipe, W8A8): the C++ layer loop and decoder.prefill's
    per-operator loop issue the same kernels -> the same logits bit for bit; against the 16-bit prefill the difference is the format's
    (an OPTIONAL arithmetic): only bounded here."""
    from videollama2_amd import ops
    from videollama2_amd.decoder import HipMistralDecoder
    g = golden_small
    cfg = g["cfg"]
    keep = lambda n: n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))
    dec = HipMistralDecoder(cfg, O.seeded_state_dict(cfg, g["seed"], only=keep), "cpu", max_seq_len=64)
    l16 = dec.prefill(g["inputs_embeds"]).clone()
    dec.enable_fp8_prefill()
    try:
        outs = {}
        for stage in (True, False):
            ops.STAGE_ABI = stage
            outs[stage] = dec.prefill(g["inputs_embeds"]).clone()
        assert torch.equal(outs[True], outs[False])
        e = rel(outs[True], l16)
        print(f"[emu] small config: fp8 (W8A8) prefill logits vs 16-bit prefill rel-L2 {e:.3e}")
        assert 1e-4 < e < 0.3
        dec.enable_fp8_prefill(False)
        assert torch.equal(dec.prefill(g["inputs_embeds"]), l16)
    finally:
        ops.STAGE_ABI = True


def test_emu_gemv_batched_matches_single_row(emu):
    """Multi-row GEMV (batched decode): every row must equal the single-row kernel's result for that row, with the fused
    RMSNorm / bias / residual / SwiGLU variants, strided rows, and a batch that needs splitting."""
    from videollama2_amd import ops
    from videollama2_amd.weights import pack_gate_up
    K, N, MB = 512, 192, 5
    xbuf = bf(MB, K + 64)                     # strided rows
    x = xbuf[:, :K]
    w, nw, bias, res = bf(N, K, scale=K ** -0.5), 1 + 0.1 * torch.randn(K), torch.randn(N), bf(MB, N)
    for kw in (dict(), dict(norm_w=nw, eps=1e-5), dict(bias=bias, res=True), dict(norm_w=nw, out_f32=True)):
        use_res = kw.pop("res", False)
        got = ops.gemv_batched(w, x, res=res if use_res else None, **kw)
        for b in range(MB):
            one = ops.gemv(w, x[b].contiguous(), res=res[b].contiguous() if use_res else None, **kw)
            assert torch.equal(got[b], one), (kw, b)
    wg, wu = bf(128, K, scale=K ** -0.5), bf(128, K, scale=K ** -0.5, seed=1)
    wgu = pack_gate_up(wg, wu)
    got = ops.gemv_batched(wgu, x, norm_w=nw, swiglu=True)
    for b in range(MB):
        assert torch.equal(got[b], ops.gemv(wgu, x[b].contiguous(), norm_w=nw, swiglu=True))


def test_emu_batched_decode_equals_sequential(emu, golden_small_v21):
    """Batched decode: requests with different prompt lengths decoded together must give, request by
    request, exactly the tokens and logits of decoding them one at a time (a row of the multi-row GEMV / batched attention is
    bit-identical to the single-sequence kernels).  Qwen2 family: q/k/v bias, GQA group 3.  Decoder level (random prompt
    embeddings) plus text-only requests through the model-level API."""
    from videollama2_amd.model import VideoLLaMA2Hip
    g = golden_small_v21
    cfg = g["cfg"]
    sd = O.seeded_state_dict(cfg, g["seed"])
    m = VideoLLaMA2Hip(cfg, sd, "cpu", max_seq_len=64)
    dec, D = m.decoder, cfg["llm"]["hidden_size"]
    embeds = [bf(n, D, scale=0.5, seed=n) for n in (9, 5)]
    seq = [dec.generate(e, max_new_tokens=3, return_logits=True) for e in embeds]
    eos = seq[1][0][0, 1].item()                                             # request 1 stops at its 2nd token ...
    outs, blogits = dec.generate_batch(embeds, max_new_tokens=3, eos_token_id=eos, return_logits=True)
    assert outs[1].tolist() == seq[1][0][0, :2].tolist()
    n0 = len(outs[0])                                                        # ... request 0 runs on (unless it meets the same id)
    assert outs[0].tolist() == seq[0][0][0, :n0].tolist() and (n0 == 3 or outs[0][-1].item() == eos)
    for b in range(2):
        assert torch.equal(blogits[:, b], seq[b][1][:blogits.shape[0]]), b
    class _Streamer:                                                         # HF BaseStreamer protocol (put / end)
        def __init__(self):
            self.ids, self.ended = [], False

        def put(self, value):
            self.ids += value.flatten().tolist()

        def end(self):
            self.ended = True

    st = _Streamer()
    ids = torch.tensor([[1, 17, 99, 5]])
    got = m.generate(ids, images=None, do_sample=False, max_new_tokens=2, streamer=st)
    assert st.ended and st.ids == got[0].tolist()
    reqs = [(torch.tensor([[1, 17, 99, 5]]), None), (torch.tensor([1, 300, 4]), None)]
    got = m.generate_batch(reqs, max_new_tokens=1)
    for (ids, _), o in zip(reqs, got):
        ids = ids if ids.dim() == 2 else ids[None]
        assert o.tolist() == m.generate(ids, images=None, do_sample=False, max_new_tokens=1)[0].tolist()


def test_emu_gemm_skinny_all_epilogues(emu):
    """Skinny-M GEMM (batched decode, 5..64 rows): weights as the MFMA B operand straight from memory, x chunks in LDS, K split
    + ordered reduction -- against torch for every epilogue and M tile count."""
    from videollama2_amd import ops
    from videollama2_amd.weights import pack_gate_up
    for M, N, K in ((5, 128, 192), (16, 64, 64), (23, 192, 384), (64, 128, 256), (33, 64, 96)):
        a, w, bias, res = bf(M, K), bf(N, K, scale=K ** -0.5), torch.randn(N), bf(M, N)
        ref = a.float() @ w.float().T
        assert rel(ops.gemm_skinny(a, w, out_f32=True), ref) < TOL_F32_OUT, (M, N, K)
        assert rel(ops.gemm_skinny(a, w, bias=bias), ref + bias) < TOL_BF16_OUT
        assert rel(ops.gemm_skinny(a, w, res=res), ref + res.float()) < TOL_BF16_OUT
    a = bf(19, 256)
    wg, wu = bf(128, 256, scale=1 / 16), bf(128, 256, scale=1 / 16, seed=1)
    ref = F.silu(a.float() @ wg.float().T) * (a.float() @ wu.float().T)
    assert rel(ops.gemm_skinny(a, pack_gate_up(wg, wu), swiglu=True), ref) < TOL_BF16_OUT


def _fp8_dequant(q, scale):
    """e4m3fn bytes x power-of-two row scales -> the 16-bit weights they stand for (exact in bf16)"""
    return (q.view(torch.float8_e4m3fn).float() * scale[:, None]).to(torch.bfloat16)


def test_emu_gemm_skinny_fp8_equals_skinny_on_the_dequantised_weights(emu):
    """One skinny body behind both weight formats and one plan from N and K only: the fp8 output is gemm_skinny's on the dequantised weights
    bit for bit (mt = 1, 2, 4; every epilogue), and a row's bits do not depend on the other rows of the batch."""
    from videollama2_amd import ops
    from videollama2_amd.weights import pack_gate_up
    for M, N, K in ((5, 128, 192), (16, 64, 64), (23, 192, 384), (64, 128, 256), (33, 64, 96)):
        a, w, bias, res = bf(M, K), bf(N, K, scale=K ** -0.5), torch.randn(N), bf(M, N)
        q, sc = ops.quant_fp8(w)
        wd = _fp8_dequant(q, sc)
        for kw in (dict(), dict(out_f32=True), dict(bias=bias), dict(res=res), dict(bias=bias, res=res, out_f32=True)):
            got = ops.gemm_skinny_fp8(a, q, sc, **kw)
            assert torch.equal(got, ops.gemm_skinny(a, wd, **kw)), (M, N, K, sorted(kw))
            for m in (1, M // 2 + 1):                                         # fewer rows (another mt where M > 16): the same bits per row
                sub = {k: (v[:m] if k == "res" else v) for k, v in kw.items()}
                assert torch.equal(ops.gemm_skinny_fp8(a[:m], q, sc, **sub), got[:m]), (M, N, K, m, sorted(kw))
    for M in (7, 19, 40):
        a, res = bf(M, 256), bf(M, 128)
        wgu = pack_gate_up(bf(128, 256, scale=1 / 16), bf(128, 256, scale=1 / 16, seed=1))
        q, sc = ops.quant_fp8(wgu)
        got = ops.gemm_skinny_fp8(a, q, sc, swiglu=True, res=res)
        assert torch.equal(got, ops.gemm_skinny(a, _fp8_dequant(q, sc), swiglu=True, res=res)), M
        assert torch.equal(ops.gemm_skinny_fp8(a[:3], q, sc, swiglu=True, res=res[:3]), got[:3]), M


def test_emu_gemv_batched_fp8_rows_equal_the_single_row_gemv(emu):
    """One fp8 GEMV body, MB a parameter: every row of a batched call (MB = 1..4 per launch, and a batch that is split) equals the single-row
    call bit for bit -- fused RMSNorm (weighted and plain), bias, residual, fp32 output, SwiGLU; strided rows; both NP forms (K <= 4096 / longer)."""
    from videollama2_amd import ops
    from videollama2_amd.weights import pack_gate_up
    for K, N in ((512, 192), (4352, 8)):
        xbuf = bf(6, K + 64)                      # strided rows
        w, nw, bias, resb = bf(N, K, scale=K ** -0.5), 1 + 0.1 * torch.randn(K), torch.randn(N), bf(6, N)
        q, sc = ops.quant_fp8(w)
        for MB in (1, 2, 3, 4, 6):
            x, res = xbuf[:MB, :K], resb[:MB]
            for kw in (dict(), dict(norm_w=nw, eps=1e-5), dict(rms_plain=True), dict(bias=bias, res=True), dict(norm_w=nw, out_f32=True)):
                kw = dict(kw)
                use_res = kw.pop("res", False)
                got = ops.gemv_batched_fp8(q, sc, x, res=res if use_res else None, **kw)
                for b in range(MB):
                    one = ops.gemv_fp8(q, sc, x[b].contiguous(), res=res[b].contiguous() if use_res else None, **kw)
                    assert torch.equal(got[b], one), (K, MB, sorted(kw), b)
    K = 512
    x, res = bf(5, K), bf(5, 128)
    q, sc = ops.quant_fp8(pack_gate_up(bf(128, K, scale=K ** -0.5), bf(128, K, scale=K ** -0.5, seed=1)))
    nw = 1 + 0.1 * torch.randn(K)
    for MB in (1, 2, 3, 4, 5):
        got = ops.gemv_batched_fp8(q, sc, x[:MB], norm_w=nw, swiglu=True, res=res[:MB])
        for b in range(MB):
            assert torch.equal(got[b], ops.gemv_fp8(q, sc, x[b].contiguous(), norm_w=nw, swiglu=True, res=res[b].contiguous())), (MB, b)


def test_emu_kv_cache_limits(emu, golden_small):
    """Maximum sizes: a prompt longer than the KV cache is refused, generation stops when the cache is full (the last token
    is produced from the logits of the last cache row), and a sequence that exactly fills the cache still prefills."""
    from videollama2_amd.decoder import HipMistralDecoder
    cfg = golden_small["cfg"]
    keep = lambda n: n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))
    sd = O.seeded_state_dict(cfg, golden_small["seed"], only=keep)
    dec = HipMistralDecoder(cfg, sd, "cpu", max_seq_len=16)
    D = cfg["llm"]["hidden_size"]
    with pytest.raises(ValueError, match="exceeds the KV cache"):
        dec.prefill(bf(17, D))
    out = dec.generate(bf(13, D, scale=0.5), max_new_tokens=100)
    assert out.shape == (1, 16 - 13 + 1) and dec.pos == 16
    with pytest.raises(ValueError, match="KV cache exhausted"):
        dec.decode_step()
    full = dec.generate(bf(16, D, scale=0.5), max_new_tokens=5)
    assert full.shape == (1, 1)


def test_emu_continuous_batching_admits_between_decode_steps(emu, golden_small):
    """serving.ContinuousBatcher (reference worker semantics serve/model_worker.py:263-300,350-352): requests
    arrive while others decode; each is prefilled into a free slot between two steps, retired at its own stop, and its tokens
    equal its solo greedy decode whatever else was in flight (multi-row GEMV rows are bit-identical to the single step)."""
    from videollama2_amd.model import VideoLLaMA2Hip
    g = golden_small
    cfg = g["cfg"]
    m = VideoLLaMA2Hip(cfg, O.seeded_state_dict(cfg, g["seed"]), "cpu", max_seq_len=96)
    idsA = g["input_ids"]
    idsB = torch.cat([idsA[:3], idsA[6:]])
    idsC = torch.cat([idsA[:2], idsA[5:]])
    fr2 = torch.flip(g["frames"], dims=[0]).contiguous()
    reqs = [(idsA, [(g["frames"], "video")], 5), (idsB, [(fr2, "video")], 2), (idsC, [(g["frames"], "video")], 4), (idsA[:4], None, 3)]
    solo = [m.generate(ids[None], attention_mask=torch.ones(1, ids.numel(), dtype=torch.long), images=im, max_new_tokens=n)[0].tolist()
            for ids, im, n in reqs]
    assert solo[0] == g["new_tokens"][:5].tolist()

    class Stream:
        def __init__(self):
            self.got, self.ended = [], False

        def put(self, t):
            self.got += t.flatten().tolist()

        def end(self):
            self.ended = True

    b = m.batcher(max_slots=2)
    st = [Stream() for _ in reqs]
    r0 = b.submit(reqs[0][0], reqs[0][1], max_new_tokens=reqs[0][2], streamer=st[0])
    r1 = b.submit(reqs[1][0], reqs[1][1], max_new_tokens=reqs[1][2], streamer=st[1])
    first = b.step()
    assert set(first) == {r0, r1} and first[r0] == solo[0][0] and first[r1] == solo[1][0]
    r2 = b.submit(reqs[2][0], reqs[2][1], max_new_tokens=reqs[2][2], streamer=st[2])      # both slots busy: waits
    r3 = b.submit(reqs[3][0], reqs[3][1], max_new_tokens=reqs[3][2], streamer=st[3])
    second = b.step()                                  # request 1 (2 tokens) finishes here and frees slot 1
    assert set(second) == {r0, r1} and st[1].ended and not st[0].ended and r1 in b.finished
    third = b.step()                                   # request 2 was admitted into slot 1 between the steps
    assert set(third) == {r0, r2} and third[r2] == solo[2][0]
    # the slot buffers are shared with generate_batch / a second batcher: while this batcher holds requests both are refused
    # (they would overwrite the caches and positions of the requests in flight), and allowed again once it has drained
    with pytest.raises(RuntimeError, match="in use by a ContinuousBatcher"):
        m.generate_batch([(reqs[0][0], reqs[0][1]), (reqs[1][0], reqs[1][1])], max_new_tokens=2)
    with pytest.raises(RuntimeError, match="in use by a ContinuousBatcher"):
        m.batcher(max_slots=2)
    done = b.run()
    assert [done[r].tolist() for r in (r0, r1, r2, r3)] == solo
    assert [s.got for s in st] == solo and all(s.ended for s in st)
    assert b.in_flight() == 0 and b.step() == {}
    again = m.generate_batch([(reqs[0][0], reqs[0][1]), (reqs[1][0], reqs[1][1])], max_new_tokens=2)     # drained: free again
    assert [o.tolist() for o in again] == [solo[0][:2], solo[1][:2]]
    # an EOS retires a request early; the slot is reused
    b2 = m.batcher(max_slots=1, eos_token_id=solo[0][1])
    ra = b2.submit(reqs[0][0], reqs[0][1], max_new_tokens=5)
    rb = b2.submit(reqs[3][0], None, max_new_tokens=3)
    out = b2.run()
    assert out[ra].tolist() == solo[0][:2] and out[rb].tolist()[:1] == solo[3][:1]


def check_pack_entry_points_against_weights_py(ops, dev):
    """include/vl2hip.h vl2_pack_* vs the tensor-op packing of videollama2_amd/weights.py on the same checkpoint-layout tensors:
    the re-laid-out weights byte for byte, the fp32 column sums / shifts to summation-order rounding.  Shared by the emulator
    test here and the GPU test (tests/test_gpu_ops.py)."""
    from videollama2_amd import weights as Wt
    g = torch.Generator().manual_seed(3)
    rb = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(torch.bfloat16).to(dev)
    N, K = 96, 320
    w, gam, beta, bias = rb(N, K, scale=K ** -0.5), (1 + 0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(dev), rb(K, scale=0.1), rb(N, scale=0.1)
    for b_, c_ in ((beta, bias), (beta, None), (None, None)):
        wp, s, t = ops.pack_fold_norm(w, gam, b_, c_)
        wp0, s0, t0 = Wt.fold_norm(w, gam, b_, c_, dev)
        assert torch.equal(wp, wp0) and torch.allclose(s, s0, rtol=0, atol=2e-5 * K ** 0.5)
        assert (t is None) == (t0 is None) and (t is None or torch.allclose(t, t0, rtol=0, atol=2e-5 * K ** 0.5))
    I, D = 128, 64
    gate, up = rb(I, D), rb(I, D)
    assert torch.equal(ops.pack_gate_up(gate, up), Wt.pack_gate_up(gate, up))
    w3 = rb(16, 24, 2, 2, 2)                                                   # Conv3d [Co, Ci, kt, kh, kw] (weights.pack_connector)
    assert torch.equal(ops.pack_permute(w3.reshape(16, 24, 8)).reshape(16, 8 * 24), w3.permute(0, 2, 3, 4, 1).reshape(16, 8 * 24).contiguous())
    dw = rb(40, 1, 3, 3)                                                        # depthwise [C, 1, 3, 3] -> [9][C] fp32 (_pack_bottleneck)
    assert torch.equal(ops.pack_permute(dw.reshape(1, 40, 9), out_f32=True)[0], dw.reshape(40, 9).t().float().contiguous())
    pw = rb(32, 588)                                                            # patch weight K 588 -> 640
    ref = torch.zeros((32, 640), dtype=torch.bfloat16, device=dev); ref[:, :588] = pw
    assert torch.equal(ops.pack_pad_rows(pw, 640), ref)
    q = rb(4 * 72, 40)                                                          # SigLIP heads 72 -> 96 rows: a "row" = one head's block
    ref = torch.zeros((4, 96, 40), dtype=torch.bfloat16, device=dev); ref[:, :72] = q.reshape(4, 72, 40)
    assert torch.equal(ops.pack_pad_rows(q.reshape(4, 72 * 40), 96 * 40).reshape(4 * 96, 40), ref.reshape(4 * 96, 40))
    v = rb(1000)
    assert torch.equal(ops.pack_cvt_f32(v), v.float())
    from videollama2_amd._lib import Vl2HipError
    with pytest.raises(Vl2HipError):
        ops.pack_gate_up(rb(48, 64)[:40], rb(48, 64)[:40])                      # I % 32 != 0


def test_emu_pack_entry_points_match_weights_py(emu):
    from videollama2_amd import ops
    check_pack_entry_points_against_weights_py(ops, "cpu")


def test_emu_parity_full_end_to_end_dry_run(emu):
    """CPU dry run of tests/test_gpu_parity_full.py::run_end_to_end (the configs[1] end-to-end chain: frames -> tower -> STC ->
    splice -> prefill -> teacher-forced decode + the free-running product generate) on the small config through the emulator, so
    that the GPU test's host logic is exercised where no GPU exists."""
    from tests import test_gpu_parity_full as PF
    saved = PF.DEV
    PF.DEV = "cpu"
    try:
        PF.FORCE_HF_FLOOR = True                                   # (exercise the HF-module floor pass of the full-depth GPU cases once on the CPU)
        try:
            PF.run_end_to_end(O.config_small(4), 4, 3, 256)
        finally:
            PF.FORCE_HF_FLOOR = False
        assert any("hf_modules_floor_rel_l2" in r for r in PF.RECORD), "the HF-module floor pass did not run"
        assert any(r.get("stage", "").startswith("e2e greedy tokens") for r in PF.RECORD)
        # second run of the same case: the seeded weights come back from the 16-bit copy (what the fp16-build test of the GPU suite does),
        # the fp32 truth from its cache, and the optional fp8-weights decode rows are appended
        n0 = len(PF.RECORD)
        PF.run_end_to_end(O.config_small(4), 4, 3, 256, fp8_decode=True)
        again = PF.RECORD[n0:]
        first = {r["stage"]: r.get("ours_rel_l2") for r in PF.RECORD[:n0] if "ours_rel_l2" in r}
        assert all(first[r["stage"]] == r["ours_rel_l2"] for r in again if r["stage"] in first)      # same weights -> same numbers
        assert any(r["stage"].startswith("fp8-weights decode:") for r in again)
        # massive-activation channels + shifted stream (ONE planted channel: the small config's streams are 64-256 wide, six channels
        # would be a tenth of it; the GPU test plants six in 1024 / 4096)
        PF.run_fp8_prefill_row(O.config_small(4), 70, 128)           # the W8A8 prefill against the truth of its own definition (oracle/fp8_oracle.py)
        assert any(r.get("stage", "").startswith("fp8 (W8A8) prefill logits") for r in PF.RECORD)
        PF.run_end_to_end(O.config_small(4), 4, 2, 256, mutate=lambda sd, cfg: PF.plant_outliers(sd, cfg, n_ch=1), tag="outliers ")
        assert any(r.get("stage", "").startswith("outliers e2e greedy tokens") for r in PF.RECORD)
    finally:
        PF.DEV = saved
        del PF.RECORD[:]


def test_emu_tensor_parallel_real_shards_in_one_process(emu):
    """dist.LocalTensorParallel (both ranks' shards in this process, partial sums added where the all-reduce sits) on the small
    decoder through the emulator: the CPU dry run of tests/test_gpu_tp.py."""
    from tests import test_gpu_tp as TP
    cfg = O.config_small(4)
    cfg["llm"].update(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, intermediate_size=512)   # 2 kv heads: TP = 2
    keep = lambda n: n.startswith(("model.layers.", "model.norm", "model.embed_tokens", "lm_head"))
    sd = O.seeded_state_dict(cfg, 21, only=keep)
    x = (torch.randn(37, 512, generator=torch.Generator().manual_seed(3)) * 0.5).bfloat16().float()
    with torch.no_grad():
        toks, lg = O.greedy_generate(sd, cfg, x, 3)
    rows = TP.run_local_tp(cfg, sd, x, toks, lg, 2, 64, "cpu")
    assert len(rows) == 3


def test_emu_attn_decode_fused_equals_two_kernels(emu):
    """CPU dry run of tests/test_gpu_ops.py::test_attn_decode_fused_combine_equals_two_kernels on the emulator (group 4 and group 7)."""
    from videollama2_amd import ops
    HD = 128
    for nh, nkv, smax, pos in ((8, 2, 256, 130), (7, 1, 128, 70)):
        qkv, kc, vc = bf((nh + 2 * nkv) * HD, seed=pos), bf(nkv, smax, HD, seed=2), bf(nkv, smax, HD, seed=3)
        inv = 1.0 / (1e6 ** (torch.arange(0, HD, 2).float() / HD))
        fr = torch.arange(smax).float()[:, None] * inv[None]
        cos_t, sin_t = fr.cos().contiguous(), fr.sin().contiguous()
        nsp, group = (smax + 63) // 64, nh // nkv
        pos_dev = torch.tensor([pos], dtype=torch.int32)
        k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
        p1, p2 = torch.full((nh * nsp * 130,), 7.0), torch.full((nh * nsp * 130,), -3.0)
        o1, o2 = torch.zeros(nh * HD, dtype=torch.bfloat16), torch.ones(nh * HD, dtype=torch.bfloat16)
        ops.attn_decode(qkv, k1, v1, cos_t, sin_t, p1, o1, nh, nkv, pos, HD ** -0.5, pos_dev=pos_dev, ctx_cap=smax)
        cnt = torch.zeros(nkv, dtype=torch.int32)
        ops.attn_decode_fused(qkv, k2, v2, cos_t, sin_t, p2, o2, nh, nkv, pos_dev, HD ** -0.5, cnt)
        assert torch.equal(o1, o2) and torch.equal(k1, k2) and torch.equal(v1, v2)
        assert cnt.tolist() == [((pos + 64) // 64) * ((group + 3) // 4)] * nkv
