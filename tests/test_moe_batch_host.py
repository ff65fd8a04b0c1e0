"""Batched decoding on the Mixtral decoder, host side: the switch and what stays refused, the argument checks of the
new entry points (before any launch) and the sizing of the step's partial-sum buffer.  No GPU needed."""
import ctypes

import pytest
import torch

from tests import moe_oracle as MO


def _bare():
    """A HipMixtralDecoder with no attribute set: what the pinned refusals of the other host tests are called on."""
    from videollama2_amd.decoder import HipMixtralDecoder
    return object.__new__(HipMixtralDecoder)


def _refusals_off(mix):
    x = torch.zeros(4, 256)
    return [(lambda: mix.prefill_batch([], [], None), "MoE \\(mixtral\\) decoder: batched prefill not built"),
            (lambda: mix.generate_batch([x]), "MoE \\(mixtral\\) decoder: batched decoding not built"),
            (lambda: mix._ensure_batch(2), "MoE \\(mixtral\\) decoder: batched / continuous decoding not built"),
            (lambda: mix.prefill(x, cache=([], [])), "MoE \\(mixtral\\) decoder: external caches \\(batched decoding\\) not built"),
            (lambda: mix.generate_batch([x], shared_prefix=x), "MoE \\(mixtral\\) decoder: shared-prefix decode is not built \\(its batched decoding is not\\)")]


def test_switch_is_off_by_default_and_every_refusal_keeps_its_text():
    from videollama2_amd.serving import ContinuousBatcher
    mix = _bare()
    assert mix.moe_batch is False
    for fn, text in _refusals_off(mix):
        with pytest.raises(NotImplementedError, match=text):
            fn()
    mix.tp, mix._dev = 1, torch.device("cpu")
    with pytest.raises(NotImplementedError, match="MoE \\(mixtral\\) decoder: batched / continuous decoding not built"):
        ContinuousBatcher(mix)
    # on and off again: the same refusals
    mix.enable_moe_batch()
    assert mix.moe_batch is True
    mix.enable_moe_batch(False)
    assert mix.moe_batch is False
    for fn, text in _refusals_off(mix):
        with pytest.raises(NotImplementedError, match=text):
            fn()


def test_what_stays_refused_with_the_switch_on():
    from videollama2_amd.decoder import HipMixtralDecoder
    mix = _bare().enable_moe_batch()
    x = torch.zeros(4, 256)
    for fn, text in [(lambda: mix.generate_batch([x], shared_prefix=x), "MoE \\(mixtral\\) decoder: shared-prefix decode is not built"),
                     (lambda: mix._shared_prefix_refusals(paged_ok=True), "MoE \\(mixtral\\) decoder: shared-prefix decode is not built"),
                     (lambda: mix.enable_paged_kv(8), "MoE \\(mixtral\\) decoder: the paged KV cache is not built for it"),
                     (lambda: mix.enable_paged_kv(8, fp8=True), "MoE \\(mixtral\\) decoder: the paged KV cache is not built for it"),
                     (lambda: mix.enable_fp8_kv(), "MoE \\(mixtral\\) decoder: the fp8 KV cache is not built for it"),
                     (lambda: mix.enable_fp8_decode(), "MoE \\(mixtral\\) decoder: fp8 weights not built"),
                     (lambda: mix.enable_fp8_prefill(), "MoE \\(mixtral\\) decoder: fp8 weights not built"),
                     (lambda: mix.enable_mxfp4_decode(), "MoE \\(mixtral\\) decoder: MXFP4 weights not built")]:
        with pytest.raises(NotImplementedError, match=text):
            fn()
    cfg = MO.small_mixtral_cfg(n_layers=1)
    for kw in (dict(tp_shard=(0, 2)), dict(tp_group=object()), dict(tp_local=object())):
        with pytest.raises(NotImplementedError, match="MoE \\(mixtral\\) decoder: tensor / expert parallelism not built"):
            HipMixtralDecoder(cfg, {}, "cpu", **kw)


def test_toggling_drops_the_graphs_and_is_refused_with_requests_in_flight():
    mix = _bare()
    mix._batch_graphs, mix._bb, mix.graph = {(4, False): object()}, dict(B=4), object()
    mix.enable_moe_batch()
    assert mix._batch_graphs == {} and mix._bb is None and mix.graph is None

    class Busy:
        n = 2

        def in_flight(self):
            return self.n
    mix._bb_busy = Busy()
    for on in (False, True):
        with pytest.raises(RuntimeError, match="enable_moe_batch: a ContinuousBatcher holds requests in flight"):
            mix.enable_moe_batch(on)
    assert mix.moe_batch is True
    mix._bb_busy.n = 0
    assert mix.enable_moe_batch(False).moe_batch is False


def test_model_switch_passes_through_and_a_dense_decoder_refuses():
    from videollama2_amd.model import VideoLLaMA2Hip
    from videollama2_amd.decoder import HipMistralDecoder
    model = object.__new__(VideoLLaMA2Hip)
    model.__dict__["decoder"] = _bare()
    assert model.enable_moe_batch() is model and model.decoder.moe_batch is True
    model.enable_moe_batch(False)
    assert model.decoder.moe_batch is False
    model.__dict__["decoder"] = object.__new__(HipMistralDecoder)
    with pytest.raises(NotImplementedError, match="enable_moe_batch: the decoder is dense"):
        model.enable_moe_batch()


def test_prefill_batch_splits_groups_at_the_scan_kernels_capacity(monkeypatch):
    """k = 4: MOE_SCAN_MAX / k = 4096 rows per group, below generate_batch's PREFILL_GROUP_TOKENS; the groups go to the dense prefill_batch
    in order, each with its own caches and logits rows."""
    from videollama2_amd.decoder import HipMistralDecoder
    mix = _bare().enable_moe_batch()
    mix.k = 4
    seen = []

    def fake(self, xs, caches, logits_out):
        seen.append(([x.shape[0] for x in xs], list(caches), logits_out.shape[0]))
        return [x.shape[0] for x in xs]
    monkeypatch.setattr(HipMistralDecoder, "prefill_batch", fake)
    lens = [3000, 1000, 97, 4096, 1, 5000, 2]
    out = mix.prefill_batch([torch.zeros(n, 8) for n in lens], list(range(len(lens))), torch.zeros(len(lens), 16))
    assert out == lens
    assert seen == [([3000, 1000], [0, 1], 2), ([97], [2], 1), ([4096], [3], 1), ([1], [4], 1), ([5000], [5], 1), ([2], [6], 1)]
    assert all(sum(g[0]) * mix.k <= 16384 or len(g[0]) == 1 for g in seen)
    seen.clear()
    mix.k = 2
    mix.prefill_batch([torch.zeros(n, 8) for n in (4096, 4096, 1)], [0, 1, 2], torch.zeros(3, 16))
    assert [g[0] for g in seen] == [[4096, 4096], [1]]


def _lib_built():
    import __graft_entry__ as ge
    ge.build()
    from videollama2_amd import _lib
    return _lib, _lib.load()


def _skinny_ks(N, K):
    """csrc/skinny_plan.h restated: the K split of the skinny-M GEMMs, a function of N and K only."""
    steps = K // 32
    ks = min(max((4096 + N // 16 - 1) // (N // 16), 1), 32)
    while ks > 1 and steps % ks:
        ks -= 1
    return ks


def test_partial_buffer_is_the_skinny_plans_split_times_the_permuted_rows():
    _lib, lib = _lib_built()
    assert "vl2_moe_gemm_skinny_part_bytes" in _lib.EXPORTS
    for name in ("vl2_moe_route_rows", "vl2_moe_gemm_skinny", "vl2_moe_gemv_batched"):
        assert name in _lib.EXPORTS and name in _lib.MOE_BATCH_SIGNATURES and name not in _lib.SIGNATURES    # the emulator's symbol set is unchanged
    assert lib.vl2_version() == 7
    for nb in (1, 5, 16, 17, 33, 64):
        for k in (1, 2, 4):
            for N, K in ((1024, 256), (256, 512), (28672, 4096), (4096, 14336), (128, 1184), (64, 32)):
                assert lib.vl2_moe_gemm_skinny_part_bytes(nb, k, N, K) == _skinny_ks(N, K) * nb * k * N * 4, (nb, k, N, K)
    assert _skinny_ks(1024, 256) > 1 and _skinny_ks(256, 512) > 1 and _skinny_ks(128, 1184) == 1
    for bad in ((65, 2, 1024, 256), (0, 2, 1024, 256), (8, 5, 1024, 256), (8, 2, 1000, 256), (8, 2, 1024, 250)):
        assert lib.vl2_moe_gemm_skinny_part_bytes(*bad) == -1, bad
    # the decoder's step buffer: the larger of gate/up (N = 2I, K = D) and down (N = D, K = I)
    mix = _bare()
    mix.k, mix.I, mix.D = 2, 14336, 4096
    for nb in (5, 64):
        assert mix.moe_part_bytes(nb) == max(_skinny_ks(28672, 4096) * nb * 2 * 28672 * 4, _skinny_ks(4096, 14336) * nb * 2 * 4096 * 4)
    assert mix.moe_part_bytes(64) == 16 * 128 * 4096 * 4                         # down (ks 16) at full width and 64 requests: 33.6 MB
    mix.k, mix.I, mix.D = 2, 512, 256
    assert mix.moe_part_bytes(8) == max(_skinny_ks(1024, 256) * 16 * 1024 * 4, _skinny_ks(256, 512) * 16 * 256 * 4)


def test_entry_points_reject_bad_shapes_and_short_buffers_before_launching():
    """In the style of test_moe_abi_rejects_short_row_strides: every check runs before every launch, so no GPU is needed."""
    _lib, lib = _lib_built()
    p = ctypes.c_void_p(4096)
    err = lambda: lib.vl2_last_error_string()
    # ---- vl2_moe_route_rows(x, ldx, wr, S, D, E, k, eps, ids, wts, logits, counts, offs, gather, inv, stream)
    assert lib.vl2_moe_route_rows(p, 64, p, 4, 128, 8, 2, 1e-5, p, p, None, p, p, p, p, None) == -2 and b"ldx>=D" in err()
    assert lib.vl2_moe_route_rows(p, 128, p, 4, 128, 65, 2, 1e-5, p, p, None, p, p, p, p, None) == -3
    assert lib.vl2_moe_route_rows(p, 128, p, 4, 128, 8, 5, 1e-5, p, p, None, p, p, p, p, None) == -3
    assert lib.vl2_moe_route_rows(p, 128, p, 8193, 128, 8, 2, 1e-5, p, p, None, p, p, p, p, None) == -3 and b"S * k <= 16384" in err()
    assert lib.vl2_moe_route_rows(p, 128, p, 4, 128, 8, 2, 1e-5, p, p, None, p, None, p, p, None) == -1 and b"come together" in err()
    assert lib.vl2_moe_route_rows(p, 128, p, 4, 128, 8, 2, 1e-5, None, p, None, p, p, p, p, None) == -1
    # ---- vl2_moe_gemm_skinny(A, lda, a_rows, rowmap, W, w_stride, ldw, C, ldc, counts, offs, S, k, E, N, K, flags, part, part_bytes, stream)
    N, K, S, k, E = 1024, 256, 8, 2, 8
    need = lib.vl2_moe_gemm_skinny_part_bytes(S, k, N, K)
    good = [p, K, S, p, p, N * K, K, p, N // 2, p, p, S, k, E, N, K, 1, p, need, None]

    def skinny(**over):
        names = ["A", "lda", "a_rows", "rowmap", "W", "w_stride", "ldw", "C", "ldc", "counts", "offs", "S", "k", "E", "N", "K", "flags", "part",
                 "part_bytes", "stream"]
        a = list(good)
        for key, v in over.items():
            a[names.index(key)] = v
        return lib.vl2_moe_gemm_skinny(*a)
    assert skinny(S=65, a_rows=65) == -2 and b"S<=64" in err()
    assert skinny(N=1000) == -2 and b"N%64==0" in err()
    assert skinny(N=960, w_stride=960 * K) == -2 and b"N%128==0 with SWIGLU" in err()
    assert skinny(K=250) == -2 and b"K%32==0" in err()
    assert skinny(part_bytes=need - 4) == -1 and b"partial buffer too small" in err() and str(need).encode() in err()
    assert skinny(part=None) == -1 and b"partial sums" in err()
    assert skinny(E=65) == -3 and skinny(k=5) == -3
    assert skinny(lda=K - 8) == -2 and skinny(ldw=K - 8) == -2 and skinny(w_stride=N * K - 8) == -2 and skinny(ldc=N // 2 - 4) == -2
    assert skinny(a_rows=S - 1) == -2 and b"A has 7 rows, need 8" in err()
    assert skinny(rowmap=None, a_rows=S * k - 1) == -2 and b"A has 15 rows, need 16" in err()
    assert skinny(flags=2) == -3
    assert skinny(counts=None) == -1 and skinny(offs=None) == -1
    # ---- vl2_moe_gemv_batched(W, w_stride, ldw, x, ldx, ids, wts, res, ldres, y, ldy, S, E, k, N, K, eps, flags, stream)
    gu = [p, N * K, K, p, K, p, None, None, 0, p, N // 2, 4, E, k, N, K, 1e-5, 1, None]
    dn = [p, K * 512, 512, p, 512, p, p, p, K, p, K, 4, E, k, K, 512, 1e-5, 0, None]

    def gemv(base, **over):
        names = ["W", "w_stride", "ldw", "x", "ldx", "ids", "wts", "res", "ldres", "y", "ldy", "S", "E", "k", "N", "K", "eps", "flags", "stream"]
        a = list(base)
        for key, v in over.items():
            a[names.index(key)] = v
        return lib.vl2_moe_gemv_batched(*a)
    assert gemv(gu, ldx=K - 8) == -2 and gemv(gu, ldw=K - 8) == -2 and gemv(gu, w_stride=N * K - 8) == -2
    assert gemv(gu, ldy=N // 2 - 8) == -2 and gemv(gu, wts=p) == -2 and gemv(gu, res=p) == -2
    assert gemv(gu, E=65) == -3 and gemv(gu, k=5) == -3 and gemv(gu, flags=3) == -3 and gemv(gu, S=0) == -1
    assert gemv(dn, wts=None) == -1 and b"routing weights" in err()
    assert gemv(dn, ldx=520) == -2 and b"without a gap" in err()
    assert gemv(dn, ldy=K - 8) == -2 and gemv(dn, ldres=K - 8) == -2
    assert gemv(dn, K=65536, ldw=65536, ldx=65536, w_stride=K * 65536) == -2 and b"fit the LDS" in err()
