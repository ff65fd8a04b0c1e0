"""Operator-level Python wrappers over the C ABI (include/vl2hip.h).  PyTorch-ROCm tensors are used ONLY as device
storage: every wrapper passes raw `data_ptr()`s plus the current HIP stream to libvl2hip.so and returns torch tensors
it allocated.  No torch math happens here and there is no fallback path."""
import ctypes

import torch

from . import _lib

ACT_NONE, ACT_QGELU, ACT_GELU, ACT_SILU, ACT_SIGMOID, ACT_GELU_TANH = 0, 1, 2, 3, 4, 5
GEMM_SWIGLU, GEMM_OUT_F32 = 1, 2
PROFILE = None      # bench.py sets this to a list: every gemm launch is then bracketed by HIP events on the launch stream


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.dim() >= 2 and t.stride(-1) != 1:
        raise ValueError(f"{name} must be contiguous in its last dim")


GEMM_SPLITK = 4
NORM_NONE, NORM_RMS, NORM_LN = 0, 1, 2

# Launch controls of the GEMM family.  They are HOST-side settings of this binding layer, handed to libvl2hip.so with every
# call (vl2_gemm_desc.variant / flags / ws): the library itself holds no mutable state.
_WORKSPACE = {}
_CTL = dict(variant=0, splitk=False, attn_variant=0, stage_flags=0, gemm_flags=0)
GEMM_PERSISTENT, GEMM_NO_MIX, GEMM_NO_FILL, GEMM_WEAVE, GEMM_FP8 = 8, 16, 32, 64, 128                                    # vl2_gemm_desc.flags (include/vl2hip.h)
STAGE_PERSISTENT_GEMM, STAGE_NO_MIX, STAGE_SELF_REDUCE, STAGE_FUSED_DECODE_ATTN, STAGE_DECODE_TAIL, STAGE_STC_UNFUSED = 1, 2, 4, 8, 16, 32
STAGE_WEAVE = 256                     # lab: LDS-DMA issue woven into the MFMA phases of the 128x256 / 224x128 / 192x128 ping-pong GEMMs
STAGE_NO_FILL_TILES = 128             # A/B of the fill-the-round GEMM tiles (csrc/k_gemm7.h)
STAGE_NO_WEAVE4, GEMM_NO_WEAVE4 = 16384, 1024   # A/B: the 192-row tiles without the woven issue (their default since round 5)
STAGE_WEAVE4, GEMM_WEAVE4 = 8192, 512 # the 256x256 / 192x256 ping-pong GEMMs issue their LDS-DMA from the matrix phases (k_gemm.h gemm4_body WEAVE4)
STAGE_NO_MFMA16 = 65536               # the decoder prefill's gate/up WITHOUT the 16x16x32-MFMA kernels (its default since round 6: decoder.prefill passes mfma16=True)
STAGE_MFMA16, GEMM_MFMA16 = 32768, 2048  # opt-in: every SwiGLU (gate/up) GEMM of the session on the 16x16x32-MFMA kernel (csrc/k_gemm9.h): as accurate, OTHER last bits
STAGE_VIT_NO_PERSISTENT = 4096        # vl2_vit_forward without the persistent GEMM form (its default since round 5): A/B
STAGE_NO_TICKET_OPS = 2048            # ops.gemm(norm_out=...) only: the appended launch instead of the in-kernel ticket (test / A/B control of the operator path)
STAGE_ROW_TICKET, GEMM_NO_TICKET = 1024, 256  # stage calls: producer-side finalize (k_gemm.h gemm_rows_ticket) instead of the row_norm_finalize launches (lab: not faster)
STAGE_PREFILL_FP8 = 512               # prefill projections on the fp8 matrix pipe (W8A8, vl2_llm_desc.layers_w8); set by the decoder, not a lab switch
STAGE_DECODE_FP8 = 64                 # decode step on the fp8 copies of the weights (vl2_llm_desc.layers_w8); set by the decoder, not a lab switch
GEMV_RMS_PLAIN = 32   # vl2_*_desc.flags of the stage calls


def attach_workspace(device):
    """Allocate (once per device, zero-filled) the GEMM workspace (split-K partial tiles + tile counters, stream-K, the skinny-M
    GEMM's fp32 partial sums); the library itself never allocates.  Calls on one device share it, so they must be ordered on
    one stream (every path in this package runs its GEMMs on the current stream)."""
    key = str(torch.device(device))
    if key not in _WORKSPACE:
        n = int(_lib.load().vl2_workspace_bytes())
        _WORKSPACE[key] = torch.zeros((n + 15) // 16 * 16, dtype=torch.uint8, device=device)
    return _WORKSPACE[key]


def _ws(device):
    return _WORKSPACE.get(str(torch.device(device)))


def set_splitk(on):
    """Split-K for small-grid GEMMs (VL2_GEMM_SPLITK; needs `attach_workspace`).  Off by default: it trades the "same rows ->
    same bits whatever M" property for latency on small-M shapes (measured on MI355X: 1154x1024x4096 45.9 -> 39.7 us,
    169x4096x4096 40.8 -> 27.9 us, 338x4096x32768 436 -> 160 us).  Never enable it while GEMMs run concurrently on several
    streams (they would share the one workspace)."""
    _CTL["splitk"] = bool(on)


def set_attn_kv_groups(n):
    """Attention structure (vl2_attn_fwd `variant`, include/vl2hip.h): 0 = auto, 1 = register-staged with one group of 4 waves per workgroup,
    2 = two groups that split the KV tiles and merge through LDS, 3 = LDS-DMA ring + transpose reads, 4 = 3 with two key streams."""
    _CTL["attn_variant"] = int(n)


def set_stage_flags(flags):
    """Experiment controls of the stage-level entry points and of `gemm` (VL2_STAGE_* in include/vl2hip.h; all off by default):
    STAGE_PERSISTENT_GEMM, STAGE_NO_MIX, STAGE_SELF_REDUCE, STAGE_FUSED_DECODE_ATTN.  They travel in the descriptors of the calls
    (the library reads no environment variables and keeps no state)."""
    _CTL["stage_flags"] = int(flags)
    _CTL["gemm_flags"] = (GEMM_PERSISTENT if flags & STAGE_PERSISTENT_GEMM else 0) | (GEMM_NO_MIX if flags & STAGE_NO_MIX else 0) | \
                         (GEMM_NO_FILL if flags & STAGE_NO_FILL_TILES else 0) | (GEMM_WEAVE if flags & STAGE_WEAVE else 0) | \
                         (GEMM_NO_TICKET if flags & STAGE_NO_TICKET_OPS else 0) | (GEMM_WEAVE4 if flags & STAGE_WEAVE4 else 0) | \
                         (GEMM_NO_WEAVE4 if flags & STAGE_NO_WEAVE4 else 0)


def stage_flags():
    return _CTL["stage_flags"]


class tower_gemm_flags:
    """The per-operator tower loops (tower.py `_hidden`) mirror what vl2_vit_forward does with its GEMMs: the persistent form (VL2_GEMM_PERSISTENT) is
    the tower's default since round 5, unless STAGE_VIT_NO_PERSISTENT is set.  A context manager around those loops; restores the session's flags."""
    def __enter__(self):
        self._saved = _CTL["gemm_flags"]
        if not (_CTL["stage_flags"] & STAGE_VIT_NO_PERSISTENT):
            _CTL["gemm_flags"] |= GEMM_PERSISTENT
        return self

    def __exit__(self, *exc):
        _CTL["gemm_flags"] = self._saved
        return False


def set_gemm_variant(v):
    """0 auto (per-shape choice), 1 128x128x64, 2 stream-K, 4 128x256x64 ping-pong, 8 256x256x32 ping-pong, 12 192x256, 32 64x64 small-M,
    256 128x128 8-wave deep-ring one-round kernel, 224 / 192 the fill-the-round 224x128 / 192x128 ping-pong kernel, 16 the 256x256 ping-pong
    kernel on v_mfma_f32_16x16x32_bf16 (the one variant with other last bits) (include/vl2hip.h)."""
    _CTL["variant"] = int(v)


def gemm(a, w, bias=None, res=None, act=ACT_NONE, swiglu=False, out_f32=False, out=None, M=None,
         gather=None, out_map=None, res_map=None, flop_k=None, stats_out=None, norm=None, norm_out=None, mfma16=False, tile_ctr=None):
    """C = epilogue(a @ w.T).  a [M,K] bf16 (or row pool when `gather`), w [N,K] bf16, bias fp32 [N], res bf16 rows.
    gather = (a_idx int32 [nseg, M], zero_row (unused), seg_k).  out_map = (grp, grp_pad, row_off),
    res_map = (row_mod, row_off) -- see include/vl2hip.h.
    stats_out: fp32 [M, N/64, 2] buffer the epilogue fills with (sum, sum of squares) per row and 64-column block of the
    stored output.  norm = (kind, stats_in, eps, w_colsum): Norm(a) @ w.T computed on the raw rows of `a` from the statistics
    the GEMM that wrote `a` emitted (NORM_RMS / NORM_LN; w must carry the norm weight folded in, bias the folded shift).
    norm_out = (kind, eps, row_norm_out fp32 [M, 2], tickets uint32 [>= M/64 + 2], zeroed once): with stats_out, the call also leaves
    (mean, rstd) of its OUTPUT rows in row_norm_out -- what row_norm_finalize(stats_out) would compute, without the launch."""
    _chk(a, _lib.elem_dtype(), "a"); _chk(w, _lib.elem_dtype(), "w"); _chk(bias, torch.float32, "bias"); _chk(res, _lib.elem_dtype(), "res")
    N = w.shape[0]
    if gather is not None:
        a_idx, _zero_row, seg_k = gather
        K = seg_k * a_idx.shape[0]
        M = a_idx.shape[1] if M is None else M
    else:
        a_idx = None
        seg_k = 0
        K = w.shape[1]
        M = a.shape[0] if M is None else M
        if a.shape[1] != K:
            raise ValueError(f"gemm: a is [{a.shape[0]},{a.shape[1]}] but w is [{N},{K}]")
    ncol = N // 2 if swiglu else N
    if out is None:
        out = torch.empty((M, ncol), dtype=torch.float32 if out_f32 else _lib.elem_dtype(), device=a.device)
    grp, grp_pad, row_off = out_map or (0, 0, 0)
    rmod, roff = res_map or (0, 0)
    ws = _ws(a.device)
    flags = (GEMM_SWIGLU if swiglu else 0) | (GEMM_OUT_F32 if out_f32 else 0) | (GEMM_SPLITK if (_CTL["splitk"] and ws is not None) else 0) | _CTL["gemm_flags"] | \
            (GEMM_MFMA16 if ((mfma16 and not _CTL["stage_flags"] & STAGE_NO_MFMA16) or (swiglu and _CTL["stage_flags"] & STAGE_MFMA16)) else 0)
    kind, stats_in, eps, colsum = norm if norm is not None else (NORM_NONE, None, 0.0, None)
    row_norm = None
    if stats_in is not None and stats_in.dim() == 2:      # [rows, 2] = already reduced (row_norm_finalize)
        row_norm, stats_in = stats_in, None
        if row_norm.shape[0] < M or row_norm.shape[1] != 2:
            raise ValueError(f"gemm: row_norm must be [>={M}, 2], got {tuple(row_norm.shape)}")
        _chk(row_norm, torch.float32, "row_norm")
    if stats_out is not None and tuple(stats_out.shape) != (M, N // 64, 2):
        raise ValueError(f"gemm: stats_out must be [{M}, {N // 64}, 2], got {tuple(stats_out.shape)}")
    if stats_in is not None and (stats_in.shape[0] < M or tuple(stats_in.shape[1:]) != (K // 64, 2)):
        raise ValueError(f"gemm: stats_in must be [>={M}, {K // 64}, 2], got {tuple(stats_in.shape)}")
    _chk(stats_out, torch.float32, "stats_out"); _chk(stats_in, torch.float32, "stats_in"); _chk(colsum, torch.float32, "w_colsum")
    d = _lib.GemmDesc(ctypes.sizeof(_lib.GemmDesc), M, N, K, _p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0),
                      _p(bias), _p(res), res.stride(0) if res is not None else 0, act, flags, _p(a_idx), seg_k,
                      grp, grp_pad, row_off, rmod, roff, _p(stats_out), _p(stats_in), kind, float(eps), _p(colsum), _p(row_norm),
                      _p(ws), ws.numel() if ws is not None else 0, _CTL["variant"])
    if norm_out is not None:
        ko, eo, rn_out, tick = norm_out
        _chk(rn_out, torch.float32, "row_norm_out")
        if stats_out is None or rn_out.shape[0] < M or tick.numel() < M // 64 + 2 or tick.dtype not in (torch.int32, torch.uint32):
            raise ValueError("gemm: norm_out needs stats_out, row_norm_out [>= M, 2] and >= M/64 + 2 zeroed 32-bit tickets")
        d.row_norm_out, d.row_ticket, d.norm_out, d.norm_out_eps = _p(rn_out), _p(tick), ko, float(eo)
    if tile_ctr is not None:        # >= 16 bytes, zeroed once: the tile queue of the persistent form (GEMM_PERSISTENT; the kernels re-arm it) -- what the stage calls pass
        d.tile_ctr = _p(tile_ctr)
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _lib.call("vl2_gemm", ctypes.byref(d), _stream())
    if PROFILE is not None:
        e1.record()
        PROFILE.append(("gemm", 2.0 * M * N * (flop_k or K), e0, e1, (M, N, K)))
    return out


def row_norm_finalize(stats, K, kind, eps, out=None):
    """stats [rows, K/64, 2] -> [rows, 2] = (mean, rstd) for NORM_RMS / NORM_LN: hand the result to gemm(norm=(kind, <it>, eps,
    colsum)) so the consuming GEMM does not reduce the partials again in every column tile."""
    _chk(stats, torch.float32, "stats")
    rows, np_ = stats.shape[0], stats.shape[1]
    out = torch.empty((rows, 2), dtype=torch.float32, device=stats.device) if out is None else out
    _lib.call("vl2_row_norm_finalize", _p(stats), _p(out), rows, np_, K, kind, float(eps), _stream())
    return out


def row_stats(x, out=None):
    """(sum, sum of squares) per row and 64-column block of x [rows, C] bf16 -> fp32 [rows, C/64, 2]: seeds a norm-carrying
    GEMM chain for a tensor no GEMM wrote (same layout and summation order as `gemm(..., stats_out=)`)."""
    _chk(x, _lib.elem_dtype(), "x")
    rows, C = x.shape
    out = torch.empty((rows, C // 64, 2), dtype=torch.float32, device=x.device) if out is None else out
    _lib.call("vl2_row_stats", _p(x), _p(out), rows, C, x.stride(0), _stream())
    return out


def layernorm(x, w, b, eps, res=None, silu=False, out=None):
    _chk(x, _lib.elem_dtype(), "x"); _chk(w, torch.float32, "w"); _chk(b, torch.float32, "b"); _chk(res, _lib.elem_dtype(), "res")
    rows, C = x.shape
    out = torch.empty((rows, C), dtype=_lib.elem_dtype(), device=x.device) if out is None else out
    _lib.call("vl2_layernorm", _p(x), _p(out), _p(w), _p(b), _p(res), rows, C, x.stride(0), out.stride(0),
              res.stride(0) if res is not None else 0, float(eps), int(silu), _stream())
    return out


def rmsnorm(x, w, eps, out=None):
    _chk(x, _lib.elem_dtype(), "x"); _chk(w, torch.float32, "w")
    rows, C = x.shape
    out = torch.empty((rows, C), dtype=_lib.elem_dtype(), device=x.device) if out is None else out
    _lib.call("vl2_rmsnorm", _p(x), _p(out), _p(w), rows, C, x.stride(0), out.stride(0), float(eps), _stream())
    return out


_DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}       # frame types of the patch-row kernels (any build reads all three)


def patchify(frames, patch, kp):
    """frames [T,3,H,W] fp32/fp16/bf16 -> [T*G*G, kp] bf16 im2col rows."""
    if frames.dtype not in _DTYPE_CODE:
        raise TypeError(f"frames dtype {frames.dtype} not supported")
    frames = frames.contiguous()
    T, C, H, W = frames.shape
    G = H // patch
    out = torch.empty((T * G * G, kp), dtype=_lib.elem_dtype(), device=frames.device)
    _lib.call("vl2_patchify", _p(frames), _DTYPE_CODE[frames.dtype], _p(out), T, H, W, patch, G, kp, _stream())
    return out


def patchify_u8(frames_thwc, patch, kp, rescale, mean, std):
    """frames [T,H,W,3] uint8 (device) -> [T*G*G, kp] bf16 im2col rows of (x*rescale - mean) / std."""
    _chk(frames_thwc, torch.uint8, "frames")
    frames_thwc = frames_thwc.contiguous()
    T, H, W, C = frames_thwc.shape
    if C != 3:
        raise ValueError(f"expected uint8 frames [T,H,W,3], got {tuple(frames_thwc.shape)}")
    G = H // patch
    out = torch.empty((T * G * G, kp), dtype=_lib.elem_dtype(), device=frames_thwc.device)
    m, sd = [float(v) for v in mean], [float(v) for v in std]
    _lib.call("vl2_patchify_u8", _p(frames_thwc), _p(out), T, H, W, patch, G, kp, float(rescale), m[0], m[1], m[2], sd[0], sd[1], sd[2],
              _stream())
    return out


def fill_cls(x, cls_pos, T, rows_per_frame):
    _lib.call("vl2_fill_cls", _p(x), _p(cls_pos), T, x.shape[1], rows_per_frame, _stream())


def attn_fwd(q, k, v, o, q_str, k_str, v_str, o_str, B, H, nq, nk, group, scale, causal, causal_off, D):
    """Strided fused attention; *_str = (batch_stride, head_stride, row_stride) in elements; q/k/v/o may be views
    into one fused buffer (pass tensors whose data_ptr is the first element of head 0, batch 0)."""
    _lib.call("vl2_attn_fwd", _p(q), _p(k), _p(v), _p(o), *q_str, *k_str, *v_str, *o_str, B, H, nq, nk, group, float(scale),
              int(causal), causal_off, D, _CTL["attn_variant"], _stream())
    return o


def dwconv3x3_ln_silu(x, w9c, lnw, lnb, F, H, W, eps=1e-5):
    _chk(x, _lib.elem_dtype(), "x")
    C = x.shape[-1]
    y = torch.empty_like(x)
    _lib.call("vl2_dwconv3x3_ln_silu", _p(x), _p(y), _p(w9c), _p(lnw), _p(lnb), F, H, W, C, float(eps), _stream())
    return y


def dwconv3x3_ln_silu_mean(x, w9c, lnw, lnb, F, H, W, eps=1e-5):
    """Depthwise 3x3 + LayerNorm2d + SiLU AND the SE squeeze of the result: returns (y [F*H*W, C], mean fp32 [F, C])."""
    _chk(x, _lib.elem_dtype(), "x")
    C = x.shape[-1]
    y = torch.empty_like(x)
    mean = torch.empty((F, C), dtype=torch.float32, device=x.device)
    nb = _lib.load().vl2_dwconv_mean_workspace_bytes(F, C)
    ws = torch.empty((nb,), dtype=torch.uint8, device=x.device)
    _lib.call("vl2_dwconv3x3_ln_silu_mean", _p(x), _p(y), _p(w9c), _p(lnw), _p(lnb), F, H, W, C, float(eps), _p(mean), _p(ws), nb, _stream())
    return y, mean


def se_excite_scale_(x, g1, w2, b2, F, HW):
    """x[f, :, c] *= sigmoid(w2[c] . g1[f] + b2[c]) in place (SE excite + scale, one launch)."""
    _chk(x, _lib.elem_dtype(), "x"); _chk(g1, torch.float32, "g1"); _chk(w2, _lib.elem_dtype(), "w2"); _chk(b2, torch.float32, "b2")
    _lib.call("vl2_se_excite_scale", _p(x), _p(g1), _p(w2), _p(b2), F, HW, x.shape[-1], w2.shape[1], _stream())
    return x


def chan_mean(x, F, HW):
    C = x.shape[-1]
    m = torch.empty((F, C), dtype=torch.float32, device=x.device)
    _lib.call("vl2_chan_mean", _p(x), _p(m), F, HW, C, _stream())
    return m


def small_linear(x, w, b, act):
    _chk(x, torch.float32, "x"); _chk(w, _lib.elem_dtype(), "w")
    F, K = x.shape
    N = w.shape[0]
    out = torch.empty((F, N), dtype=torch.float32, device=x.device)
    _lib.call("vl2_small_linear", _p(x), _p(w), _p(b), _p(out), F, N, K, act, _stream())
    return out


def se_scale_(x, gate, F, HW):
    _lib.call("vl2_se_scale", _p(x), _p(gate), F, HW, x.shape[-1], _stream())
    return x


def rope_kv(qkv, q_out, kcache, vcache, cos_t, sin_t, nh, nkv, pos0):
    S = qkv.shape[0]
    smax = kcache.shape[1]
    _lib.call("vl2_rope_kv", _p(qkv), _p(q_out), _p(kcache), _p(vcache), _p(cos_t), _p(sin_t), S, nh, nkv, smax, pos0, _stream())


def gemv(w, x, norm_w=None, eps=1e-5, res=None, swiglu=False, out_f32=False, out=None, bias=None):
    _chk(w, _lib.elem_dtype(), "w"); _chk(x, _lib.elem_dtype(), "x"); _chk(bias, torch.float32, "bias")
    N, K = w.shape
    n_out = N // 2 if swiglu else N
    if out is None:
        out = torch.empty((n_out,), dtype=torch.float32 if out_f32 else _lib.elem_dtype(), device=w.device)
    flags = (GEMM_SWIGLU if swiglu else 0) | (GEMM_OUT_F32 if out_f32 else 0)
    _lib.call("vl2_gemv_bf16", _p(w), _p(x), _p(norm_w), _p(res), _p(bias), _p(out), N, K, w.stride(0), float(eps), flags, _stream())
    return out


def quant_fp8(w):
    """include/vl2hip.h vl2_pack_quant_fp8: 16-bit weights [N, K] -> (e4m3fn bytes [N, K] as uint8, power-of-two row scales [N] fp32)."""
    _chk(w, _lib.elem_dtype(), "w")
    N, K = w.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    sc = torch.empty((N,), dtype=torch.float32, device=w.device)
    _lib.call("vl2_pack_quant_fp8", _p(w), N, K, w.stride(0), _p(q), _p(sc), _stream())
    return q, sc


def quant_act_fp8(x, rms_eps=None, out=None, row_tab=None):
    """include/vl2hip.h vl2_quant_act_fp8: 16-bit activation rows [M, K] -> (e4m3fn bytes [M, K] as uint8, row table [M, 2] fp32 = (0, row scale
    [x RMS rstd when rms_eps is given])), the A operand and `row_norm` of gemm_fp8."""
    _chk(x, _lib.elem_dtype(), "x")
    M, K = x.shape
    q = torch.empty((M, K), dtype=torch.uint8, device=x.device) if out is None else out
    tab = torch.empty((M, 2), dtype=torch.float32, device=x.device) if row_tab is None else row_tab
    _lib.call("vl2_quant_act_fp8", _p(x), x.stride(0), _p(q), q.stride(0), _p(tab), M, K, NORM_NONE if rms_eps is None else NORM_RMS,
              0.0 if rms_eps is None else float(rms_eps), _stream())
    return q, tab


def gemm_fp8(a8, row_tab, w8, col_scale, bias=None, res=None, act=ACT_NONE, swiglu=False, out_f32=False, out=None):
    """C = epilogue(row_tab[m, 1] * col_scale[n] * (a8 @ w8.T)) on the fp8 matrix pipe (vl2_gemm with VL2_GEMM_FP8; W8A8, an OPTIONAL
    arithmetic): a8 [M, K] / w8 [N, K] e4m3fn bytes (quant_act_fp8 / quant_fp8), K % 128 == 0, N % 256 == 0."""
    _chk(a8, torch.uint8, "a8"); _chk(w8, torch.uint8, "w8"); _chk(row_tab, torch.float32, "row_tab"); _chk(col_scale, torch.float32, "col_scale")
    _chk(bias, torch.float32, "bias"); _chk(res, _lib.elem_dtype(), "res")
    M, K = a8.shape
    N = w8.shape[0]
    if w8.shape[1] != K or row_tab.shape[0] < M or col_scale.shape[0] != N:
        raise ValueError("gemm_fp8: shapes of a8 / w8 / row_tab / col_scale do not agree")
    ncol = N // 2 if swiglu else N
    if out is None:
        out = torch.empty((M, ncol), dtype=torch.float32 if out_f32 else _lib.elem_dtype(), device=a8.device)
    flags = GEMM_FP8 | (GEMM_SWIGLU if swiglu else 0) | (GEMM_OUT_F32 if out_f32 else 0)
    d = _lib.GemmDesc(ctypes.sizeof(_lib.GemmDesc), M, N, K, _p(a8), a8.stride(0), _p(w8), w8.stride(0), _p(out), out.stride(0),
                      _p(bias), _p(res), res.stride(0) if res is not None else 0, act, flags, None, 0, 0, 0, 0, 0, 0, None, None, NORM_NONE, 0.0, None,
                      _p(row_tab), None, 0, _CTL["variant"] if _CTL["variant"] in (4, 8, 12) else 0, _p(col_scale))
    if PROFILE is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _lib.call("vl2_gemm", ctypes.byref(d), _stream())
    if PROFILE is not None:
        e1.record()
        PROFILE.append(("gemm_fp8", 2.0 * M * N * K, e0, e1, (M, N, K)))
    return out


def _out_flags(rows, N, swiglu, out_f32, out, device, rms_plain=False):
    """The output tensor ([rows, n_out]; [n_out] for rows = None) and the flag word of a decode projection on quantised weights."""
    n_out = N // 2 if swiglu else N
    if out is None:
        out = torch.empty((n_out,) if rows is None else (rows, n_out), dtype=torch.float32 if out_f32 else _lib.elem_dtype(), device=device)
    return out, (GEMM_SWIGLU if swiglu else 0) | (GEMM_OUT_F32 if out_f32 else 0) | (GEMV_RMS_PLAIN if rms_plain else 0)


def gemv_fp8(q, scale, x, norm_w=None, eps=1e-5, res=None, swiglu=False, out_f32=False, out=None, bias=None, rms_plain=False):
    """y = scale * (q @ x) (+ bias) (+ res) for one token on fp8 weights (include/vl2hip.h vl2_gemv_fp8; W8A16)."""
    _chk(q, torch.uint8, "q"); _chk(scale, torch.float32, "scale"); _chk(x, _lib.elem_dtype(), "x"); _chk(bias, torch.float32, "bias")
    N, K = q.shape
    out, flags = _out_flags(None, N, swiglu, out_f32, out, q.device, rms_plain)
    _lib.call("vl2_gemv_fp8", _p(q), _p(scale), _p(x), _p(norm_w), _p(res), _p(bias), _p(out), N, K, q.stride(0), float(eps), flags, _stream())
    return out


def gemm_skinny(a, w, bias=None, res=None, swiglu=False, out_f32=False, out=None):
    """C = epilogue(a @ w.T) for M = a.shape[0] <= 64 rows (batched decode): weights streamed once, GEMV-style, into MFMA.
    Needs `attach_workspace` (fp32 partial sums of the K split)."""
    _chk(a, _lib.elem_dtype(), "a"); _chk(w, _lib.elem_dtype(), "w"); _chk(bias, torch.float32, "bias"); _chk(res, _lib.elem_dtype(), "res")
    M, K = a.shape
    N = w.shape[0]
    ncol = N // 2 if swiglu else N
    if out is None:
        out = torch.empty((M, ncol), dtype=torch.float32 if out_f32 else _lib.elem_dtype(), device=a.device)
    flags = (GEMM_SWIGLU if swiglu else 0) | (GEMM_OUT_F32 if out_f32 else 0)
    ws = attach_workspace(a.device)
    _lib.call("vl2_gemm_skinny_bf16", _p(a), _p(w), _p(out), _p(bias), _p(res), M, N, K, a.stride(0), w.stride(0), out.stride(0),
              0 if res is None else res.stride(0), flags, _p(ws), ws.numel(), _stream())
    return out


def gemv_batched(w, x, norm_w=None, eps=1e-5, res=None, swiglu=False, out_f32=False, out=None, bias=None):
    """y[b] = W x[b] for the rows of x [MB, K] in one pass over W (batched decode).  res / out are [MB, n_out]."""
    _chk(w, _lib.elem_dtype(), "w"); _chk(x, _lib.elem_dtype(), "x"); _chk(bias, torch.float32, "bias")
    N, K = w.shape
    MB = x.shape[0]
    n_out = N // 2 if swiglu else N
    if out is None:
        out = torch.empty((MB, n_out), dtype=torch.float32 if out_f32 else _lib.elem_dtype(), device=w.device)
    flags = (GEMM_SWIGLU if swiglu else 0) | (GEMM_OUT_F32 if out_f32 else 0)
    _lib.call("vl2_gemv_batched_bf16", _p(w), _p(x), _p(norm_w), _p(res), _p(bias), _p(out), MB, N, K, w.stride(0), x.stride(0),
              out.stride(0), 0 if res is None else res.stride(0), float(eps), flags, _stream())
    return out


def gemm_skinny_fp8(a, q, scale, bias=None, res=None, swiglu=False, out_f32=False, out=None):
    """C = epilogue(scale * (a @ q.T)) on fp8 weights (include/vl2hip.h vl2_gemm_skinny_fp8; W8A16): q [N, K] e4m3fn bytes and scale [N] from
    `quant_fp8`.  Bit for bit `gemm_skinny(a, dequant(q, scale))`.  More than 64 rows run as calls of at most 64 rows each (the weights stream
    once per call; a row's bits do not depend on the chunk it lands in).  Needs `attach_workspace`."""
    _chk(a, _lib.elem_dtype(), "a"); _chk(q, torch.uint8, "q"); _chk(scale, torch.float32, "scale"); _chk(bias, torch.float32, "bias")
    _chk(res, _lib.elem_dtype(), "res")
    M, K = a.shape
    N = q.shape[0]
    out, flags = _out_flags(M, N, swiglu, out_f32, out, a.device)
    ws = attach_workspace(a.device)
    for m0 in range(0, M, 64):
        m1 = min(M, m0 + 64)
        _lib.call("vl2_gemm_skinny_fp8", _p(a[m0:m1]), _p(q), _p(scale), _p(out[m0:m1]), _p(bias), _p(None if res is None else res[m0:m1]),
                  m1 - m0, N, K, a.stride(0), q.stride(0), out.stride(0), 0 if res is None else res.stride(0), flags, _p(ws), ws.numel(), _stream())
    return out


def gemv_batched_fp8(q, scale, x, norm_w=None, eps=1e-5, res=None, swiglu=False, out_f32=False, out=None, bias=None, rms_plain=False):
    """y[b] = gemv_fp8(q, scale, x[b], ...) for the rows of x [MB, K] in one pass over q per launch of up to 4 rows (include/vl2hip.h
    vl2_gemv_batched_fp8): every row bit for bit the single-row call.  res / out are [MB, n_out]."""
    _chk(q, torch.uint8, "q"); _chk(scale, torch.float32, "scale"); _chk(x, _lib.elem_dtype(), "x"); _chk(bias, torch.float32, "bias")
    _chk(res, _lib.elem_dtype(), "res")
    N, K = q.shape
    MB = x.shape[0]
    out, flags = _out_flags(MB, N, swiglu, out_f32, out, q.device, rms_plain)
    _lib.call("vl2_gemv_batched_fp8", _p(q), _p(scale), _p(x), _p(norm_w), _p(res), _p(bias), _p(out), MB, N, K, q.stride(0), x.stride(0),
              out.stride(0), 0 if res is None else res.stride(0), float(eps), flags, _stream())
    return out


def quant_mxfp4(w):
    """include/vl2hip.h vl2_pack_quant_mxfp4: 16-bit weights [N, K], K % 32 == 0 -> (q uint8 [N, K / 2]: two E2M1 codes per byte, k = 2j in bits
    3:0; s uint8 [N, K / 32]: one E8M0 scale per block of 32)."""
    _chk(w, _lib.elem_dtype(), "w")
    N, K = w.shape
    q = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    s = torch.empty((N, K // 32), dtype=torch.uint8, device=w.device)
    _lib.call("vl2_pack_quant_mxfp4", _p(w), N, K, w.stride(0), _p(q), _p(s), s.stride(0), _stream())
    return q, s


def _mxfp4_args(q, s, x, bias, res):
    _chk(q, torch.uint8, "q"); _chk(s, torch.uint8, "s"); _chk(x, _lib.elem_dtype(), "x"); _chk(bias, torch.float32, "bias")
    _chk(res, _lib.elem_dtype(), "res")
    N, K = q.shape[0], q.shape[1] * 2
    if s.shape[0] != N or s.shape[1] * 32 != K or x.shape[-1] != K:
        raise ValueError(f"mxfp4: q {tuple(q.shape)}, s {tuple(s.shape)} and x {tuple(x.shape)} do not agree")
    return N, K


def gemv_mxfp4(q, s, x, norm_w=None, eps=1e-5, res=None, swiglu=False, out_f32=False, out=None, bias=None, rms_plain=False):
    """y = W~ x (+ bias) (+ res) for one token on MXFP4 weights (include/vl2hip.h vl2_gemv_mxfp4; W4A16): q, s from `quant_mxfp4`."""
    N, K = _mxfp4_args(q, s, x, bias, res)
    out, flags = _out_flags(None, N, swiglu, out_f32, out, q.device, rms_plain)
    _lib.call("vl2_gemv_mxfp4", _p(q), _p(s), s.stride(0), _p(x), _p(norm_w), _p(res), _p(bias), _p(out), N, K, q.stride(0), float(eps), flags,
              _stream())
    return out


def gemv_batched_mxfp4(q, s, x, norm_w=None, eps=1e-5, res=None, swiglu=False, out_f32=False, out=None, bias=None, rms_plain=False):
    """y[b] = gemv_mxfp4(q, s, x[b], ...) for the rows of x [MB, K] in one pass over q per launch of up to 4 rows (include/vl2hip.h
    vl2_gemv_batched_mxfp4): every row bit for bit the single-row call.  res / out are [MB, n_out]."""
    N, K = _mxfp4_args(q, s, x, bias, res)
    MB = x.shape[0]
    out, flags = _out_flags(MB, N, swiglu, out_f32, out, q.device, rms_plain)
    _lib.call("vl2_gemv_batched_mxfp4", _p(q), _p(s), s.stride(0), _p(x), _p(norm_w), _p(res), _p(bias), _p(out), MB, N, K, q.stride(0),
              x.stride(0), out.stride(0), 0 if res is None else res.stride(0), float(eps), flags, _stream())
    return out


def gemm_skinny_mxfp4(a, q, s, bias=None, res=None, swiglu=False, out_f32=False, out=None):
    """C = epilogue(a @ W~.T) on MXFP4 weights (include/vl2hip.h vl2_gemm_skinny_mxfp4; W4A16).  Bit for bit `gemm_skinny(a, dequant(q, s))`.
    More than 64 rows run as calls of at most 64 rows each (the weights stream once per call; a row's bits do not depend on the chunk it
    lands in).  Needs `attach_workspace`."""
    N, K = _mxfp4_args(q, s, a, bias, res)
    M = a.shape[0]
    out, flags = _out_flags(M, N, swiglu, out_f32, out, a.device)
    ws = attach_workspace(a.device)
    for m0 in range(0, M, 64):
        m1 = min(M, m0 + 64)
        _lib.call("vl2_gemm_skinny_mxfp4", _p(a[m0:m1]), _p(q), _p(s), s.stride(0), _p(out[m0:m1]), _p(bias),
                  _p(None if res is None else res[m0:m1]), m1 - m0, N, K, a.stride(0), q.stride(0), out.stride(0),
                  0 if res is None else res.stride(0), flags, _p(ws), ws.numel(), _stream())
    return out


def attn_decode(qkv, kcache, vcache, cos_t, sin_t, partial, out, nh, nkv, pos, scale, pos_dev=None, ctx_cap=0):
    """RoPE + KV append + flash-decoding attention of one new token (un-roped fused qkv row) at position `pos`
    (or *pos_dev, for hipGraph replay; then ctx_cap bounds the positions the launch covers)."""
    _lib.call("vl2_attn_decode", _p(qkv), _p(kcache), _p(vcache), _p(cos_t), _p(sin_t), _p(partial), _p(out), nh, nkv,
              kcache.shape[1], int(pos), _p(pos_dev), int(ctx_cap), float(scale), _stream())
    return out


def attn_decode_fused(qkv, kcache, vcache, cos_t, sin_t, partial, out, nh, nkv, pos_dev, scale, cnt):
    """attention + combine of one decode token in ONE launch (vl2_attn_decode_fused): position from device memory, `partial` sized for
    the whole cache, `cnt` = nkv zeroed int32 ticket counters (re-zero before every call).  Same bits as `attn_decode`."""
    smax = kcache.shape[-2]
    _lib.call("vl2_attn_decode_fused", _p(qkv), _p(kcache), _p(vcache), _p(cos_t), _p(sin_t), _p(partial), _p(out), nh, nkv, smax,
              _p(pos_dev), float(scale), _p(cnt), _stream())
    return out


def attn_decode_batched(qkv, kcache, vcache, cos_t, sin_t, partial, out, nh, nkv, pos_dev, ctx_cap, scale):
    """Batched decode attention: qkv [B, (nh+2nkv)*128], caches [B, nkv, smax, 128], out [B, nh*128], pos_dev int32 [B]."""
    B = qkv.shape[0]
    _lib.call("vl2_attn_decode_batched", _p(qkv), _p(kcache), _p(vcache), _p(cos_t), _p(sin_t), _p(partial), _p(out), B,
              qkv.stride(0), kcache.stride(0), out.stride(0), nh, nkv, kcache.shape[2], _p(pos_dev), int(ctx_cap), float(scale), _stream())
    return out


def kv8_alloc(shape_prefix, nkv, smax, device):
    """One layer's fp8 KV cache (include/vl2hip.h, csrc/k_kv8.h) as (k8, v8, ks, vs): e4m3fn codes uint8 [*shape_prefix, nkv, smax, 128] and
    fp32 row scales [*shape_prefix, nkv, smax] (scale 1 on the empty rows, so that every row always dequantises to finite numbers)."""
    codes = lambda: torch.zeros((*shape_prefix, nkv, smax, 128), dtype=torch.uint8, device=device)
    scales = lambda: torch.ones((*shape_prefix, nkv, smax), dtype=torch.float32, device=device)
    return codes(), codes(), scales(), scales()


def _chk_kv8(kv8):
    k8, v8, ks, vs = kv8
    for t, dt, name in ((k8, torch.uint8, "k8"), (v8, torch.uint8, "v8"), (ks, torch.float32, "ks"), (vs, torch.float32, "vs")):
        _chk(t, dt, name)
    if k8.shape[-1] != 128 or v8.shape != k8.shape or ks.shape != k8.shape[:-1] or vs.shape != ks.shape:
        raise ValueError(f"fp8 KV cache: need codes [.., nkv, smax, 128] and scales [.., nkv, smax], got {tuple(k8.shape)}, {tuple(v8.shape)}, "
                         f"{tuple(ks.shape)}, {tuple(vs.shape)}")
    if not (k8[0:1].is_contiguous() and v8[0:1].is_contiguous() and ks[0:1].is_contiguous() and vs[0:1].is_contiguous()):
        raise ValueError("fp8 KV cache: a sequence's codes and scales must be contiguous")
    return k8, v8, ks, vs


def kv_quant(kcache, vcache, kv8, p0, p1):
    """include/vl2hip.h vl2_kv_quant: rows [p0, p1) of one sequence's 16-bit caches [nkv, smax, 128] -> e4m3fn codes and power-of-two row
    scales at the same rows of kv8 = (k8, v8, ks, vs) (uint8 [nkv, smax, 128] x 2, fp32 [nkv, smax] x 2).  Other rows are not written."""
    _chk(kcache, _lib.elem_dtype(), "kcache"); _chk(vcache, _lib.elem_dtype(), "vcache")
    k8, v8, ks, vs = _chk_kv8(kv8)
    if k8.dim() != 3 or kcache.shape != k8.shape or vcache.shape != k8.shape or not (kcache.is_contiguous() and vcache.is_contiguous()):
        raise ValueError(f"kv_quant: need contiguous 16-bit caches of the codes' shape {tuple(k8.shape)}, got {tuple(kcache.shape)}, {tuple(vcache.shape)}")
    nkv, smax, _ = k8.shape
    _lib.call("vl2_kv_quant", _p(kcache), _p(vcache), _p(k8), _p(v8), _p(ks), _p(vs), nkv, smax, int(p0), int(p1), _stream())
    return kv8


def attn_decode_kv8(qkv, kv8, cos_t, sin_t, partial, out, nh, nkv, pos, scale, pos_dev=None, ctx_cap=0):
    """include/vl2hip.h vl2_attn_decode_kv8: `attn_decode` on one sequence's fp8 cache kv8 = (k8, v8, ks, vs): the new token's K / V rows are
    quantised into row `pos` (or *pos_dev), the attention reads codes and scales."""
    k8, v8, ks, vs = _chk_kv8(kv8)
    if k8.dim() != 3:
        raise ValueError(f"attn_decode_kv8: one sequence's cache [nkv, smax, 128], got {tuple(k8.shape)}")
    _lib.call("vl2_attn_decode_kv8", _p(qkv), _p(k8), _p(v8), _p(ks), _p(vs), _p(cos_t), _p(sin_t), _p(partial), _p(out), nh, nkv,
              k8.shape[1], int(pos), _p(pos_dev), int(ctx_cap), float(scale), _stream())
    return out


def attn_decode_kv8_batched(qkv, kv8, cos_t, sin_t, partial, out, nh, nkv, pos_dev, ctx_cap, scale):
    """include/vl2hip.h vl2_attn_decode_kv8_batched: `attn_decode_batched` on the slots' fp8 caches kv8 = (k8, v8, ks, vs) with a leading
    slot dimension: codes [B, nkv, smax, 128], scales [B, nkv, smax]."""
    k8, v8, ks, vs = _chk_kv8(kv8)
    B = qkv.shape[0]
    if k8.dim() != 4 or k8.shape[0] != B or v8.stride(0) != k8.stride(0) or vs.stride(0) != ks.stride(0):
        raise ValueError(f"attn_decode_kv8_batched: need the {B} sequences' caches [B, nkv, smax, 128] with equal strides, got {tuple(k8.shape)}")
    _lib.call("vl2_attn_decode_kv8_batched", _p(qkv), _p(k8), _p(v8), _p(ks), _p(vs), _p(cos_t), _p(sin_t), _p(partial), _p(out), B,
              qkv.stride(0), k8.stride(0), ks.stride(0), out.stride(0), nh, nkv, k8.shape[2], _p(pos_dev), int(ctx_cap), float(scale), _stream())
    return out


KV_PAGE_ROWS = 64      # positions per page of the paged KV cache = keys per slice of the decode attention (csrc/k_attn_paged.h)


def kv_pool_alloc(n_pages, nkv, device):
    """One layer's page pools (include/vl2hip.h, csrc/k_attn_paged.h) as (kpool, vpool): [n_pages, nkv, 64, 128] elements of the build's
    16-bit type, zero (page 0, the parking page, must hold finite rows)."""
    n_pages = int(n_pages)
    if n_pages < 1 or nkv <= 0:
        raise ValueError(f"kv_pool_alloc: need n_pages >= 1 (the parking page) and nkv > 0, got {n_pages}, {nkv}")
    mk = lambda: torch.zeros((n_pages, nkv, KV_PAGE_ROWS, 128), dtype=_lib.elem_dtype(), device=device)
    return mk(), mk()


def _dtypes(who, *triples):
    """dtype checks that come before the shape checks (and before `_chk`, which asks for a device tensor first)."""
    for t, dt, name in triples:
        if t.dtype != dt:
            raise TypeError(f"{who}: {name} must be {dt}, got {t.dtype}")


def _chk_pools(who, kpool, vpool, nkv=None):
    _dtypes(who, (kpool, _lib.elem_dtype(), "kpool"), (vpool, _lib.elem_dtype(), "vpool"))
    if kpool.dim() != 4 or tuple(kpool.shape[2:]) != (KV_PAGE_ROWS, 128) or vpool.shape != kpool.shape or (nkv is not None and kpool.shape[1] != nkv):
        raise ValueError(f"{who}: the pools must be [n_pages, nkv, 64, 128], got {tuple(kpool.shape)}, {tuple(vpool.shape)}")
    if not (kpool.is_contiguous() and vpool.is_contiguous()):
        raise ValueError(f"{who}: the pools' pages must be contiguous")
    return kpool.shape[0], kpool.shape[1]


def kv_page_scatter(kcache, vcache, kpool, vpool, table_row, p0, p1):
    """include/vl2hip.h vl2_kv_page_scatter: rows [p0, p1) of one sequence's contiguous 16-bit caches [nkv, smax, 128] -> the pages its table
    row names (int32 [>= ceil(smax / 64)], contiguous), byte for byte; rows whose page id is outside the pools are skipped."""
    e = _lib.elem_dtype()
    _dtypes("kv_page_scatter", (kcache, e, "kcache"), (vcache, e, "vcache"), (table_row, torch.int32, "table_row"))
    n_pages, nkv = _chk_pools("kv_page_scatter", kpool, vpool)
    if kcache.dim() != 3 or kcache.shape[0] != nkv or kcache.shape[2] != 128 or vcache.shape != kcache.shape or \
            not (kcache.is_contiguous() and vcache.is_contiguous()):
        raise ValueError(f"kv_page_scatter: need contiguous 16-bit caches [nkv = {nkv}, smax, 128], got {tuple(kcache.shape)}, {tuple(vcache.shape)}")
    smax = kcache.shape[1]
    if table_row.dim() != 1 or not table_row.is_contiguous() or table_row.numel() < (smax + KV_PAGE_ROWS - 1) // KV_PAGE_ROWS:
        raise ValueError(f"kv_page_scatter: the table row must be a contiguous int32 vector of at least {(smax + KV_PAGE_ROWS - 1) // KV_PAGE_ROWS} "
                         f"entries, got {tuple(table_row.shape)}")
    p0, p1 = int(p0), int(p1)
    if not 0 <= p0 <= p1 <= smax:
        raise ValueError(f"kv_page_scatter: rows [{p0}, {p1}) outside the cache ({smax})")
    for t, name in ((kcache, "kcache"), (vcache, "vcache"), (kpool, "kpool"), (vpool, "vpool"), (table_row, "table_row")):
        _chk(t, t.dtype, name)
    _lib.call("vl2_kv_page_scatter", _p(kcache), _p(vcache), _p(kpool), _p(vpool), _p(table_row), nkv, smax, n_pages, p0, p1, _stream())


def attn_decode_paged(qkv, kpool, vpool, table, cos_t, sin_t, partial, out, nh, nkv, pos_dev, ctx_cap, scale):
    """include/vl2hip.h vl2_attn_decode_paged: `attn_decode_batched` on the paged cache.  qkv [B, (nh+2nkv)*128] un-roped, pools
    [n_pages, nkv, 64, 128], table int32 [>= B, pages_per_seq] (row b: request b's pages, -1 = not assigned), out [B, nh*128], pos_dev int32
    [B]; seq_cap = 64 * pages_per_seq, which cos_t / sin_t must cover; partial: B * nh * ceil(ctx_cap/64) * 130 floats.  Bit for bit
    `attn_decode_batched` on contiguous copies of the same rows.  Everything is checked here, before the library is called."""
    if qkv.dim() != 2 or nh <= 0 or nkv <= 0 or nh % nkv or qkv.shape[1] != (nh + 2 * nkv) * 128:
        raise ValueError(f"attn_decode_paged: qkv must be [B, (nh + 2 nkv) * 128] with nh = nkv * group, got {tuple(qkv.shape)} for nh {nh}, nkv {nkv}")
    B = qkv.shape[0]
    e = _lib.elem_dtype()
    operands = ((qkv, e, "qkv"), (out, e, "out"), (cos_t, torch.float32, "cos_t"), (sin_t, torch.float32, "sin_t"),
                (partial, torch.float32, "partial"), (pos_dev, torch.int32, "pos_dev"), (table, torch.int32, "table"))
    _dtypes("attn_decode_paged", *operands)
    n_pages, _ = _chk_pools("attn_decode_paged", kpool, vpool, nkv)
    if table.dim() != 2 or table.shape[0] < B or table.shape[1] < 1 or table.stride(1) != 1:
        raise ValueError(f"attn_decode_paged: the page table must be int32 [>= {B}, pages_per_seq], got {tuple(table.shape)}")
    seq_cap = table.shape[1] * KV_PAGE_ROWS
    ctx_cap = int(ctx_cap)
    if not 0 < ctx_cap <= seq_cap:
        raise ValueError(f"attn_decode_paged: ctx_cap {ctx_cap} outside the table's {seq_cap} positions")
    if cos_t.shape != sin_t.shape or cos_t.dim() != 2 or cos_t.shape[1] != 64 or cos_t.shape[0] < seq_cap or not (cos_t.is_contiguous() and sin_t.is_contiguous()):
        raise ValueError(f"attn_decode_paged: positions up to {seq_cap - 1} need contiguous cos / sin tables [>= {seq_cap}, 64], got {tuple(cos_t.shape)}")
    if pos_dev.numel() < B or out.dim() != 2 or out.shape[0] < B or out.shape[1] != nh * 128:
        raise ValueError(f"attn_decode_paged: need {B} positions and out [B, nh * 128], got {pos_dev.numel()}, {tuple(out.shape)}")
    need = B * nh * ((ctx_cap + 63) // 64) * 130
    if partial.numel() < need:
        raise ValueError(f"attn_decode_paged: partial holds {partial.numel()} floats, need {need}")
    for t, dt, name in operands + ((kpool, e, "kpool"), (vpool, e, "vpool")):
        _chk(t, dt, name)
    _lib.call("vl2_attn_decode_paged", _p(qkv), _p(kpool), _p(vpool), _p(table), _p(cos_t), _p(sin_t), _p(partial), _p(out), B, qkv.stride(0),
              table.stride(0), n_pages, out.stride(0), nh, nkv, seq_cap, _p(pos_dev), ctx_cap, float(scale), _stream())
    return out


def kv8_pool_alloc(n_pages, nkv, device):
    """One layer's fp8 page pools (include/vl2hip.h, csrc/k_attn_paged_kv8.h) as (k8pool, v8pool, kspool, vspool): e4m3fn codes uint8
    [n_pages, nkv, 64, 128], zero, and fp32 row scales [n_pages, nkv, 64], one (page 0, the parking page, must dequantise to finite rows)."""
    n_pages = int(n_pages)
    if n_pages < 1 or nkv <= 0:
        raise ValueError(f"kv8_pool_alloc: need n_pages >= 1 (the parking page) and nkv > 0, got {n_pages}, {nkv}")
    codes = lambda: torch.zeros((n_pages, nkv, KV_PAGE_ROWS, 128), dtype=torch.uint8, device=device)
    scales = lambda: torch.ones((n_pages, nkv, KV_PAGE_ROWS), dtype=torch.float32, device=device)
    return codes(), codes(), scales(), scales()


def _chk_pools8(who, pools8, nkv=None):
    k8pool, v8pool, kspool, vspool = pools8
    _dtypes(who, (k8pool, torch.uint8, "k8pool"), (v8pool, torch.uint8, "v8pool"), (kspool, torch.float32, "kspool"), (vspool, torch.float32, "vspool"))
    if k8pool.dim() != 4 or tuple(k8pool.shape[2:]) != (KV_PAGE_ROWS, 128) or v8pool.shape != k8pool.shape or kspool.shape != k8pool.shape[:3] or \
            vspool.shape != kspool.shape or (nkv is not None and k8pool.shape[1] != nkv):
        raise ValueError(f"{who}: the pools must be codes [n_pages, nkv, 64, 128] and scales [n_pages, nkv, 64], got {tuple(k8pool.shape)}, "
                         f"{tuple(v8pool.shape)}, {tuple(kspool.shape)}, {tuple(vspool.shape)}")
    if not all(t.is_contiguous() for t in pools8):
        raise ValueError(f"{who}: the pools' pages must be contiguous")
    return k8pool.shape[0], k8pool.shape[1]


def kv_page_quant(kcache, vcache, pools8, table_row, p0, p1):
    """include/vl2hip.h vl2_kv_page_quant: rows [p0, p1) of one sequence's contiguous 16-bit caches [nkv, smax, 128] -> e4m3fn codes and
    power-of-two row scales in the pages its table row names (int32 [>= ceil(smax / 64)], contiguous) of pools8 = (k8pool, v8pool, kspool,
    vspool): byte for byte what `kv_quant` writes at those rows of a contiguous fp8 cache; rows whose page id is outside the pools are skipped."""
    e = _lib.elem_dtype()
    _dtypes("kv_page_quant", (kcache, e, "kcache"), (vcache, e, "vcache"), (table_row, torch.int32, "table_row"))
    n_pages, nkv = _chk_pools8("kv_page_quant", pools8)
    if kcache.dim() != 3 or kcache.shape[0] != nkv or kcache.shape[2] != 128 or vcache.shape != kcache.shape or \
            not (kcache.is_contiguous() and vcache.is_contiguous()):
        raise ValueError(f"kv_page_quant: need contiguous 16-bit caches [nkv = {nkv}, smax, 128], got {tuple(kcache.shape)}, {tuple(vcache.shape)}")
    smax = kcache.shape[1]
    if table_row.dim() != 1 or not table_row.is_contiguous() or table_row.numel() < (smax + KV_PAGE_ROWS - 1) // KV_PAGE_ROWS:
        raise ValueError(f"kv_page_quant: the table row must be a contiguous int32 vector of at least {(smax + KV_PAGE_ROWS - 1) // KV_PAGE_ROWS} "
                         f"entries, got {tuple(table_row.shape)}")
    p0, p1 = int(p0), int(p1)
    if not 0 <= p0 <= p1 <= smax:
        raise ValueError(f"kv_page_quant: rows [{p0}, {p1}) outside the cache ({smax})")
    k8pool, v8pool, kspool, vspool = pools8
    for t, name in ((kcache, "kcache"), (vcache, "vcache"), (k8pool, "k8pool"), (v8pool, "v8pool"), (kspool, "kspool"), (vspool, "vspool"),
                    (table_row, "table_row")):
        _chk(t, t.dtype, name)
    _lib.call("vl2_kv_page_quant", _p(kcache), _p(vcache), _p(k8pool), _p(v8pool), _p(kspool), _p(vspool), _p(table_row), nkv, smax, n_pages,
              p0, p1, _stream())


def kv_pages_move(pool, arena, page_ids, to_arena):
    """include/vl2hip.h vl2_kv_pages_move: the n = len(page_ids) whole pages of ONE pool tensor that page_ids (int32 [n], contiguous) names to
    (to_arena=True) or from (False) slots 0 .. n-1 of the packed device arena, byte for byte.  pool: contiguous, one of the three pool kinds --
    [n_pages, nkv, 64, 128] of the build's 16-bit type or of uint8 codes, [n_pages, nkv, 64] of fp32 row scales; arena: contiguous, the pool's
    dtype and page shape, at least n slots.  An id outside [1, n_pages) is skipped.  Everything is checked here, before the library is called;
    n == 0 returns after the checks without calling it (an empty tensor has no address to hand over)."""
    kinds = ((_lib.elem_dtype(), (KV_PAGE_ROWS, 128)), (torch.uint8, (KV_PAGE_ROWS, 128)), (torch.float32, (KV_PAGE_ROWS,)))
    if pool.dtype not in [k[0] for k in kinds]:
        raise TypeError(f"kv_pages_move: pool must be {_lib.elem_dtype()} rows, torch.uint8 codes or torch.float32 row scales, got {pool.dtype}")
    _dtypes("kv_pages_move", (arena, pool.dtype, "arena"), (page_ids, torch.int32, "page_ids"))
    tail = dict(kinds)[pool.dtype]
    if pool.dim() != 2 + len(tail) or tuple(pool.shape[2:]) != tail or pool.shape[0] < 1 or pool.shape[1] < 1:
        raise ValueError(f"kv_pages_move: a {pool.dtype} pool must be [n_pages, nkv, {', '.join(map(str, tail))}], got {tuple(pool.shape)}")
    if not (pool.is_contiguous() and arena.is_contiguous()):
        raise ValueError("kv_pages_move: the pool's and the arena's pages must be contiguous")
    if page_ids.dim() != 1 or not page_ids.is_contiguous():
        raise ValueError(f"kv_pages_move: page_ids must be a contiguous int32 vector, got {tuple(page_ids.shape)}")
    n = page_ids.numel()
    if arena.dim() != pool.dim() or arena.shape[1:] != pool.shape[1:] or arena.shape[0] < n:
        raise ValueError(f"kv_pages_move: the arena must hold at least {n} pages of {tuple(pool.shape[1:])}, got {tuple(arena.shape)}")
    page_bytes = pool.stride(0) * pool.element_size()
    if page_bytes % 16:
        raise ValueError(f"kv_pages_move: a page of {page_bytes} bytes is no multiple of 16")
    for t, name in ((pool, "pool"), (arena, "arena"), (page_ids, "page_ids")):
        _chk(t, t.dtype, name)
    if not (pool.device == arena.device == page_ids.device):
        raise ValueError(f"kv_pages_move: pool, arena and page_ids must be on one device, got {pool.device}, {arena.device}, {page_ids.device}")
    if n == 0:
        return
    _lib.call("vl2_kv_pages_move", _p(pool), _p(arena), _p(page_ids), n, pool.shape[0], page_bytes, 1 if to_arena else 0, _stream())


def attn_decode_kv8_paged(qkv, pools8, table, cos_t, sin_t, partial, out, nh, nkv, pos_dev, ctx_cap, scale):
    """include/vl2hip.h vl2_attn_decode_kv8_paged: `attn_decode_kv8_batched` on the paged fp8 cache.  qkv [B, (nh+2nkv)*128] un-roped, pools8 =
    (k8pool, v8pool, kspool, vspool): codes uint8 [n_pages, nkv, 64, 128] and scales fp32 [n_pages, nkv, 64]; table, out, pos_dev, seq_cap,
    cos_t / sin_t and partial as `attn_decode_paged`.  Bit for bit `attn_decode_kv8_batched` on contiguous copies of the same codes and scales.
    Everything is checked here, before the library is called."""
    if qkv.dim() != 2 or nh <= 0 or nkv <= 0 or nh % nkv or qkv.shape[1] != (nh + 2 * nkv) * 128:
        raise ValueError(f"attn_decode_kv8_paged: qkv must be [B, (nh + 2 nkv) * 128] with nh = nkv * group, got {tuple(qkv.shape)} for nh {nh}, "
                         f"nkv {nkv}")
    B = qkv.shape[0]
    e = _lib.elem_dtype()
    operands = ((qkv, e, "qkv"), (out, e, "out"), (cos_t, torch.float32, "cos_t"), (sin_t, torch.float32, "sin_t"),
                (partial, torch.float32, "partial"), (pos_dev, torch.int32, "pos_dev"), (table, torch.int32, "table"))
    _dtypes("attn_decode_kv8_paged", *operands)
    n_pages, _ = _chk_pools8("attn_decode_kv8_paged", pools8, nkv)
    if table.dim() != 2 or table.shape[0] < B or table.shape[1] < 1 or table.stride(1) != 1:
        raise ValueError(f"attn_decode_kv8_paged: the page table must be int32 [>= {B}, pages_per_seq], got {tuple(table.shape)}")
    seq_cap = table.shape[1] * KV_PAGE_ROWS
    ctx_cap = int(ctx_cap)
    if not 0 < ctx_cap <= seq_cap:
        raise ValueError(f"attn_decode_kv8_paged: ctx_cap {ctx_cap} outside the table's {seq_cap} positions")
    if cos_t.shape != sin_t.shape or cos_t.dim() != 2 or cos_t.shape[1] != 64 or cos_t.shape[0] < seq_cap or not (cos_t.is_contiguous() and sin_t.is_contiguous()):
        raise ValueError(f"attn_decode_kv8_paged: positions up to {seq_cap - 1} need contiguous cos / sin tables [>= {seq_cap}, 64], got "
                         f"{tuple(cos_t.shape)}")
    if pos_dev.numel() < B or out.dim() != 2 or out.shape[0] < B or out.shape[1] != nh * 128:
        raise ValueError(f"attn_decode_kv8_paged: need {B} positions and out [B, nh * 128], got {pos_dev.numel()}, {tuple(out.shape)}")
    need = B * nh * ((ctx_cap + 63) // 64) * 130
    if partial.numel() < need:
        raise ValueError(f"attn_decode_kv8_paged: partial holds {partial.numel()} floats, need {need}")
    k8pool, v8pool, kspool, vspool = pools8
    for t, dt, name in operands + ((k8pool, torch.uint8, "k8pool"), (v8pool, torch.uint8, "v8pool"), (kspool, torch.float32, "kspool"),
                                   (vspool, torch.float32, "vspool")):
        _chk(t, dt, name)
    _lib.call("vl2_attn_decode_kv8_paged", _p(qkv), _p(k8pool), _p(v8pool), _p(kspool), _p(vspool), _p(table), _p(cos_t), _p(sin_t), _p(partial),
              _p(out), B, qkv.stride(0), table.stride(0), n_pages, out.stride(0), nh, nkv, seq_cap, _p(pos_dev), ctx_cap, float(scale), _stream())
    return out


_APPEND_WS = {}


def attn_append(q, kcache, vcache, out, P, nh, nkv, scale, ws=None):
    """include/vl2hip.h vl2_attn_append: the n = q.shape[0] roped query rows q [n, nh*128] at positions P .. P+n-1 attend causally to the
    P + n keys of one sequence's caches [nkv, smax, 128] (rows P .. P+n-1 already appended) -> out [n, nh*128].  ws: fp32 workspace of at
    least vl2_attn_append_ws_bytes (default: one per device, grown on demand)."""
    _chk(q, _lib.elem_dtype(), "q"); _chk(kcache, _lib.elem_dtype(), "kcache"); _chk(vcache, _lib.elem_dtype(), "vcache")
    _chk(out, _lib.elem_dtype(), "out"); _chk(ws, torch.float32, "ws")
    n = q.shape[0]
    need = int(_lib.load().vl2_attn_append_ws_bytes(int(P), n, nh))
    if ws is None:
        key = str(q.device)
        ws = _APPEND_WS.get(key)
        if ws is None or ws.numel() * 4 < need:
            ws = _APPEND_WS[key] = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=q.device)
    _lib.call("vl2_attn_append", _p(q), q.stride(0), _p(kcache), _p(vcache), _p(out), out.stride(0), int(P), n, nh, nkv, kcache.shape[-2],
              float(scale), _p(ws), ws.numel() * 4, _stream())
    return out


def shared_prefix_splits(P):
    """Splits of the prefix keys [0, P) in vl2_attn_decode_shared (csrc/vl2_abi.hip attn_shared_split): a function of P alone -- at least
    two 64-key tiles per split, at most 24 splits."""
    tiles = (P + 63) // 64
    chunk = max((tiles + 23) // 24, 2) * 64
    return (P + chunk - 1) // chunk


def shared_own_cap(longest_suffix, max_new_tokens):
    """Rows of a request's private cache in the shared-prefix mode: its suffix and every token it may feed, rounded up to the 64-key slice."""
    return (int(longest_suffix) + int(max_new_tokens) + 63) // 64 * 64


def shared_live_slices(P, pos):
    """Slices the combine of vl2_attn_decode_shared merges for a request whose new token sits at absolute position pos >= P."""
    return shared_prefix_splits(P) + (pos - P + 64) // 64


def shared_partial_floats(P, own_cap, nh):
    """Floats ONE request takes in the `partial` workspace of vl2_attn_decode_shared (= vl2_attn_decode_shared_partial_floats)."""
    return nh * (shared_prefix_splits(P) + own_cap // 64) * 130


def attn_decode_shared(qkv, kprefix, vprefix, kown, vown, cos_t, sin_t, partial, out, nh, nkv, P, pos_dev, scale):
    """include/vl2hip.h vl2_attn_decode_shared: the batched decode attention of B = qkv.shape[0] requests that share the keys of positions
    [0, P) in ONE cache kprefix / vprefix [nkv, smax, 128] and keep their own rows, from position P on, in kown / vown [B, nkv, own_cap, 128]
    (private row = position - P; own_cap a multiple of 64).  qkv [B, (nh+2nkv)*128] un-roped, pos_dev int32 [B] absolute positions, out
    [B, nh*128]; partial: fp32, at least B * shared_partial_floats(P, own_cap, nh) floats.  Everything is checked here, before the library
    is called."""
    P = int(P)
    if qkv.dim() != 2 or nh <= 0 or nkv <= 0 or nh % nkv or qkv.shape[1] != (nh + 2 * nkv) * 128:
        raise ValueError(f"attn_decode_shared: qkv must be [B, (nh + 2 nkv) * 128] with nh = nkv * group, got {tuple(qkv.shape)} for nh {nh}, nkv {nkv}")
    B = qkv.shape[0]
    if kprefix.dim() != 3 or kprefix.shape[0] != nkv or kprefix.shape[2] != 128 or vprefix.shape != kprefix.shape or \
            not (kprefix.is_contiguous() and vprefix.is_contiguous()):
        raise ValueError(f"attn_decode_shared: the prefix caches must be contiguous [nkv, smax, 128], got {tuple(kprefix.shape)}, {tuple(vprefix.shape)}")
    if not 0 < P <= kprefix.shape[1]:
        raise ValueError(f"attn_decode_shared: a prefix of {P} rows is outside the prefix cache ({kprefix.shape[1]} rows)")
    if kown.dim() != 4 or kown.shape[0] < B or kown.shape[1] != nkv or kown.shape[3] != 128 or vown.shape != kown.shape or \
            vown.stride() != kown.stride() or not kown[0].is_contiguous():
        raise ValueError(f"attn_decode_shared: the private caches must be [B, nkv, own_cap, 128] with contiguous slots, got {tuple(kown.shape)}, "
                         f"{tuple(vown.shape)}")
    own_cap = kown.shape[2]
    if own_cap % 64:
        raise ValueError(f"attn_decode_shared: own_cap {own_cap} must be a multiple of 64")
    if cos_t.shape != sin_t.shape or cos_t.dim() != 2 or cos_t.shape[1] != 64 or P + own_cap > cos_t.shape[0]:
        raise ValueError(f"attn_decode_shared: positions up to {P + own_cap - 1} need cos / sin tables [>= {P + own_cap}, 64], got {tuple(cos_t.shape)}")
    if pos_dev.numel() < B or out.dim() != 2 or out.shape[0] < B or out.shape[1] != nh * 128:
        raise ValueError(f"attn_decode_shared: need {B} positions and out [B, nh * 128], got {pos_dev.numel()}, {tuple(out.shape)}")
    need = B * shared_partial_floats(P, own_cap, nh)
    if partial.numel() < need:
        raise ValueError(f"attn_decode_shared: partial holds {partial.numel()} floats, need {need}")
    e = _lib.elem_dtype()
    for t, dt, name in ((qkv, e, "qkv"), (kprefix, e, "kprefix"), (vprefix, e, "vprefix"), (kown, e, "kown"), (vown, e, "vown"), (out, e, "out"),
                        (cos_t, torch.float32, "cos_t"), (sin_t, torch.float32, "sin_t"), (partial, torch.float32, "partial"),
                        (pos_dev, torch.int32, "pos_dev")):
        _chk(t, dt, name)
    _lib.call("vl2_attn_decode_shared", _p(qkv), _p(kprefix), _p(vprefix), _p(kown), _p(vown), _p(cos_t), _p(sin_t), _p(partial), partial.numel(),
              _p(out), B, qkv.stride(0), kown.stride(0), out.stride(0), nh, nkv, P, kprefix.shape[1], own_cap, cos_t.shape[0], _p(pos_dev),
              float(scale), _stream())
    return out


def kv_page_gather(kpool, vpool, kcache, vcache, table_row, p0, p1):
    """include/vl2hip.h vl2_kv_page_gather, the inverse of `kv_page_scatter`: rows [p0, p1) of the pages a table row names (int32
    [>= ceil(smax / 64)], contiguous) -> one sequence's contiguous 16-bit caches [nkv, smax, 128], byte for byte; rows whose page id is outside
    the pools are skipped and nothing else in the caches is written."""
    e = _lib.elem_dtype()
    _dtypes("kv_page_gather", (kcache, e, "kcache"), (vcache, e, "vcache"), (table_row, torch.int32, "table_row"))
    n_pages, nkv = _chk_pools("kv_page_gather", kpool, vpool)
    if kcache.dim() != 3 or kcache.shape[0] != nkv or kcache.shape[2] != 128 or vcache.shape != kcache.shape or \
            not (kcache.is_contiguous() and vcache.is_contiguous()):
        raise ValueError(f"kv_page_gather: need contiguous 16-bit caches [nkv = {nkv}, smax, 128], got {tuple(kcache.shape)}, {tuple(vcache.shape)}")
    smax = kcache.shape[1]
    if table_row.dim() != 1 or not table_row.is_contiguous() or table_row.numel() < (smax + KV_PAGE_ROWS - 1) // KV_PAGE_ROWS:
        raise ValueError(f"kv_page_gather: the table row must be a contiguous int32 vector of at least {(smax + KV_PAGE_ROWS - 1) // KV_PAGE_ROWS} "
                         f"entries, got {tuple(table_row.shape)}")
    p0, p1 = int(p0), int(p1)
    if not 0 <= p0 <= p1 <= smax:
        raise ValueError(f"kv_page_gather: rows [{p0}, {p1}) outside the cache ({smax})")
    for t, name in ((kcache, "kcache"), (vcache, "vcache"), (kpool, "kpool"), (vpool, "vpool"), (table_row, "table_row")):
        _chk(t, t.dtype, name)
    _lib.call("vl2_kv_page_gather", _p(kpool), _p(vpool), _p(kcache), _p(vcache), _p(table_row), nkv, smax, n_pages, p0, p1, _stream())


def attn_decode_shared_paged(qkv, kpool, vpool, table, prefix_pages, cos_t, sin_t, partial, out, nh, nkv, P, own_cap, pos_dev, scale):
    """include/vl2hip.h vl2_attn_decode_shared_paged: `attn_decode_shared` with the shared prefix and the own rows in pages of one pool.  P (a
    positive multiple of 64) shared positions live in the pages prefix_pages (int32 [>= P / 64], contiguous) for every request; request b's own
    rows from position P on live in the pages table[b, P / 64 + s], s < own_cap / 64 (own_cap a multiple of 64).  qkv [B, (nh+2nkv)*128]
    un-roped, pools [n_pages, nkv, 64, 128], table int32 [>= B, >= P / 64 + own_cap / 64], pos_dev int32 [B] absolute positions, out
    [B, nh*128]; partial: at least B * shared_partial_floats(P, own_cap, nh) floats.  Bit for bit `attn_decode_shared` on contiguous copies of
    the same rows.  Everything is checked here, before the library is called."""
    P, own_cap = int(P), int(own_cap)
    if qkv.dim() != 2 or nh <= 0 or nkv <= 0 or nh % nkv or qkv.shape[1] != (nh + 2 * nkv) * 128:
        raise ValueError(f"attn_decode_shared_paged: qkv must be [B, (nh + 2 nkv) * 128] with nh = nkv * group, got {tuple(qkv.shape)} for nh {nh}, "
                         f"nkv {nkv}")
    B = qkv.shape[0]
    e = _lib.elem_dtype()
    operands = ((qkv, e, "qkv"), (out, e, "out"), (cos_t, torch.float32, "cos_t"), (sin_t, torch.float32, "sin_t"),
                (partial, torch.float32, "partial"), (pos_dev, torch.int32, "pos_dev"), (table, torch.int32, "table"),
                (prefix_pages, torch.int32, "prefix_pages"))
    _dtypes("attn_decode_shared_paged", *operands)
    n_pages, _ = _chk_pools("attn_decode_shared_paged", kpool, vpool, nkv)
    if P <= 0 or P % KV_PAGE_ROWS:
        raise ValueError(f"attn_decode_shared_paged: P {P} must be a positive multiple of 64 (whole pages are shared)")
    if own_cap <= 0 or own_cap % KV_PAGE_ROWS:
        raise ValueError(f"attn_decode_shared_paged: own_cap {own_cap} must be a positive multiple of 64")
    if table.dim() != 2 or table.shape[0] < B or table.stride(1) != 1 or table.shape[1] < (P + own_cap) // KV_PAGE_ROWS:
        raise ValueError(f"attn_decode_shared_paged: the page table must be int32 [>= {B}, >= {(P + own_cap) // KV_PAGE_ROWS}] ({P // KV_PAGE_ROWS} "
                         f"prefix + {own_cap // KV_PAGE_ROWS} own pages), got {tuple(table.shape)}")
    if prefix_pages.dim() != 1 or not prefix_pages.is_contiguous() or prefix_pages.numel() < P // KV_PAGE_ROWS:
        raise ValueError(f"attn_decode_shared_paged: prefix_pages must be a contiguous int32 vector of at least {P // KV_PAGE_ROWS} entries, got "
                         f"{tuple(prefix_pages.shape)}")
    if cos_t.shape != sin_t.shape or cos_t.dim() != 2 or cos_t.shape[1] != 64 or cos_t.shape[0] < P + own_cap or \
            not (cos_t.is_contiguous() and sin_t.is_contiguous()):
        raise ValueError(f"attn_decode_shared_paged: positions up to {P + own_cap - 1} need contiguous cos / sin tables [>= {P + own_cap}, 64], got "
                         f"{tuple(cos_t.shape)}")
    if pos_dev.numel() < B or out.dim() != 2 or out.shape[0] < B or out.shape[1] != nh * 128:
        raise ValueError(f"attn_decode_shared_paged: need {B} positions and out [B, nh * 128], got {pos_dev.numel()}, {tuple(out.shape)}")
    need = B * shared_partial_floats(P, own_cap, nh)
    if partial.numel() < need:
        raise ValueError(f"attn_decode_shared_paged: partial holds {partial.numel()} floats, need {need}")
    for t, dt, name in operands + ((kpool, e, "kpool"), (vpool, e, "vpool")):
        _chk(t, dt, name)
    _lib.call("vl2_attn_decode_shared_paged", _p(qkv), _p(kpool), _p(vpool), _p(table), _p(prefix_pages), _p(cos_t), _p(sin_t), _p(partial),
              partial.numel(), _p(out), B, qkv.stride(0), table.stride(0), n_pages, out.stride(0), nh, nkv, P, own_cap, cos_t.shape[0],
              _p(pos_dev), float(scale), _stream())
    return out


def argmax(logits, tok, hist=None, step=0, state=None):
    _lib.call("vl2_argmax", _p(logits), logits.numel(), _p(tok), _p(hist), step, _p(state), _stream())


def sample_token(logits, tok, u, temperature, top_k=50, top_p=1.0, hist=None, step=0, state=None, dbg=None):
    """One sampled token from fp32 logits (include/vl2hip.h vl2_sample_token): temperature -> top-k -> top-p (HF's warpers, HF's order), then the
    inverse CDF of the kept, renormalised probabilities at u[step] (u: device fp32 uniforms in [0, 1)).  tok / hist / step / state as `argmax`."""
    _chk(logits, torch.float32, "logits"); _chk(u, torch.float32, "u"); _chk(dbg, torch.float32, "dbg")
    _lib.call("vl2_sample_token", _p(logits), logits.numel(), float(temperature), int(top_k), float(top_p), _p(u), _p(tok), _p(hist), int(step),
              _p(state), _p(dbg), _stream())


def sample_tokens(logits, temperature, top_k, top_p, u, step, tok):
    """The draws of nb rows in ONE launch (include/vl2hip.h vl2_sample_tokens): logits [nb, V] fp32; per row temperature (fp32, <= 0 = greedy: the
    `argmax` token), top_k (int32), top_p (fp32), its uniform numbers u [nb, n] (fp32, contiguous) and step (int32: a sampled row draws at
    u[b, step[b]] -- `sample_token`'s token -- and advances it); tok [nb] int32 receives the tokens."""
    _chk(logits, torch.float32, "logits"); _chk(temperature, torch.float32, "temperature"); _chk(top_k, torch.int32, "top_k")
    _chk(top_p, torch.float32, "top_p"); _chk(u, torch.float32, "u"); _chk(step, torch.int32, "step"); _chk(tok, torch.int32, "tok")
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be [nb, V] with unit column stride")
    nb = logits.shape[0]
    if u.dim() != 2 or u.shape[0] < nb or u.stride(1) != 1 or u.stride(0) != u.shape[1]:
        raise ValueError("u must be a contiguous [>= nb, n] tensor")
    for t, n in ((temperature, "temperature"), (top_k, "top_k"), (top_p, "top_p"), (step, "step"), (tok, "tok")):
        if t.dim() != 1 or t.numel() < nb or t.stride(0) != 1:
            raise ValueError(f"{n} must be a contiguous vector of >= {nb} entries")
    _lib.call("vl2_sample_tokens", _p(logits), logits.stride(0), logits.shape[1], nb, _p(temperature), _p(top_k), _p(top_p), _p(u), u.stride(0),
              _p(step), _p(tok), _stream())


def embed_rows(ids_i32, table, out):
    _lib.call("vl2_embed_rows", _p(ids_i32), _p(table), _p(out), ids_i32.numel(), table.shape[1], out.stride(0), _stream())
    return out


# ------------------------------------------------------------------------------------------------ one-time weight re-layout
# The C-ABI forms of what weights.py does with tensor ops (include/vl2hip.h vl2_pack_*): for hosts without PyTorch; here they are
# bound so that the tests can hold them against weights.py byte for byte.
def pack_fold_norm(w, g, beta=None, bias=None):
    """(W' bf16 [N,K], colsum fp32 [N], shift fp32 [N] or None) = weights.fold_norm(w, g, beta, bias)."""
    for t, n in ((w, "w"), (g, "g"), (beta, "beta"), (bias, "bias")):
        _chk(t, _lib.elem_dtype(), n)
    N, K = w.shape
    wp = torch.empty((N, K), dtype=_lib.elem_dtype(), device=w.device)
    s = torch.empty((N,), dtype=torch.float32, device=w.device)
    t = torch.empty((N,), dtype=torch.float32, device=w.device) if beta is not None else None
    _lib.call("vl2_pack_fold_norm", _p(w), _p(g), _p(beta), _p(bias), _p(wp), _p(s), _p(t), N, K, w.stride(0), _stream())
    return wp, s, t


def pack_gate_up(gate, up):
    _chk(gate, _lib.elem_dtype(), "gate"); _chk(up, _lib.elem_dtype(), "up")
    I, D = gate.shape
    out = torch.empty((2 * I, D), dtype=_lib.elem_dtype(), device=gate.device)
    _lib.call("vl2_pack_gate_up", _p(gate), _p(up), _p(out), I, D, _stream())
    return out


def pack_permute(x, out_f32=False):
    """[A, B, C] bf16 -> [A, C, B] (bf16, or fp32 with out_f32)."""
    _chk(x, _lib.elem_dtype(), "x")
    A, B, C = x.shape
    out = torch.empty((A, C, B), dtype=torch.float32 if out_f32 else _lib.elem_dtype(), device=x.device)
    _lib.call("vl2_pack_permute", _p(x), _p(out), A, B, C, int(out_f32), _stream())
    return out


def pack_pad_rows(x, cols_dst):
    _chk(x, _lib.elem_dtype(), "x")
    rows, cs = x.shape
    out = torch.empty((rows, cols_dst), dtype=_lib.elem_dtype(), device=x.device)
    _lib.call("vl2_pack_pad_rows", _p(x), _p(out), rows, cs, cols_dst, _stream())
    return out


def pack_cvt_f32(x):
    _chk(x, _lib.elem_dtype(), "x")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.call("vl2_pack_cvt_f32", _p(x), _p(out), x.numel(), _stream())
    return out


# ------------------------------------------------------------------------------------------------ stage-level entry points
# One C call per stage (include/vl2hip.h vl2_vit_forward / vl2_llm_prefill / vl2_llm_decode_step): the layer loop runs inside
# libvl2hip.so.  The descriptors hold raw device pointers, so every builder returns (desc, keepalive): the caller keeps
# `keepalive` (the tensors and the ctypes layer array) referenced for as long as the descriptor is used.
STAGE_ABI = True        # the towers / connector / decoder use the stage calls ...


def stage_enabled():
    """... unless a per-GEMM profile is being taken (ops.PROFILE) or one of the per-call experiment controls (forced GEMM
    variant, split-K, forced attention variant: set_gemm_variant / set_splitk / set_attn_kv_groups) is on: those are arguments of
    the per-operator entry points, the stage calls always use the library's own choice."""
    return STAGE_ABI and PROFILE is None and not (_CTL["variant"] or _CTL["splitk"] or _CTL["attn_variant"])


def vit_desc(w, v, family, act):
    """weights.pack_tower / pack_siglip_tower dict + vision config -> (_lib.VitDesc, keepalive)."""
    layers = (_lib.VitLayer * len(w["layers"]))()
    for i, lw in enumerate(w["layers"]):
        for n in ("wqkv", "bqkv", "sqkv", "wo", "bo", "w1", "b1", "s1", "w2", "b2"):
            setattr(layers[i], n, _p(lw[n]))
    nh = v["num_attention_heads"]
    hd_real = v["hidden_size"] // nh
    d = _lib.VitDesc(ctypes.sizeof(_lib.VitDesc), family, v["image_size"], v["patch_size"], v["hidden_size"], w["layers"][0]["w1"].shape[0], nh,
                     w.get("hdp", hd_real), len(w["layers"]), w["kp"], act, float(v["layer_norm_eps"]), float(hd_real ** -0.5),
                     _p(w["patch_w"]), _p(w.get("patch_b")), _p(w["pos"]), _p(w.get("cls_pos")), _p(w.get("pre_w")), _p(w.get("pre_b")), layers)
    return d, (layers, w)


def vit_forward(desc, frames, T, out, u8_norm=None):
    """frames [T,3,S,S] fp32 / fp16 / bf16 or uint8 [T,S,S,3] -> out [T * tokens, D] bf16 (class-token row included)."""
    code = 3 if frames.dtype == torch.uint8 else _DTYPE_CODE[frames.dtype]
    n = int(_lib.load().vl2_vit_workspace_bytes(ctypes.byref(desc), T))
    if n < 0:
        raise _lib.Vl2HipError("vl2_vit_workspace_bytes: bad descriptor")
    ws = torch.empty((n,), dtype=torch.uint8, device=out.device)
    nrm = (ctypes.c_float * 7)(*[float(x) for x in u8_norm]) if u8_norm is not None else None
    desc.flags = _CTL["stage_flags"]
    _lib.call("vl2_vit_forward", ctypes.byref(desc), _p(frames), code, ctypes.addressof(nrm) if nrm is not None else None, T, _p(out),
              _p(ws), n, _stream())
    return out


def stc_desc(w):
    """weights.pack_connector dict -> (_lib.StcDesc, keepalive)."""
    d = _lib.StcDesc()
    d.size = ctypes.sizeof(_lib.StcDesc)
    d.cin, d.C = w["s1"][0]["conv1_w"].shape[1], w["s1"][0]["conv1_w"].shape[0]
    for stage, blocks in (("s1", d.s1), ("s2", d.s2)):
        for i, b in enumerate(w[stage]):
            for n, _t in _lib.StcBlock._fields_[:-1]:
                setattr(blocks[i], n, _p(b.get(n)))
            blocks[i].rd = b["fc1_w"].shape[0]
    for n in ("samp_w", "samp_b", "ro0_w", "ro0_b", "ro2_w", "ro2_b"):
        setattr(d, n, _p(w[n]))
    return d, (w,)


def stc_forward(desc, x, T, hw, idx, dims, out):
    """x [T*hw*hw, cin] bf16 tower features -> out [To*Ho*Wo, C] bf16 (idx, dims from connector.conv3d_k2s2p1_index)."""
    _chk(x, _lib.elem_dtype(), "x"); _chk(out, _lib.elem_dtype(), "out"); _chk(idx, torch.int32, "idx")
    To, Ho, Wo = dims
    n = int(_lib.load().vl2_stc_workspace_bytes(ctypes.byref(desc), T, hw, To * Ho * Wo))
    if n < 0:
        raise _lib.Vl2HipError("vl2_stc_workspace_bytes: bad descriptor")
    ws = torch.empty((n,), dtype=torch.uint8, device=out.device)
    desc.flags = _CTL["stage_flags"]
    _lib.call("vl2_stc_forward", ctypes.byref(desc), _p(x), T, hw, _p(idx), To, Ho, Wo, _p(out), _p(ws), n, _stream())
    return out


def llm_desc(w, cfg_llm, nh, nkv, smax, eps, kcache, vcache, cos_t, sin_t, w8=None):
    """weights.pack_decoder dict + this decoder's caches -> (_lib.LlmDesc, keepalive).  w8: optional fp8 copies (decoder.enable_fp8_decode)."""
    layers = (_lib.LlmLayer * len(w["layers"]))()
    for i, lw in enumerate(w["layers"]):
        layers[i].wqkv, layers[i].bqkv, layers[i].wo = _p(lw["wqkv"]), _p(lw["bqkv"]), _p(lw["wo"])
        layers[i].wgu, layers[i].wd = _p(lw["wgu"]), _p(lw["wd"])
        layers[i].kcache, layers[i].vcache = _p(kcache[i]), _p(vcache[i])
    d = _lib.LlmDesc(ctypes.sizeof(_lib.LlmDesc), cfg_llm["hidden_size"], w["layers"][0]["wd"].shape[1], nh, nkv, len(w["layers"]),
                     w["lm_head"].shape[0], smax, float(eps), layers, _p(w["embed"]), _p(w["norm_w"]), _p(w["ones"]), _p(w["lm_head"]),
                     _p(cos_t), _p(sin_t))
    l8 = None
    if w8 is not None:
        l8 = (_lib.LlmLayerW8 * len(w["layers"]))()
        for i, q in enumerate(w8["layers"]):
            for n in ("qkv", "o", "gu", "d"):
                setattr(l8[i], "w" + n, _p(q["w" + n][0]))
                setattr(l8[i], "s" + n, _p(q["w" + n][1]))
        d.layers_w8 = l8
        d.lm_head_w8, d.lm_head_scale = _p(w8["lm_head"][0]), _p(w8["lm_head"][1])
    return d, (layers, w, kcache, vcache, l8, w8)


def _llm_ws(desc, S, device):
    n = int(_lib.load().vl2_llm_workspace_bytes(ctypes.byref(desc), S))
    if n < 0:
        raise _lib.Vl2HipError("vl2_llm_workspace_bytes: bad descriptor")
    return torch.empty((n,), dtype=torch.uint8, device=device), n


def llm_prefill(desc, x, logits_out, fp8=False):
    desc.flags = _CTL["stage_flags"] | (STAGE_PREFILL_FP8 if fp8 else 0)      # (before the size query: the fp8 activation image is carved only with the flag)
    ws, n = _llm_ws(desc, x.shape[0], x.device)
    _lib.call("vl2_llm_prefill", ctypes.byref(desc), _p(x), x.shape[0], _p(logits_out), _p(ws), n, _stream())
    return logits_out


def llm_decode_step(desc, logits, tok, state, hist, partial, ws, fp8=False):
    desc.flags = _CTL["stage_flags"] | (STAGE_DECODE_FP8 if fp8 else 0)
    _lib.call("vl2_llm_decode_step", ctypes.byref(desc), _p(logits), _p(tok), _p(state), _p(hist), _p(partial), _p(ws), ws.numel(), _stream())


# ------------------------------------------------------------------------------------------------ sparse MoE (Mixtral), csrc/k_moe.h
MOE_BM = 128           # row tile of the grouped GEMM: every expert's rows are padded to it


def moe_rows(S, k, E):
    """Rows of the permuted buffers for S tokens: the worst case S*k + E*(MOE_BM - 1), rounded up to the row tile (the counts stay on
    the device, so the buffers are sized without them)."""
    return (S * k + E * (MOE_BM - 1) + MOE_BM - 1) // MOE_BM * MOE_BM


def moe_route(x, wr, k, eps, xg=True, logits=False):
    """include/vl2hip.h vl2_moe_route: x [S, D], wr [E, D] fp32 (norm folded) -> dict of device tensors: ids / wts [S, k], counts [E],
    offs [E+1], gather [P], inv [S, k], and (xg=True) the permuted rows xg [P, D] with their row-norm table rn [P, 2]."""
    _chk(x, _lib.elem_dtype(), "x"); _chk(wr, torch.float32, "wr")
    S, D = x.shape
    E = wr.shape[0]
    P = moe_rows(S, k, E)
    dev = x.device
    i32 = dict(dtype=torch.int32, device=dev)
    r = dict(ids=torch.empty((S, k), **i32), wts=torch.empty((S, k), dtype=torch.float32, device=dev),
             rstd=torch.empty((S,), dtype=torch.float32, device=dev), counts=torch.empty((E,), **i32), offs=torch.empty((E + 1,), **i32),
             gather=torch.empty((P,), **i32), inv=torch.empty((S, k), **i32), P=P,
             logits=torch.empty((S, E), dtype=torch.float32, device=dev) if logits else None,
             xg=torch.empty((P, D), dtype=_lib.elem_dtype(), device=dev) if xg else None,
             rn=torch.empty((P, 2), dtype=torch.float32, device=dev) if xg else None)
    _lib.call("vl2_moe_route", _p(x), x.stride(0), _p(wr), S, D, E, k, float(eps), _p(r["ids"]), _p(r["wts"]), _p(r["rstd"]), _p(r["logits"]),
              _p(r["counts"]), _p(r["offs"]), _p(r["gather"]), _p(r["inv"]), P, _p(r["xg"]), _p(r["rn"]), _stream())
    return r


def moe_gemm(a, w, route, S, k, swiglu=False, row_norm=None, eps=0.0, out=None):
    """include/vl2hip.h vl2_moe_gemm: the grouped GEMM over the permuted rows a [P, K] (route = moe_route's dict), w [E, N, K] (SwiGLU:
    each expert packed like pack_gate_up) -> [P, N] (SwiGLU [P, N/2]); rows of padding are left unwritten."""
    _chk(a, _lib.elem_dtype(), "a"); _chk(w, _lib.elem_dtype(), "w"); _chk(row_norm, torch.float32, "row_norm")
    E, N, K = w.shape
    P = a.shape[0]
    if out is None:
        out = torch.empty((P, N // 2 if swiglu else N), dtype=_lib.elem_dtype(), device=a.device)
    _lib.call("vl2_moe_gemm", _p(a), a.stride(0), _p(w), w.stride(0), w.stride(1), _p(out), out.stride(0), _p(row_norm), float(eps),
              _p(route["counts"]), _p(route["offs"]), S, k, E, P, N, K, GEMM_SWIGLU if swiglu else 0, _stream())
    return out


def moe_combine(x1, y, route, eps, out=None, row_norm=None):
    """include/vl2hip.h vl2_moe_combine: x1 [S, D] + sum_j w_tj y[inv(t, j)] -> out (may be x1); row_norm [S, 2] gets (0, rstd)."""
    _chk(x1, _lib.elem_dtype(), "x1"); _chk(y, _lib.elem_dtype(), "y"); _chk(row_norm, torch.float32, "row_norm")
    S, D = x1.shape
    k = route["inv"].shape[1]
    out = torch.empty_like(x1) if out is None else out
    _lib.call("vl2_moe_combine", _p(x1), x1.stride(0), _p(y), y.stride(0), _p(route["inv"]), _p(route["wts"]), S, k, D, float(eps),
              _p(out), out.stride(0), _p(row_norm), _stream())
    return out


def moe_route_gemv(x, wr, ids, wts, eps, logits=None):
    """include/vl2hip.h vl2_moe_route_gemv: one token x [D] -> ids [k] int32, wts [k] fp32 (device buffers, written in place)."""
    _chk(x, _lib.elem_dtype(), "x"); _chk(wr, torch.float32, "wr"); _chk(wts, torch.float32, "wts"); _chk(logits, torch.float32, "logits")
    E, D = wr.shape
    _lib.call("vl2_moe_route_gemv", _p(x), _p(wr), D, E, ids.numel(), float(eps), _p(ids), _p(wts), _p(logits), _stream())


def moe_gemv(w, x, ids, wts=None, res=None, swiglu=False, eps=1e-5, out=None):
    """include/vl2hip.h vl2_moe_gemv over the experts in ids [k] (device): swiglu=True: x [D] -> [k, N/2] (RMSNorm with the folded weight);
    else x = [k, K] SwiGLU rows -> [N] = res + sum_j wts[j] * W_{ids[j]} x[j]."""
    _chk(w, _lib.elem_dtype(), "w"); _chk(x, _lib.elem_dtype(), "x"); _chk(res, _lib.elem_dtype(), "res"); _chk(wts, torch.float32, "wts")
    E, N, K = w.shape
    k = ids.numel()
    if out is None:
        out = torch.empty((k, N // 2) if swiglu else (N,), dtype=_lib.elem_dtype(), device=w.device)
    _lib.call("vl2_moe_gemv", _p(w), w.stride(0), w.stride(1), _p(x), _p(ids), _p(wts), _p(res), _p(out), E, k, N, K, float(eps),
              GEMM_SWIGLU if swiglu else 0, _stream())
    return out


# ------------------------------------------------------------------------------------------------ batched MoE decode, csrc/k_moe_skinny.h
def moe_route_rows(x, wr, k, eps, ids, wts, tables=None, logits=None):
    """include/vl2hip.h vl2_moe_route_rows: route the rows x [S, D] into ids / wts [S, k] (device buffers, written in place) and, with
    tables = dict(counts [E], offs [E+1], gather [S*k], inv [S, k]), the compact tables of the grouped skinny GEMM (row tile 1: no padding)."""
    _chk(x, _lib.elem_dtype(), "x"); _chk(wr, torch.float32, "wr"); _chk(wts, torch.float32, "wts"); _chk(logits, torch.float32, "logits")
    S, D = x.shape
    E = wr.shape[0]
    t = tables or {}
    for name, n in (("ids", S * k), ("wts", S * k)) + ((("counts", E), ("offs", E + 1), ("gather", S * k), ("inv", S * k)) if tables else ()):
        buf = {**t, "ids": ids, "wts": wts}[name]
        if buf.numel() < n or not buf.is_contiguous():
            raise ValueError(f"moe_route_rows: {name} needs {n} contiguous elements, got {tuple(buf.shape)}")
    _lib.call("vl2_moe_route_rows", _p(x), x.stride(0), _p(wr), S, D, E, k, float(eps), _p(ids), _p(wts), _p(logits), _p(t.get("counts")),
              _p(t.get("offs")), _p(t.get("gather")), _p(t.get("inv")), _stream())


def moe_skinny_part_bytes(S, k, N, K):
    """Bytes of fp32 partial sums moe_gemm_skinny needs for S tokens: ks * S*k * N * 4, ks = the skinny-M K split of (N, K)."""
    n = int(_lib.load().vl2_moe_gemm_skinny_part_bytes(S, k, N, K))
    if n < 0:
        raise ValueError(f"moe_gemm_skinny: shape not built (S={S} k={k} N={N} K={K}: S <= 64, N % 64 == 0, K % 32 == 0)")
    return n


def moe_gemm_skinny(a, w, tables, S, k, part, rowmap=None, swiglu=False, out=None):
    """include/vl2hip.h vl2_moe_gemm_skinny: the grouped skinny-M GEMM of S <= 64 tokens over the S*k permuted rows of the compact tables
    (moe_route_rows).  a: the permuted rows [S*k, K], or with rowmap [S*k] (permuted row -> row of a) the token rows [S, K]; w [E, N, K]
    (swiglu: each expert packed like pack_gate_up) -> [S*k, N] (swiglu [S*k, N/2]).  part: fp32 buffer of moe_skinny_part_bytes(S, k, N, K)."""
    _chk(a, _lib.elem_dtype(), "a"); _chk(w, _lib.elem_dtype(), "w"); _chk(part, torch.float32, "part")
    E, N, K = w.shape
    R = S * k
    if out is None:
        out = torch.empty((R, N // 2 if swiglu else N), dtype=_lib.elem_dtype(), device=a.device)
    if out.shape[0] < R or (rowmap is not None and rowmap.numel() < R) or tables["counts"].numel() < E or tables["offs"].numel() < E + 1:
        raise ValueError("moe_gemm_skinny: out / rowmap / tables are too short for S * k rows and E experts")
    _lib.call("vl2_moe_gemm_skinny", _p(a), a.stride(0), a.shape[0], _p(rowmap), _p(w), w.stride(0), w.stride(1), _p(out), out.stride(0),
              _p(tables["counts"]), _p(tables["offs"]), S, k, E, N, K, GEMM_SWIGLU if swiglu else 0, _p(part), part.numel() * 4, _stream())
    return out


def moe_gemv_batched(w, x, ids, wts=None, res=None, swiglu=False, eps=1e-5, out=None):
    """include/vl2hip.h vl2_moe_gemv_batched: moe_gemv for the S tokens of ids [S, k] in one launch.  swiglu=True: x [S, D] -> [S*k, N/2];
    else x = the SwiGLU rows [S*k, K] -> [S, N] = res + sum_j wts[t, j] * W_{ids[t, j]} x[t*k + j].  A token's rows are moe_gemv's bits."""
    _chk(w, _lib.elem_dtype(), "w"); _chk(x, _lib.elem_dtype(), "x"); _chk(res, _lib.elem_dtype(), "res"); _chk(wts, torch.float32, "wts")
    E, N, K = w.shape
    S, k = ids.shape
    if x.shape[0] < (S if swiglu else S * k) or (res is not None and res.shape[0] < S) or (wts is not None and wts.numel() < S * k):
        raise ValueError("moe_gemv_batched: x / res / wts are too short for the S tokens of ids")
    if out is None:
        out = torch.empty((S * k, N // 2) if swiglu else (S, N), dtype=_lib.elem_dtype(), device=w.device)
    if out.shape[0] < (S * k if swiglu else S):
        raise ValueError("moe_gemv_batched: out is too short for the S tokens of ids")
    _lib.call("vl2_moe_gemv_batched", _p(w), w.stride(0), w.stride(1), _p(x), x.stride(0), _p(ids), _p(wts), _p(res),
              0 if res is None else res.stride(0), _p(out), out.stride(0), S, E, k, N, K, float(eps), GEMM_SWIGLU if swiglu else 0, _stream())
    return out


# ------------------------------------------------------------------------------------------------ fp8 expert weights of the MoE decode, csrc/k_moe_fp8.h
def moe_quant_fp8(w):
    """An expert stack w [E, N, K] (contiguous, 16-bit) -> (q uint8 [E, N, K] e4m3fn bytes, scale fp32 [E, N]: one power-of-two scale per expert
    and output row): ONE vl2_pack_quant_fp8 call on the [E * N, K] view, so expert e is `quant_fp8(w[e])` bit for bit."""
    _chk(w, _lib.elem_dtype(), "w")
    E, N, K = w.shape
    if not w.is_contiguous():
        raise ValueError("moe_quant_fp8: the expert stack must be contiguous (it is quantised as its [E * N, K] view)")
    q, sc = quant_fp8(w.view(E * N, K))
    return q.view(E, N, K), sc.view(E, N)


def _chk_moe8(who, q, scale):
    _chk(q, torch.uint8, "q"); _chk(scale, torch.float32, "scale")
    if q.dim() != 3 or scale.dim() != 2 or tuple(scale.shape) != tuple(q.shape[:2]) or q.stride(2) != 1 or scale.stride(1) != 1:
        raise ValueError(f"{who}: need q [E, N, K] bytes and scale [E, N] (moe_quant_fp8), got {tuple(q.shape)} and {tuple(scale.shape)}")
    return q.shape


def moe_gemv_fp8(q, scale, x, ids, wts=None, res=None, swiglu=False, eps=1e-5, out=None):
    """include/vl2hip.h vl2_moe_gemv_fp8: `moe_gemv` on the fp8 expert stack (q, scale) of `moe_quant_fp8`.  swiglu=True: slot j is bit for bit
    gemv_fp8(q[ids[j]], scale[ids[j]], x, swiglu=True, rms_plain=True); else out = res + sum_j wts[j] * gemv_fp8(.., x[j], out_f32=True) as an fma
    chain in slot order, rounded once."""
    E, N, K = _chk_moe8("moe_gemv_fp8", q, scale)
    _chk(x, _lib.elem_dtype(), "x"); _chk(res, _lib.elem_dtype(), "res"); _chk(wts, torch.float32, "wts")
    k = ids.numel()
    if out is None:
        out = torch.empty((k, N // 2) if swiglu else (N,), dtype=_lib.elem_dtype(), device=q.device)
    _lib.call("vl2_moe_gemv_fp8", _p(q), q.stride(0), q.stride(1), _p(scale), scale.stride(0), _p(x), _p(ids), _p(wts), _p(res), _p(out), E, k, N, K,
              float(eps), GEMM_SWIGLU if swiglu else 0, _stream())
    return out


def moe_gemv_batched_fp8(q, scale, x, ids, wts=None, res=None, swiglu=False, eps=1e-5, out=None):
    """include/vl2hip.h vl2_moe_gemv_batched_fp8: `moe_gemv_fp8` for the S tokens of ids [S, k] in one launch; a token's rows are its bits."""
    E, N, K = _chk_moe8("moe_gemv_batched_fp8", q, scale)
    _chk(x, _lib.elem_dtype(), "x"); _chk(res, _lib.elem_dtype(), "res"); _chk(wts, torch.float32, "wts")
    S, k = ids.shape
    if x.shape[0] < (S if swiglu else S * k) or (res is not None and res.shape[0] < S) or (wts is not None and wts.numel() < S * k):
        raise ValueError("moe_gemv_batched_fp8: x / res / wts are too short for the S tokens of ids")
    if out is None:
        out = torch.empty((S * k, N // 2) if swiglu else (S, N), dtype=_lib.elem_dtype(), device=q.device)
    if out.shape[0] < (S * k if swiglu else S):
        raise ValueError("moe_gemv_batched_fp8: out is too short for the S tokens of ids")
    _lib.call("vl2_moe_gemv_batched_fp8", _p(q), q.stride(0), q.stride(1), _p(scale), scale.stride(0), _p(x), x.stride(0), _p(ids), _p(wts), _p(res),
              0 if res is None else res.stride(0), _p(out), out.stride(0), S, E, k, N, K, float(eps), GEMM_SWIGLU if swiglu else 0, _stream())
    return out


def moe_gemm_skinny_fp8(a, q, scale, tables, S, k, part, rowmap=None, swiglu=False, out=None):
    """include/vl2hip.h vl2_moe_gemm_skinny_fp8: `moe_gemm_skinny` on the fp8 expert stack (q, scale): a permuted row is bit for bit
    `gemm_skinny_fp8` on that one row with its expert's bytes and scales.  part: fp32 buffer of moe_skinny_part_bytes(S, k, N, K)."""
    E, N, K = _chk_moe8("moe_gemm_skinny_fp8", q, scale)
    _chk(a, _lib.elem_dtype(), "a"); _chk(part, torch.float32, "part")
    R = S * k
    if out is None:
        out = torch.empty((R, N // 2 if swiglu else N), dtype=_lib.elem_dtype(), device=a.device)
    if out.shape[0] < R or (rowmap is not None and rowmap.numel() < R) or tables["counts"].numel() < E or tables["offs"].numel() < E + 1:
        raise ValueError("moe_gemm_skinny_fp8: out / rowmap / tables are too short for S * k rows and E experts")
    _lib.call("vl2_moe_gemm_skinny_fp8", _p(a), a.stride(0), a.shape[0], _p(rowmap), _p(q), q.stride(0), q.stride(1), _p(scale), scale.stride(0),
              _p(out), out.stride(0), _p(tables["counts"]), _p(tables["offs"]), S, k, E, N, K, GEMM_SWIGLU if swiglu else 0, _p(part),
              part.numel() * 4, _stream())
    return out


# ------------------------------------------------------------------------------------------------ tiled W8A16 grouped GEMM, csrc/k_moe_gemm8.h
def moe_gemm_fp8(a, q, scale, route, S, k, swiglu=False, row_norm=None, eps=0.0, out=None):
    """include/vl2hip.h vl2_moe_gemm_fp8: `moe_gemm` on the fp8 expert stack (q, scale) of `moe_quant_fp8`, any number of tokens: the grouped
    GEMM over the permuted rows a [P, K] (route = moe_route's dict) -> [P, N] (swiglu [P, N/2]); rows of padding are left unwritten.  A row is
    bit for bit `moe_gemm` on the dequantised stack q * scale."""
    E, N, K = _chk_moe8("moe_gemm_fp8", q, scale)
    _chk(a, _lib.elem_dtype(), "a"); _chk(row_norm, torch.float32, "row_norm")
    P = a.shape[0]
    if out is None:
        out = torch.empty((P, N // 2 if swiglu else N), dtype=_lib.elem_dtype(), device=a.device)
    _lib.call("vl2_moe_gemm_fp8", _p(a), a.stride(0), _p(q), q.stride(0), q.stride(1), _p(scale), scale.stride(0), _p(out), out.stride(0),
              _p(row_norm), float(eps), _p(route["counts"]), _p(route["offs"]), S, k, E, P, N, K, GEMM_SWIGLU if swiglu else 0, _stream())
    return out


# ------------------------------------------------------------------------------------------------ MXFP4 expert weights of the MoE decode, csrc/k_moe_mxfp4.h
def moe_quant_mxfp4(w):
    """An expert stack w [E, N, K] (contiguous, 16-bit, K % 32 == 0) -> (q uint8 [E, N, K / 2]: two E2M1 codes per byte, k = 2j in bits 3:0;
    s uint8 [E, N, K / 32]: one E8M0 scale per block of 32): ONE vl2_pack_quant_mxfp4 call on the [E * N, K] view, so expert e is
    `quant_mxfp4(w[e])` bit for bit."""
    _chk(w, _lib.elem_dtype(), "w")
    E, N, K = w.shape
    if not w.is_contiguous():
        raise ValueError("moe_quant_mxfp4: the expert stack must be contiguous (it is quantised as its [E * N, K] view)")
    q, s = quant_mxfp4(w.view(E * N, K))
    return q.view(E, N, K // 2), s.view(E, N, K // 32)


def _chk_moe4(who, q, s):
    _chk(q, torch.uint8, "q"); _chk(s, torch.uint8, "s")
    if q.dim() != 3 or s.dim() != 3 or tuple(s.shape[:2]) != tuple(q.shape[:2]) or s.shape[2] * 16 != q.shape[2] or q.stride(2) != 1 or s.stride(2) != 1:
        raise ValueError(f"{who}: need q [E, N, K / 2] bytes and s [E, N, K / 32] bytes (moe_quant_mxfp4), got {tuple(q.shape)} and {tuple(s.shape)}")
    return q.shape[0], q.shape[1], q.shape[2] * 2


def moe_gemv_mxfp4(q, s, x, ids, wts=None, res=None, swiglu=False, eps=1e-5, out=None):
    """include/vl2hip.h vl2_moe_gemv_mxfp4: `moe_gemv` on the MXFP4 expert stack (q, s) of `moe_quant_mxfp4` (strided views are taken as they
    are).  swiglu=True: slot j is bit for bit gemv_mxfp4(q[ids[j]], s[ids[j]], x, swiglu=True, rms_plain=True); else out = res + sum_j wts[j] *
    gemv_mxfp4(.., x[j], out_f32=True) as an fma chain in slot order, rounded once."""
    E, N, K = _chk_moe4("moe_gemv_mxfp4", q, s)
    _chk(x, _lib.elem_dtype(), "x"); _chk(res, _lib.elem_dtype(), "res"); _chk(wts, torch.float32, "wts")
    k = ids.numel()
    if out is None:
        out = torch.empty((k, N // 2) if swiglu else (N,), dtype=_lib.elem_dtype(), device=q.device)
    _lib.call("vl2_moe_gemv_mxfp4", _p(q), q.stride(0), q.stride(1), _p(s), s.stride(0), s.stride(1), _p(x), _p(ids), _p(wts), _p(res), _p(out), E, k,
              N, K, float(eps), GEMM_SWIGLU if swiglu else 0, _stream())
    return out


def moe_gemv_batched_mxfp4(q, s, x, ids, wts=None, res=None, swiglu=False, eps=1e-5, out=None):
    """include/vl2hip.h vl2_moe_gemv_batched_mxfp4: `moe_gemv_mxfp4` for the S tokens of ids [S, k] in one launch; a token's rows are its bits."""
    E, N, K = _chk_moe4("moe_gemv_batched_mxfp4", q, s)
    _chk(x, _lib.elem_dtype(), "x"); _chk(res, _lib.elem_dtype(), "res"); _chk(wts, torch.float32, "wts")
    S, k = ids.shape
    if x.shape[0] < (S if swiglu else S * k) or (res is not None and res.shape[0] < S) or (wts is not None and wts.numel() < S * k):
        raise ValueError("moe_gemv_batched_mxfp4: x / res / wts are too short for the S tokens of ids")
    if out is None:
        out = torch.empty((S * k, N // 2) if swiglu else (S, N), dtype=_lib.elem_dtype(), device=q.device)
    if out.shape[0] < (S * k if swiglu else S):
        raise ValueError("moe_gemv_batched_mxfp4: out is too short for the S tokens of ids")
    _lib.call("vl2_moe_gemv_batched_mxfp4", _p(q), q.stride(0), q.stride(1), _p(s), s.stride(0), s.stride(1), _p(x), x.stride(0), _p(ids), _p(wts),
              _p(res), 0 if res is None else res.stride(0), _p(out), out.stride(0), S, E, k, N, K, float(eps), GEMM_SWIGLU if swiglu else 0, _stream())
    return out


def moe_gemm_skinny_mxfp4(a, q, s, tables, S, k, part, rowmap=None, swiglu=False, out=None):
    """include/vl2hip.h vl2_moe_gemm_skinny_mxfp4: `moe_gemm_skinny` on the MXFP4 expert stack (q, s): a permuted row is bit for bit
    `gemm_skinny_mxfp4` on that one row with its expert's bytes and scales.  part: fp32 buffer of moe_skinny_part_bytes(S, k, N, K)."""
    E, N, K = _chk_moe4("moe_gemm_skinny_mxfp4", q, s)
    _chk(a, _lib.elem_dtype(), "a"); _chk(part, torch.float32, "part")
    R = S * k
    if out is None:
        out = torch.empty((R, N // 2 if swiglu else N), dtype=_lib.elem_dtype(), device=a.device)
    if out.shape[0] < R or (rowmap is not None and rowmap.numel() < R) or tables["counts"].numel() < E or tables["offs"].numel() < E + 1:
        raise ValueError("moe_gemm_skinny_mxfp4: out / rowmap / tables are too short for S * k rows and E experts")
    _lib.call("vl2_moe_gemm_skinny_mxfp4", _p(a), a.stride(0), a.shape[0], _p(rowmap), _p(q), q.stride(0), q.stride(1), _p(s), s.stride(0), s.stride(1),
              _p(out), out.stride(0), _p(tables["counts"]), _p(tables["offs"]), S, k, E, N, K, GEMM_SWIGLU if swiglu else 0, _p(part),
              part.numel() * 4, _stream())
    return out


# ------------------------------------------------------------------------------------------------ tiled W4A16 grouped GEMM, csrc/k_moe_gemm4.h
def moe_gemm_mxfp4(a, q, s, route, S, k, swiglu=False, row_norm=None, eps=0.0, out=None):
    """include/vl2hip.h vl2_moe_gemm_mxfp4: `moe_gemm` on the MXFP4 expert stack (q, s) of `moe_quant_mxfp4` (strided views are taken as they
    are), any number of tokens: the grouped GEMM over the permuted rows a [P, K] (route = moe_route's dict) -> [P, N] (swiglu [P, N/2]); rows
    of padding are left unwritten.  A row is bit for bit `moe_gemm` on the dequantised stack 2^e * E2M1(q)."""
    E, N, K = _chk_moe4("moe_gemm_mxfp4", q, s)
    _chk(a, _lib.elem_dtype(), "a"); _chk(row_norm, torch.float32, "row_norm")
    P = a.shape[0]
    if out is None:
        out = torch.empty((P, N // 2 if swiglu else N), dtype=_lib.elem_dtype(), device=a.device)
    _lib.call("vl2_moe_gemm_mxfp4", _p(a), a.stride(0), _p(q), q.stride(0), q.stride(1), _p(s), s.stride(0), s.stride(1), _p(out), out.stride(0),
              _p(row_norm), float(eps), _p(route["counts"]), _p(route["offs"]), S, k, E, P, N, K, GEMM_SWIGLU if swiglu else 0, _stream())
    return out
