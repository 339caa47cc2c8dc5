"""Thin typed wrappers: torch CUDA tensors in, C-ABI kernel launches out (on torch's current
stream).  torch is used here for device memory and streams only — every arithmetic step is a
libmoviigen_hip.so kernel; a failure raises, nothing falls back to torch math."""
import ctypes

import torch

from . import lib

BIAS_BF16, BIAS_GELU_BF16, GATE_RESID_F32, BIAS_F32 = 0, 1, 2, 3


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _epilogue_dtype(epilogue):
    """what a GEMM epilogue writes (MG_EPI_* in include/moviigen_hip.h): bf16 behind bias / bias+GELU, fp32 otherwise"""
    return torch.bfloat16 if epilogue in (BIAS_BF16, BIAS_GELU_BF16) else torch.float32


def _chk(t, dtype, name):
    if t is None:
        return
    if not t.is_cuda:
        raise lib.MoviigenHipError(f'{name}: expected a CUDA (HIP) tensor — the hot path has no CPU fallback')
    if t.dtype != dtype:
        raise lib.MoviigenHipError(f'{name}: expected {dtype}, got {t.dtype}')
    if t.dim() >= 1 and t.stride(-1) != 1:
        raise lib.MoviigenHipError(f'{name}: innermost dimension must be contiguous')


def _chk_flat(t, dtype, name, optional=False):
    """a tensor its kernel reads or writes flat, or with a row stride the C ABI does not carry: _chk, and dense row-major"""
    if t is None and not optional:
        raise lib.MoviigenHipError(f'{name}: expected a tensor, got None')
    _chk(t, dtype, name)
    if t is not None and not t.is_contiguous():
        raise lib.MoviigenHipError(f'{name}: must be contiguous, got shape {tuple(t.shape)} with strides {tuple(t.stride())}')


def _chk_rows(t, dtype, name):
    """a [rows, cols] tensor whose row stride goes to the kernel: _chk, two dimensions, rows that do not overlap"""
    if t is None:
        raise lib.MoviigenHipError(f'{name}: expected a tensor, got None')
    _chk(t, dtype, name)
    if t.dim() != 2 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise lib.MoviigenHipError(f'{name}: expected [rows, cols] with a row stride >= cols, got shape {tuple(t.shape)} with strides {tuple(t.stride())}')


def ln_modulate(x, scale, shift, add_one, eps, out, round_norm_bf16=False):
    """x [rows, dim] fp32 -> out [rows, dim] (bf16 or fp32)."""
    _chk(x, torch.float32, 'x'); _chk(scale, torch.float32, 'scale'); _chk(shift, torch.float32, 'shift')
    rows, dim = x.shape
    lib.call('mg_ln_modulate', _p(x), x.stride(0), rows, dim, _p(scale), _p(shift), int(add_one), float(eps),
             int(round_norm_bf16), _p(out), int(out.dtype == torch.float32), out.stride(0), _st())
    return out


def resid_ln_modulate(x, r, scale, shift, eps, out):
    """out [rows, dim] fp32 = LN(x + r) * (1 + scale) + shift, x and r [rows, dim] fp32 (row strides free), only read: the bits of
    ln_modulate(lincomb(x, r), scale, shift, True, eps, out) in one pass (the step cache's skipped step)."""
    _chk(x, torch.float32, 'x'); _chk(r, torch.float32, 'r'); _chk(scale, torch.float32, 'scale'); _chk(shift, torch.float32, 'shift')
    _chk(out, torch.float32, 'out')
    if x.dim() != 2 or tuple(r.shape) != tuple(x.shape) or tuple(out.shape) != tuple(x.shape):
        raise lib.MoviigenHipError(f'resid_ln_modulate shape mismatch x{tuple(x.shape)} r{tuple(r.shape)} out{tuple(out.shape)}')
    rows, dim = x.shape
    for name, t in (('scale', scale), ('shift', shift)):
        if t is not None and t.numel() != dim:
            raise lib.MoviigenHipError(f'resid_ln_modulate: {name} must have {dim} elements, got {t.numel()}')
    lib.call('mg_resid_ln_modulate_f32', _p(x), x.stride(0), _p(r), r.stride(0), rows, dim, _p(scale), _p(shift), float(eps), _p(out),
             out.stride(0), _st())
    return out


def step_resid_partials(device):
    """the caller-owned scratch of step_resid_capture(stats=...): mg_step_resid_partials_bytes() bytes as fp64, no initial value needed"""
    return torch.empty(int(lib.load().mg_step_resid_partials_bytes()) // 8, dtype=torch.float64, device=device)


def step_resid_capture(r, x, xin, stats=None, partials=None):
    """r <- x - xin (contiguous fp32 tensors of equal size, r IN PLACE).  stats: fp64 [2] receiving (sum |r_new - r_old|, sum |r_old|),
    r_old = what r held — deterministic (fixed grid, fixed order); it needs `partials` (step_resid_partials).  None: no reduction."""
    for name, t in (('r', r), ('x', x), ('xin', xin)):
        _chk(t, torch.float32, name)
        if t is None or not t.is_contiguous():
            raise lib.MoviigenHipError(f'{name} must be a contiguous fp32 tensor')
    if x.numel() != r.numel() or xin.numel() != r.numel():
        raise lib.MoviigenHipError(f'step_resid_capture size mismatch r{tuple(r.shape)} x{tuple(x.shape)} xin{tuple(xin.shape)}')
    if stats is not None:
        _chk(stats, torch.float64, 'stats'); _chk(partials, torch.float64, 'partials')
        if stats.numel() < 2 or not stats.is_contiguous() or partials is None or not partials.is_contiguous() \
                or partials.numel() * 8 < int(lib.load().mg_step_resid_partials_bytes()):
            raise lib.MoviigenHipError('step_resid_capture: stats must be fp64 [2] and partials step_resid_partials(device)')
    lib.call('mg_step_resid_capture_f32', _p(r), _p(x), _p(xin), r.numel(), _p(stats), _p(partials) if stats is not None else None, _st())
    return r


ATTN_LOG2E = 1.4426950408889634


def rmsnorm_rope(x, weight, eps, head_dim, out, rope_cs=None, grid=(1, 1, 1), pos0=0, out_scale=1.0):
    """x [rows, dim] bf16 (may be a strided column slice) -> out bf16.  out_scale: factor applied before the one
    rounding to bf16 (the attention's scale*log2(e) for a q that goes to attention_hd128(..., prescaled=True))."""
    _chk(x, torch.bfloat16, 'x'); _chk(out, torch.bfloat16, 'out'); _chk(weight, torch.float32, 'weight')
    rows, dim = x.shape
    lib.call('mg_rmsnorm_rope_bf16', _p(x), x.stride(0), _p(out), out.stride(0), rows, dim, _p(weight), float(eps),
             int(head_dim), _p(rope_cs), int(grid[0]), int(grid[1]), int(grid[2]), int(pos0), float(out_scale), _st())
    return out


def packed_kv_numel(L, heads):
    """elements of one packed K (or V) buffer for L keys: heads * ceil(L/64) tiles of 8192."""
    return heads * ((L + 63) // 64) * 8192


def pack_kv(k, v, heads, kp, vp):
    """k, v [L, heads*128] bf16 (strided column slices ok; either may be None) -> packed 64-key tiles
    kp / vp (flat bf16 buffers of packed_kv_numel elements) for attention_hd128."""
    _chk(k, torch.bfloat16, 'k'); _chk(v, torch.bfloat16, 'v'); _chk(kp, torch.bfloat16, 'kp'); _chk(vp, torch.bfloat16, 'vp')
    ref = k if k is not None else v
    L = ref.shape[0]
    for name, buf in (('kp', kp if k is not None else None), ('vp', vp if v is not None else None)):
        if buf is not None and buf.numel() < packed_kv_numel(L, heads):
            raise lib.MoviigenHipError(f'{name} too small for {L} keys x {heads} heads')
    lib.call('mg_pack_kv_bf16', _p(k), 0 if k is None else k.stride(0), _p(v), 0 if v is None else v.stride(0), L,
             int(heads), 128, _p(kp), _p(vp), _st())


def gemm(a, w, bias, epilogue, out, gate=None):
    """out[M,N] (+)= a[M,K] @ w[N,K]^T (+bias ...) — see MG_EPI_* in include/moviigen_hip.h."""
    _chk(a, torch.bfloat16, 'a'); _chk(w, torch.bfloat16, 'w'); _chk(bias, torch.float32, 'bias')
    _chk(gate, torch.float32, 'gate')
    _chk(out, _epilogue_dtype(epilogue), 'out')
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K or out.shape[0] != M or out.shape[1] != N:
        raise lib.MoviigenHipError(f'gemm shape mismatch a{tuple(a.shape)} w{tuple(w.shape)} out{tuple(out.shape)}')
    lib.call('mg_gemm_bf16', _p(a), a.stride(0), _p(w), w.stride(0), _p(bias), M, N, K, int(epilogue), _p(out),
             out.stride(0), _p(gate), _st())
    return out


def quant_mxfp8(x, q=None, scales=None):
    """x [rows, K] bf16 (row stride free) -> (q uint8 [rows, K] e4m3fn bytes, scales uint8 [rows, K/32] E8M0 bytes): OCP MXFP8
    with the project's saturating definition (include/moviigen_hip.h).  q / scales are allocated when not given."""
    _chk(x, torch.bfloat16, 'x')
    if x.dim() != 2:
        raise lib.MoviigenHipError(f'quant_mxfp8: expected [rows, K], got {tuple(x.shape)}')
    rows, K = x.shape
    if q is None:
        q = torch.empty(rows, K, dtype=torch.uint8, device=x.device)
    if scales is None:
        scales = torch.empty(rows, K // 32, dtype=torch.uint8, device=x.device)
    _chk(q, torch.uint8, 'q'); _chk(scales, torch.uint8, 'scales')
    if tuple(q.shape) != (rows, K) or tuple(scales.shape) != (rows, K // 32):
        raise lib.MoviigenHipError(f'quant_mxfp8 shape mismatch x{tuple(x.shape)} q{tuple(q.shape)} scales{tuple(scales.shape)}')
    lib.call('mg_quant_mxfp8_rows', _p(x), x.stride(0), rows, K, _p(q), q.stride(0), _p(scales), scales.stride(0), _st())
    return q, scales


def gemm_mxfp8(aq, a_scales, wq, w_scales, bias, epilogue, out, gate=None):
    """out[M,N] (+)= dequant(aq, a_scales)[M,K] @ dequant(wq, w_scales)[N,K]^T (+bias ...) on the block-scaled MFMA; the epilogues
    of `gemm` (MG_EPI_* in include/moviigen_hip.h)."""
    _chk(aq, torch.uint8, 'aq'); _chk(a_scales, torch.uint8, 'a_scales'); _chk(wq, torch.uint8, 'wq')
    _chk(w_scales, torch.uint8, 'w_scales'); _chk(bias, torch.float32, 'bias'); _chk(gate, torch.float32, 'gate')
    _chk(out, _epilogue_dtype(epilogue), 'out')
    M, K = aq.shape
    N = wq.shape[0]
    if (wq.shape[1] != K or out.shape[0] != M or out.shape[1] != N or tuple(a_scales.shape) != (M, K // 32)
            or tuple(w_scales.shape) != (N, K // 32)):
        raise lib.MoviigenHipError(f'gemm_mxfp8 shape mismatch aq{tuple(aq.shape)} a_scales{tuple(a_scales.shape)} '
                                   f'wq{tuple(wq.shape)} w_scales{tuple(w_scales.shape)} out{tuple(out.shape)}')
    lib.call('mg_gemm_mxfp8', _p(aq), aq.stride(0), _p(a_scales), a_scales.stride(0), _p(wq), wq.stride(0), _p(w_scales),
             w_scales.stride(0), _p(bias), M, N, K, int(epilogue), _p(out), out.stride(0), _p(gate), _st())
    return out


def ln_modulate_mxfp8(x, scale, shift, add_one, eps, q, scales, out=None, round_norm_bf16=False):
    """ln_modulate (bf16 result) leaving as MXFP8: x [rows, dim] fp32 -> q uint8 [rows, dim] + scales uint8 [rows, dim/32], the bytes
    quant_mxfp8 makes of ln_modulate's bf16 output; `out` (bf16 [rows, dim]) receives that output as well when given."""
    _chk(x, torch.float32, 'x'); _chk(scale, torch.float32, 'scale'); _chk(shift, torch.float32, 'shift')
    _chk(q, torch.uint8, 'q'); _chk(scales, torch.uint8, 'scales'); _chk(out, torch.bfloat16, 'out')
    rows, dim = x.shape
    if tuple(q.shape) != (rows, dim) or tuple(scales.shape) != (rows, dim // 32) or (out is not None and tuple(out.shape) != (rows, dim)):
        raise lib.MoviigenHipError(f'ln_modulate_mxfp8 shape mismatch x{tuple(x.shape)} q{tuple(q.shape)} scales{tuple(scales.shape)}')
    lib.call('mg_ln_modulate_mxfp8', _p(x), x.stride(0), rows, dim, _p(scale), _p(shift), int(add_one), float(eps),
             int(round_norm_bf16), _p(out), 0 if out is None else out.stride(0), _p(q), q.stride(0), _p(scales), scales.stride(0), _st())
    return q, scales


def gemm_mxfp8_gelu_q(aq, a_scales, wq, w_scales, bias, oq, o_scales):
    """gemm_mxfp8 with the BIAS_GELU_BF16 epilogue whose bf16 result leaves as MXFP8: oq uint8 [M, N] + o_scales uint8 [M, N/32], the
    bytes quant_mxfp8 makes of that epilogue's output."""
    _chk(aq, torch.uint8, 'aq'); _chk(a_scales, torch.uint8, 'a_scales'); _chk(wq, torch.uint8, 'wq')
    _chk(w_scales, torch.uint8, 'w_scales'); _chk(bias, torch.float32, 'bias'); _chk(oq, torch.uint8, 'oq')
    _chk(o_scales, torch.uint8, 'o_scales')
    M, K = aq.shape
    N = wq.shape[0]
    if (wq.shape[1] != K or tuple(oq.shape) != (M, N) or tuple(o_scales.shape) != (M, N // 32)
            or tuple(a_scales.shape) != (M, K // 32) or tuple(w_scales.shape) != (N, K // 32)):
        raise lib.MoviigenHipError(f'gemm_mxfp8_gelu_q shape mismatch aq{tuple(aq.shape)} a_scales{tuple(a_scales.shape)} '
                                   f'wq{tuple(wq.shape)} w_scales{tuple(w_scales.shape)} oq{tuple(oq.shape)} o_scales{tuple(o_scales.shape)}')
    lib.call('mg_gemm_mxfp8_gelu_q', _p(aq), aq.stride(0), _p(a_scales), a_scales.stride(0), _p(wq), wq.stride(0), _p(w_scales),
             w_scales.stride(0), _p(bias), M, N, K, _p(oq), oq.stride(0), _p(o_scales), o_scales.stride(0), _st())
    return oq, o_scales


_ATTN_WS = {}


def attention_workspace(device=None, stream=None):
    """The caller-owned workspace of mg_attn_fwd_bf16_hd128* for launches on `stream` of `device` (default: the current ones):
    mg_attn_workspace_bytes() zeroed bytes, allocated once per (device, stream) HERE — outside the library, which never
    allocates — and shared by that stream's launches (they are ordered; each leaves it zeroed)."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    st = torch.cuda.current_stream(dev) if stream is None else stream
    key = (dev, st.cuda_stream)
    ws = _ATTN_WS.get(key)
    if ws is None:
        with torch.cuda.stream(st):
            ws = torch.zeros(int(lib.load().mg_attn_workspace_bytes()), dtype=torch.uint8, device=f'cuda:{dev}')
        _ATTN_WS[key] = ws
    return ws


def attention_item_queries(lq, lk, heads, prescaled=True, n_cu=256):
    """queries per work item (256 or 320) of the attention_hd128 launch for this shape on a persistent grid of n_cu workgroups: the library's
    own rule (mg_attn_hd128_item_queries, a host function — no GPU needed).  A launch has heads * ceil(lq / item) items."""
    return int(lib.load().mg_attn_hd128_item_queries(int(lq), int(lk), int(heads), int(bool(prescaled)), int(n_cu)))


def attention_hd128(q, kp, vp, out, lk, heads, scale, prescaled=False, reserve_cus=0, workspace='stream', lse=None):
    """q [Lq, >=heads*128] bf16; kp/vp from pack_kv for the same lk keys; out [Lq, >=heads*128].
    prescaled: q was produced with rmsnorm_rope(out_scale=scale * ATTN_LOG2E) — `scale` is then only documentation.
    reserve_cus (prescaled entry): CUs the persistent grid leaves free for a kernel on another stream (the exchange).
    workspace: 'stream' = attention_workspace() of the current stream; a uint8 tensor of the caller's; None = no tickets.
    lse: fp32 [heads, Lq] that also receives the log-sum-exp of the scaled scores (ring attention), or None."""
    _chk(q, torch.bfloat16, 'q'); _chk(kp, torch.bfloat16, 'kp'); _chk(vp, torch.bfloat16, 'vp')
    _chk(out, torch.bfloat16, 'out'); _chk(lse, torch.float32, 'lse')
    if min(kp.numel(), vp.numel()) < packed_kv_numel(int(lk), int(heads)):
        raise lib.MoviigenHipError('packed K/V buffers too small for lk keys')
    if lse is not None and (lse.numel() < int(heads) * q.shape[0] or not lse.is_contiguous()):
        raise lib.MoviigenHipError('lse must be a contiguous [heads, Lq] fp32 tensor')
    ws = attention_workspace(q.device) if isinstance(workspace, str) else workspace
    head = (_p(q), q.stride(0), _p(kp), _p(vp), _p(out), out.stride(0))
    if prescaled:
        lib.call('mg_attn_fwd_bf16_hd128_prescaled', *head, _p(lse), q.shape[0], int(lk), int(heads), int(reserve_cus), _p(ws), _st())
    elif lse is not None:
        lib.call('mg_attn_fwd_bf16_hd128_lse', *head, _p(lse), q.shape[0], int(lk), int(heads), float(scale), _p(ws), _st())
    else:
        lib.call('mg_attn_fwd_bf16_hd128', *head, q.shape[0], int(lk), int(heads), float(scale), _p(ws), _st())
    return out


_attention_hd128 = attention_hd128      # the engine's own function, whatever a caller binds to the public name (bench.py times that one)


def attention_hd128_lse(q, kp, vp, out, lse, lk, heads, scale, prescaled=False):
    """attention_hd128(..., lse=lse) -> (out, lse)"""
    return _attention_hd128(q, kp, vp, out, lk, heads, scale, prescaled=prescaled, lse=lse), lse


def attention_generic(q, k, v, out, lk, heads, head_dim, scale):
    _chk(q, torch.bfloat16, 'q'); _chk(k, torch.bfloat16, 'k'); _chk(v, torch.bfloat16, 'v')
    _chk(out, torch.bfloat16, 'out')
    lib.call('mg_attn_fwd_bf16_generic', _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out),
             out.stride(0), q.shape[0], int(lk), int(heads), int(head_dim), float(scale), _st())
    return out


def sinusoid_embed(t, dim, out):
    """t [n] int64 / fp32 / fp64 positions -> out [n, dim] fp32 = cos(t w_j) | sin(t w_j), w_j = 10000^(-j / (dim/2)), evaluated in fp64."""
    code = {torch.int64: 0, torch.float32: 1, torch.float64: 2}.get(t.dtype)
    if code is None or not t.is_cuda or not t.is_contiguous():
        raise lib.MoviigenHipError('timestep must be a contiguous CUDA int64/float32/float64 tensor')
    _chk_flat(out, torch.float32, 'out')
    dim = int(dim)
    if dim <= 0 or dim % 2 or out.numel() != t.numel() * dim:
        raise lib.MoviigenHipError(f'sinusoid_embed: dim {dim} must be even and out {tuple(out.shape)} hold {t.numel()} rows of it')
    lib.call('mg_sinusoid_embed', _p(t), code, t.numel(), dim, _p(out), _st())
    return out


def gemv(w, bias, x, y, silu_in=False):
    """y [N] = w [N, K] @ (silu(x) if silu_in else x) [K] + bias [N] (None = 0): dense fp32 tensors, K a multiple of 4."""
    _chk_flat(w, torch.float32, 'w'); _chk_flat(bias, torch.float32, 'bias', optional=True)
    _chk_flat(x, torch.float32, 'x'); _chk_flat(y, torch.float32, 'y')
    if w.dim() != 2 or w.shape[1] % 4 or x.numel() != w.shape[1] or y.numel() != w.shape[0] or (bias is not None and bias.numel() != w.shape[0]):
        raise lib.MoviigenHipError(f'gemv shape mismatch w{tuple(w.shape)} (K a multiple of 4) x{tuple(x.shape)} y{tuple(y.shape)}'
                                   + ('' if bias is None else f' bias{tuple(bias.shape)}'))
    lib.call('mg_gemv_f32', _p(w), _p(bias), _p(x), _p(y), w.shape[0], w.shape[1], int(silu_in), _st())
    return y


def add_rows(a, b, out, period):
    """out [rows, dim] = a [rows, dim] + b [>= period, dim] with row r of a meeting row r % period of b: dense fp32 tensors."""
    _chk_flat(a, torch.float32, 'a'); _chk_flat(b, torch.float32, 'b'); _chk_flat(out, torch.float32, 'out')
    period = int(period)
    if a.dim() != 2 or b.dim() != 2 or period < 1 or b.shape[0] < period or b.shape[1] != a.shape[1] or tuple(out.shape) != tuple(a.shape):
        raise lib.MoviigenHipError(f'add_rows shape mismatch a{tuple(a.shape)} b{tuple(b.shape)} out{tuple(out.shape)} period {period}')
    rows, dim = a.shape
    lib.call('mg_add_rows_f32', _p(a), _p(b), _p(out), rows, dim, period, _st())
    return out


def head_gemm(x, w, bias, out):
    """out [M, N <= 64] = x [M, K] @ w [N, K]^T + bias [N] (None = 0) in fp32: x may be a column slice (row stride free), w and out are dense."""
    _chk_rows(x, torch.float32, 'x'); _chk_flat(w, torch.float32, 'w'); _chk_flat(bias, torch.float32, 'bias', optional=True)
    _chk_flat(out, torch.float32, 'out')
    if w.dim() != 2 or w.shape[0] > 64 or w.shape[1] != x.shape[1] or tuple(out.shape) != (x.shape[0], w.shape[0]) \
            or (bias is not None and bias.numel() != w.shape[0]):
        raise lib.MoviigenHipError(f'head_gemm shape mismatch x{tuple(x.shape)} w{tuple(w.shape)} (N <= 64) out{tuple(out.shape)}'
                                   + ('' if bias is None else f' bias{tuple(bias.shape)}'))
    lib.call('mg_head_gemm_f32', _p(x), x.stride(0), _p(w), _p(bias), _p(out), x.shape[0], w.shape[0], w.shape[1],
             _st())
    return out


def patchify(lat, ph, pw, out):
    """lat [C, F, H, W] fp32 dense -> out [>= F (H/ph) (W/pw), >= C ph pw] bf16 (row stride free): row = patch in (f, h, w) order,
    column = (c, i, j); columns behind C ph pw are not written."""
    _chk_flat(lat, torch.float32, 'lat'); _chk_rows(out, torch.bfloat16, 'out')
    ph, pw = int(ph), int(pw)
    if lat.dim() != 4 or ph < 1 or pw < 1 or lat.shape[2] % ph or lat.shape[3] % pw:
        raise lib.MoviigenHipError(f'patchify: lat {tuple(lat.shape)} is not [C, F, H, W] with H, W multiples of the patch {(ph, pw)}')
    C, F, H, W = lat.shape
    if out.shape[0] < F * (H // ph) * (W // pw) or out.shape[1] < C * ph * pw:
        raise lib.MoviigenHipError(f'patchify: out {tuple(out.shape)} is smaller than [{F * (H // ph) * (W // pw)}, {C * ph * pw}]')
    lib.call('mg_patchify_bf16', _p(lat), C, F, H, W, ph, pw, _p(out), out.stride(0), _st())
    return out


def unpatchify(tok, C, F, Hg, Wg, ph, pw, lat):
    """tok [>= F Hg Wg, >= ph pw C] fp32 (row stride free), column = (i, j, c) -> lat [C, F, Hg ph, Wg pw] fp32 dense."""
    _chk_rows(tok, torch.float32, 'tok'); _chk_flat(lat, torch.float32, 'lat')
    C, F, Hg, Wg, ph, pw = (int(v) for v in (C, F, Hg, Wg, ph, pw))
    if min(C, F, Hg, Wg, ph, pw) < 1 or tok.shape[0] < F * Hg * Wg or tok.shape[1] < ph * pw * C or lat.numel() != C * F * Hg * ph * Wg * pw:
        raise lib.MoviigenHipError(f'unpatchify: tok {tuple(tok.shape)}, lat {tuple(lat.shape)} do not fit (C, F, Hg, Wg, ph, pw) = '
                                   f'{(C, F, Hg, Wg, ph, pw)}')
    lib.call('mg_unpatchify_f32', _p(tok), tok.stride(0), C, F, Hg, Wg, ph, pw, _p(lat), _st())
    return lat


def lincomb(out, terms):
    """out = sum(c_i * x_i) for 1 to 4 (tensor, coef) terms: dense fp32 tensors of out's size."""
    terms = list(terms)
    _chk_flat(out, torch.float32, 'out')
    if not 1 <= len(terms) <= 4:
        raise lib.MoviigenHipError(f'lincomb takes 1 to 4 terms, got {len(terms)}')
    args = []
    for i, (x, c) in enumerate(terms):
        _chk_flat(x, torch.float32, f'x{i}')
        if x.numel() != out.numel():
            raise lib.MoviigenHipError(f'lincomb size mismatch out{tuple(out.shape)} x{i}{tuple(x.shape)}')
        args += [_p(x), float(c)]
    args += [None, 0.0] * (4 - len(terms))
    lib.call('mg_lincomb4_f32', _p(out), out.numel(), *args, _st())
    return out


def lora_merge(w, up, down):
    """w [N, K] bf16 or fp32, IN PLACE: w <- round(w + up [N, R] fp32 @ down [R, K] fp32), fp32 products and sums, one rounding for
    bf16 storage (include/moviigen_hip.h).  w may be a row slice or a column view of a larger matrix (row stride free, a multiple of
    16 bytes): nothing outside [N, K] is written."""
    if not torch.is_tensor(w) or w.dtype not in (torch.bfloat16, torch.float32):
        raise lib.MoviigenHipError(f'w: expected a bf16 or fp32 tensor, got {getattr(w, "dtype", type(w))}')
    _chk(w, w.dtype, 'w'); _chk(up, torch.float32, 'up'); _chk(down, torch.float32, 'down')
    if w.dim() != 2 or up.dim() != 2 or down.dim() != 2 or up.shape[0] != w.shape[0] or down.shape[1] != w.shape[1] \
            or up.shape[1] != down.shape[0]:
        raise lib.MoviigenHipError(f'lora_merge shape mismatch w{tuple(w.shape)} up{tuple(up.shape)} down{tuple(down.shape)}')
    N, K = w.shape
    lib.call('mg_lora_merge', _p(w), int(w.dtype == torch.float32), w.stride(0), N, K, _p(up), up.stride(0), _p(down),
             down.stride(0), up.shape[1], _st())
    return w


def cfg_combine(out, uncond, cond, g):
    """out = uncond + g * (cond - uncond): dense fp32 tensors of one size."""
    _chk_flat(out, torch.float32, 'out'); _chk_flat(uncond, torch.float32, 'uncond'); _chk_flat(cond, torch.float32, 'cond')
    if uncond.numel() != out.numel() or cond.numel() != out.numel():
        raise lib.MoviigenHipError(f'cfg_combine size mismatch out{tuple(out.shape)} uncond{tuple(uncond.shape)} cond{tuple(cond.shape)}')
    lib.call('mg_cfg_combine_f32', _p(out), _p(uncond), _p(cond), float(g), out.numel(), _st())
    return out


def cfg_stats_partials(device):
    """the caller-owned scratch of cfg_stats: mg_cfg_stats_partials_bytes() bytes as fp64, no initial value needed"""
    return torch.empty(int(lib.load().mg_cfg_stats_partials_bytes()) // 8, dtype=torch.float64, device=device)


def _chk_aligned16(t, name):
    if t.data_ptr() % 16:
        raise lib.MoviigenHipError(f'{name}: must be 16-byte aligned (a view that starts inside a row is not)')


def cfg_stats(uncond, cond, stats, partials):
    """stats fp64 [5] <- (sum u, sum c, sum u^2, sum c^2, sum u c) over the dense fp32 tensors uncond (u) and cond (c) of one size:
    fp64 products and sums in a fixed order (the same inputs give the same 40 bytes), no host read; partials: cfg_stats_partials(device).
    The inputs are only read.  DESIGN.md 3.8."""
    _chk_flat(uncond, torch.float32, 'uncond'); _chk_flat(cond, torch.float32, 'cond')
    _chk_flat(stats, torch.float64, 'stats'); _chk_flat(partials, torch.float64, 'partials')
    if uncond.numel() < 1 or cond.numel() != uncond.numel():
        raise lib.MoviigenHipError(f'cfg_stats size mismatch uncond{tuple(uncond.shape)} cond{tuple(cond.shape)} (at least one element)')
    if stats.numel() != 5 or partials.numel() * 8 < int(lib.load().mg_cfg_stats_partials_bytes()):
        raise lib.MoviigenHipError('cfg_stats: stats must be fp64 [5] and partials cfg_stats_partials(device)')
    _chk_aligned16(uncond, 'uncond'); _chk_aligned16(cond, 'cond')
    lib.call('mg_cfg_stats_f32', _p(uncond), _p(cond), uncond.numel(), _p(stats), _p(partials), _st())
    return stats


def cfg_coefficients(stats, n, g, zero_star, rescale, coef):
    """coef fp32 [2] <- (a_u, a_c) of the guided prediction a_u u + a_c c from cfg_stats' sums over n elements: guide scale g, CFG-Zero*'s
    projection when zero_star, guidance rescale by `rescale` in [0, 1] (0 = off) — on the device, in fp64 (include/moviigen_hip.h)."""
    _chk_flat(stats, torch.float64, 'stats'); _chk_flat(coef, torch.float32, 'coef')
    g, rescale = float(g), float(rescale)
    if stats.numel() != 5 or coef.numel() != 2 or int(n) < 1:
        raise lib.MoviigenHipError(f'cfg_coefficients: stats must be fp64 [5], coef fp32 [2], n >= 1; got {tuple(stats.shape)}, {tuple(coef.shape)}, {n}')
    if g != g or abs(g) == float('inf') or not 0.0 <= rescale <= 1.0:
        raise lib.MoviigenHipError(f'cfg_coefficients: g must be finite and rescale in [0, 1], got {g}, {rescale}')
    lib.call('mg_cfg_coef_f32', _p(stats), int(n), g, int(bool(zero_star)), rescale, _p(coef), _st())
    return coef


def cfg_combine_coef(out, uncond, cond, coef):
    """out = a_u * uncond + a_c * cond with (a_u, a_c) = coef fp32 [2] ON THE DEVICE (cfg_coefficients): the bits of
    lincomb(out, [(uncond, a_u), (cond, a_c)]).  Dense fp32 tensors of one size; out may be uncond or cond."""
    _chk_flat(out, torch.float32, 'out'); _chk_flat(uncond, torch.float32, 'uncond'); _chk_flat(cond, torch.float32, 'cond')
    _chk_flat(coef, torch.float32, 'coef')
    if uncond.numel() != out.numel() or cond.numel() != out.numel():
        raise lib.MoviigenHipError(f'cfg_combine_coef size mismatch out{tuple(out.shape)} uncond{tuple(uncond.shape)} cond{tuple(cond.shape)}')
    if coef.numel() != 2:
        raise lib.MoviigenHipError(f'cfg_combine_coef: coef must be fp32 [2], got {tuple(coef.shape)}')
    _chk_aligned16(out, 'out'); _chk_aligned16(uncond, 'uncond'); _chk_aligned16(cond, 'cond')
    lib.call('mg_cfg_combine_coef_f32', _p(out), _p(uncond), _p(cond), out.numel(), _p(coef), _st())
    return out


def nag_combine(zp, zn, out, scale, tau, alpha):
    """out [rows, dim] bf16 <- the normalized-attention-guidance mix of the cross-attention outputs zp (positive prompt) and zn (negative
    prompt), per row: g = scale zp - (scale - 1) zn, clipped to tau times zp's L1 norm, blended with zp by alpha (include/moviigen_hip.h,
    DESIGN.md 3.11).  Row strides are free (multiples of 8); out may be zp itself, not zn.  1 <= scale <= 64, tau >= 1, 0 <= alpha <= 1."""
    _chk_rows(zp, torch.bfloat16, 'zp'); _chk_rows(zn, torch.bfloat16, 'zn'); _chk_rows(out, torch.bfloat16, 'out')
    if tuple(zn.shape) != tuple(zp.shape) or tuple(out.shape) != tuple(zp.shape):
        raise lib.MoviigenHipError(f'nag_combine shape mismatch zp{tuple(zp.shape)} zn{tuple(zn.shape)} out{tuple(out.shape)}')
    rows, dim = zp.shape
    if dim < 8 or dim % 8 or dim > 8192:
        raise lib.MoviigenHipError(f'nag_combine: dim must be a multiple of 8 in [8, 8192], got {dim}')
    for name, t in (('zp', zp), ('zn', zn), ('out', out)):
        if t.stride(0) % 8 or (rows == 1 and t.stride(0) < dim):
            raise lib.MoviigenHipError(f'nag_combine: {name} needs a row stride that is a multiple of 8 and >= dim, got {t.stride(0)}')
        _chk_aligned16(t, name)
    scale, tau, alpha = float(scale), float(tau), float(alpha)
    if not (1.0 <= scale <= 64.0 and 1.0 <= tau < float('inf') and 0.0 <= alpha <= 1.0):
        raise lib.MoviigenHipError(f'nag_combine: 1 <= scale <= 64, 1 <= tau < inf, 0 <= alpha <= 1; got {scale}, {tau}, {alpha}')
    if rows == 0:
        return out
    lib.call('mg_nag_combine_bf16', _p(zp), zp.stride(0), _p(zn), zn.stride(0), _p(out), out.stride(0), rows, dim, scale, tau, alpha, _st())
    return out


# ---- umT5 encoder glue ---------------------------------------------------------------------------
def embed_rows(table, ids, out):
    """out [n, dim] = table [vocab, dim][ids [n]] (ids clamped to the table): dense bf16 / int64 tensors, dim a multiple of 8."""
    _chk_flat(table, torch.bfloat16, 'table'); _chk_flat(ids, torch.int64, 'ids'); _chk_flat(out, torch.bfloat16, 'out')
    if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] % 8 or tuple(out.shape) != (ids.numel(), table.shape[1]):
        raise lib.MoviigenHipError(f'embed_rows shape mismatch table{tuple(table.shape)} (dim a multiple of 8) ids{tuple(ids.shape)} '
                                   f'out{tuple(out.shape)}')
    lib.call('mg_embed_rows_bf16', _p(table), table.shape[0], table.shape[1], _p(ids), ids.numel(), _p(out), _st())
    return out


def ew_bf16(a, b, out, mode):
    """mode 0: a + b; mode 1: a * gelu_tanh(b) — contiguous bf16 tensors of equal size."""
    for n, t in (('a', a), ('b', b), ('out', out)):
        _chk(t, torch.bfloat16, n)
        if not t.is_contiguous():
            raise lib.MoviigenHipError(f'{n} must be contiguous')
    lib.call('mg_ew_bf16', _p(a), _p(b), _p(out), out.numel(), int(mode), _st())
    return out


def t5_attention(q, k, v, rel_emb, rel_bucket, out, lk, heads, head_dim):
    """q, k, v: column slices of one [L, 3*heads*head_dim] buffer (same row stride)."""
    _chk(q, torch.bfloat16, 'q'); _chk(k, torch.bfloat16, 'k'); _chk(v, torch.bfloat16, 'v')
    _chk(rel_emb, torch.bfloat16, 'rel_emb'); _chk(rel_bucket, torch.int32, 'rel_bucket'); _chk(out, torch.bfloat16, 'out')
    if not (q.stride(0) == k.stride(0) == v.stride(0)):
        raise lib.MoviigenHipError('q, k, v must share a row stride')
    if rel_bucket.numel() != q.shape[0] + int(lk) - 1:
        raise lib.MoviigenHipError('rel_bucket must have Lq + Lk - 1 entries')
    lib.call('mg_t5_attn_bf16', _p(q), _p(k), _p(v), q.stride(0), _p(rel_emb), _p(rel_bucket), _p(out), out.stride(0),
             q.shape[0], int(lk), int(heads), int(head_dim), _st())
    return out


# ---- VAE (fp32, channels-last) -------------------------------------------------------------------
VAE_EXACT, VAE_BF16X3 = 0, 1     # MG_VAE_EXACT / MG_VAE_BF16X3 (include/moviigen_hip.h): the arithmetic of one convolution call


def _vae_err(what, msg):
    raise lib.MoviigenHipError(f'{what}: {msg}')


def _vae_conv_geometry(what, x, w, bias, cache, kernel):
    """the operands every VAE convolution shares: x [T,H,W,Cin] dense; w dense, [Cout,kt,kh,kw,Cin] for kernel = (kt, kh, kw) or the folded
    [4,Cout,2,2,Cin] for kernel = 'phases'; bias of Cout floats; cache dense, at most kt - 1 frames of x's geometry.
    -> (T, H, W, Cin, Cout, tc)"""
    _chk_flat(x, torch.float32, f'{what}: x')
    _chk_flat(w, torch.float32, f'{what}: w')
    _chk_flat(bias, torch.float32, f'{what}: bias', optional=True)
    _chk_flat(cache, torch.float32, f'{what}: cache', optional=True)
    if x.dim() != 4 or w.dim() != 5:
        _vae_err(what, f'x must be [T, H, W, Cin] and w have five dimensions, got {tuple(x.shape)} and {tuple(w.shape)}')
    T, H, W, Cin = x.shape
    if kernel == 'phases':
        Cout, kt = w.shape[1], 1
        want = (4, Cout, 2, 2, Cin)
    else:
        Cout, kt = w.shape[0], kernel[0]
        want = (Cout, *kernel, Cin)
    if tuple(w.shape) != want:
        _vae_err(what, f'w must be {want} for x {tuple(x.shape)}, got {tuple(w.shape)}')
    if Cout > 4 and Cout % 4:
        _vae_err(what, f'Cout = {Cout}: more than 4 output channels have to be a multiple of 4 (the rows of out and residual move as float4)')
    if bias is not None and bias.numel() != Cout:
        _vae_err(what, f'bias has {bias.numel()} elements, Cout is {Cout}')
    tc = 0
    if cache is not None:
        if cache.dim() != 4 or tuple(cache.shape[1:]) != (H, W, Cin) or cache.shape[0] > kt - 1:
            _vae_err(what, f'the cache must be at most {kt - 1} frames with the frame geometry of x {tuple(x.shape)}, got {tuple(cache.shape)}')
        tc = cache.shape[0]
    return T, H, W, Cin, Cout, tc


def _vae_conv_out(what, out, residual, want):
    """out, and residual when given: dense fp32 of exactly the shape the kernel writes"""
    _chk_flat(out, torch.float32, f'{what}: out')
    _chk_flat(residual, torch.float32, f'{what}: residual', optional=True)
    for n, t in (('out', out), ('residual', residual)):
        if t is not None and tuple(t.shape) != want:
            _vae_err(what, f'{n} must be {want}, got {tuple(t.shape)}')


def vae_conv(x, w, bias, out, kt, kh, kw, cache=None, up2=False, residual=None, mode=VAE_EXACT):
    """x [T,H,W,Cin]; w [Cout,kt,kh,kw,Cin]; out [T,Ho,Wo,Cout]."""
    kt, kh, kw = int(kt), int(kh), int(kw)
    T, H, W, Cin, Cout, tc = _vae_conv_geometry('vae_conv', x, w, bias, cache, (kt, kh, kw))
    _vae_conv_out('vae_conv', out, residual, (T, 2 * H, 2 * W, Cout) if up2 else (T, H, W, Cout))
    lib.call('mg_vae_conv_f32', _p(x), _p(cache), tc, T, H, W, Cin, _p(w), _p(bias), Cout, kt, kh, kw,
             int(up2), _p(residual), _p(out), int(mode), _st())
    return out


def vae_conv_cols(x, w, bias, out, kt, kh, kw, col0, cache=None, residual=None, mode=VAE_EXACT):
    """the W-band form: x [T,H,W,Cin] and cache carry the neighbours' halo columns; out (and residual) [T,H,cols,Cout] compact =
    the output columns [col0, col0 + cols) of vae_conv on the whole image."""
    kt, kh, kw, col0 = int(kt), int(kh), int(kw), int(col0)
    T, H, W, Cin, Cout, tc = _vae_conv_geometry('vae_conv_cols', x, w, bias, cache, (kt, kh, kw))
    _chk_flat(out, torch.float32, 'vae_conv_cols: out')
    cols = out.shape[2] if out.dim() == 4 else 0
    if col0 < 0 or cols < 1 or col0 + cols > W:
        _vae_err('vae_conv_cols', f'columns [{col0}, {col0} + {cols}) of out {tuple(out.shape)} are not inside x {tuple(x.shape)}')
    _vae_conv_out('vae_conv_cols', out, residual, (T, H, cols, Cout))
    lib.call('mg_vae_conv_cols_f32', _p(x), _p(cache), tc, T, H, W, Cin, _p(w), _p(bias), Cout, kt, kh, kw,
             _p(residual), _p(out), col0, int(cols), int(mode), _st())
    return out


def vae_upconv_fold_weights(w):
    """w [Cout,1,3,3,Cin] (the conv behind a nearest-2x upsample) -> [4,Cout,2,2,Cin]: one 2x2 kernel per output parity."""
    _chk_flat(w, torch.float32, 'vae_upconv_fold_weights: w')
    if w.dim() != 5:
        _vae_err('vae_upconv_fold_weights', f'w must be [Cout, 1, 3, 3, Cin], got {tuple(w.shape)}')
    Cout, kt, kh, kw, Cin = w.shape
    if (kt, kh, kw) != (1, 3, 3):
        raise ValueError(f'the phase decomposition is defined for 1x3x3 kernels, got {kt}x{kh}x{kw}')
    wp = torch.empty(4, Cout, 2, 2, Cin, dtype=torch.float32, device=w.device)
    lib.call('mg_vae_upconv_fold_weights_f32', _p(w), Cout, Cin, _p(wp), _st())
    return wp


def vae_upconv_phases(x, wp, bias, out, mode=VAE_EXACT):
    """x [T,H,W,Cin]; wp from vae_upconv_fold_weights; out [T,2H,2W,Cout] = conv3x3(nearest-2x(x))."""
    T, H, W, Cin, Cout, _ = _vae_conv_geometry('vae_upconv_phases', x, wp, bias, None, 'phases')
    _vae_conv_out('vae_upconv_phases', out, None, (T, 2 * H, 2 * W, Cout))
    lib.call('mg_vae_upconv_phases_f32', _p(x), T, H, W, Cin, _p(wp), _p(bias), Cout, _p(out), int(mode), _st())
    return out


def vae_upconv_phases_cols(x, wp, bias, out, col0, mode=VAE_EXACT):
    """the W-band form of vae_upconv_phases: x [T,H,W,Cin] with halo columns, out [T,2H,2 cols,Cout] compact."""
    col0 = int(col0)
    T, H, W, Cin, Cout, _ = _vae_conv_geometry('vae_upconv_phases_cols', x, wp, bias, None, 'phases')
    _chk_flat(out, torch.float32, 'vae_upconv_phases_cols: out')
    cols2 = out.shape[2] if out.dim() == 4 else 1
    cols = cols2 // 2
    if cols2 % 2 or col0 < 0 or cols < 1 or col0 + cols > W:
        _vae_err('vae_upconv_phases_cols', f'out {tuple(out.shape)} is not [T, 2H, 2 cols, Cout] for columns [{col0}, {col0} + cols) inside x {tuple(x.shape)}')
    _vae_conv_out('vae_upconv_phases_cols', out, None, (T, 2 * H, 2 * cols, Cout))
    lib.call('mg_vae_upconv_phases_cols_f32', _p(x), T, H, W, Cin, _p(wp), _p(bias), Cout, _p(out), col0, cols, int(mode), _st())
    return out


def vae_rmsnorm_silu(x, gamma, out, do_silu=True):
    """x [..., C] -> out of the same shape: x / max(|x|, 1e-12) * sqrt(C) * gamma over the last dimension, then SiLU when do_silu."""
    for n, t in (('x', x), ('gamma', gamma), ('out', out)):
        _chk_flat(t, torch.float32, f'vae_rmsnorm_silu: {n}')
    if x.dim() < 1 or x.shape[-1] < 1:
        _vae_err('vae_rmsnorm_silu', f'x must be [..., C], got {tuple(x.shape)}')
    C = x.shape[-1]
    if gamma.numel() != C or out.shape != x.shape:
        _vae_err('vae_rmsnorm_silu', f'x {tuple(x.shape)} needs a gamma of {C} elements and an out of its shape, got {tuple(gamma.shape)} and {tuple(out.shape)}')
    lib.call('mg_vae_rmsnorm_silu_f32', _p(x), _p(gamma), _p(out), x.numel() // C, C, int(do_silu), _st())
    return out


def vae_attn_workspace_floats(L, C):
    return int(lib.load().mg_vae_attn_workspace_floats(int(L), int(C)))


def vae_attn(qkv, out, workspace):
    """qkv [frames, L, 3C] = q | k | v per pixel, out [frames, L, C] = softmax(q k^T / sqrt(C)) v per frame."""
    for n, t in (('qkv', qkv), ('out', out), ('workspace', workspace)):
        _chk_flat(t, torch.float32, f'vae_attn: {n}')
    if qkv.dim() != 3 or qkv.shape[2] % 3 or qkv.shape[2] == 0:
        _vae_err('vae_attn', f'qkv must be [frames, L, 3C], got {tuple(qkv.shape)}')
    frames, L, C3 = qkv.shape
    C = C3 // 3
    if tuple(out.shape) != (frames, L, C):
        _vae_err('vae_attn', f'out must be {(frames, L, C)}, got {tuple(out.shape)}')
    if workspace.numel() < vae_attn_workspace_floats(L, C):
        raise lib.MoviigenHipError('vae_attn workspace too small')
    lib.call('mg_vae_attn_f32', _p(qkv), _p(out), frames, L, C, _p(workspace), _st())
    return out


def vae_attn_rows(q, kv, out, workspace):
    """q [frames, Lq, >= C] (a column slice of the band's q|k|v is fine), kv [frames, Lk, 2C] = k | v of ALL pixels of the frame in image
    order, out [frames, Lq, C]: the band's rows of vae_attn, same bits."""
    _chk(q, torch.float32, 'vae_attn_rows: q')
    for n, t in (('kv', kv), ('out', out), ('workspace', workspace)):
        _chk_flat(t, torch.float32, f'vae_attn_rows: {n}')
    if q is None or q.dim() != 3 or kv.dim() != 3 or kv.shape[2] % 2 or kv.shape[2] == 0:
        _vae_err('vae_attn_rows', f'q must be [frames, Lq, >= C] and kv [frames, Lk, 2C], got {None if q is None else tuple(q.shape)} and {tuple(kv.shape)}')
    frames, Lq = q.shape[:2]
    Lk, C = kv.shape[1], kv.shape[2] // 2
    if Lq > Lk:
        _vae_err('vae_attn_rows', f'Lq = {Lq} query rows exceed the Lk = {Lk} keys: the queries are a subset of the frame\'s pixels')
    if kv.shape[0] != frames or q.shape[2] < C or q.stride(1) < q.shape[2] or q.stride(0) != Lq * q.stride(1) or tuple(out.shape) != (frames, Lq, C):
        _vae_err('vae_attn_rows', f'shapes: q {tuple(q.shape)} with strides {tuple(q.stride())}, kv {tuple(kv.shape)}, out {tuple(out.shape)}')
    if workspace.numel() < vae_attn_workspace_floats(Lk, C):
        raise lib.MoviigenHipError('vae_attn workspace too small')
    lib.call('mg_vae_attn_rows_f32', _p(q), q.stride(1), _p(kv), ctypes.c_void_p(kv.data_ptr() + 4 * C), 2 * C, _p(out), frames, Lq, Lk, C,
             _p(workspace), _st())
    return out


def vae_latent_in(z, mean, inv_std, out):
    """z [C,T,H,W] -> out [T,H,W,C] = z / inv_std + mean per channel."""
    for n, t in (('z', z), ('mean', mean), ('inv_std', inv_std), ('out', out)):
        _chk_flat(t, torch.float32, f'vae_latent_in: {n}')
    if z.dim() != 4:
        _vae_err('vae_latent_in', f'z must be [C, T, H, W], got {tuple(z.shape)}')
    C, T, H, W = z.shape
    if tuple(out.shape) != (T, H, W, C) or mean.numel() < C or inv_std.numel() < C:
        _vae_err('vae_latent_in', f'z {tuple(z.shape)} needs out {(T, H, W, C)} and {C} means and scales, got out {tuple(out.shape)}, '
                                  f'{mean.numel()} and {inv_std.numel()}')
    lib.call('mg_vae_latent_in_f32', _p(z), _p(mean), _p(inv_std), C, T, H, W, _p(out), _st())
    return out


def vae_video_out(x, out, t_off):
    """x [T,H,W,C] -> out[:, t_off:t_off + T] of out [C,T_total,H,W], clamped to [-1, 1] (NaN becomes -1)."""
    _chk_flat(x, torch.float32, 'vae_video_out: x')
    _chk_flat(out, torch.float32, 'vae_video_out: out')
    if x.dim() != 4 or out.dim() != 4:
        _vae_err('vae_video_out', f'x must be [T, H, W, C] and out [C, T_total, H, W], got {tuple(x.shape)} and {tuple(out.shape)}')
    T, H, W, C = x.shape
    t_off = int(t_off)
    if (out.shape[0], out.shape[2], out.shape[3]) != (C, H, W) or t_off < 0 or t_off + T > out.shape[1]:
        _vae_err('vae_video_out', f'frames [{t_off}, {t_off} + {T}) of x {tuple(x.shape)} do not fit out {tuple(out.shape)}')
    lib.call('mg_vae_video_out_f32', _p(x), C, T, H, W, _p(out), t_off, out.shape[1], _st())
    return out


def vae_time_interleave(x, out):
    """x [T,H,W,2C] -> out [2T,H,W,C]: frame 2t from channels [0, C), frame 2t + 1 from [C, 2C)."""
    _chk_flat(x, torch.float32, 'vae_time_interleave: x')
    _chk_flat(out, torch.float32, 'vae_time_interleave: out')
    if x.dim() != 4 or x.shape[3] % 2 or x.shape[3] == 0:
        _vae_err('vae_time_interleave', f'x must be [T, H, W, 2C], got {tuple(x.shape)}')
    T, H, W, C2 = x.shape
    if tuple(out.shape) != (2 * T, H, W, C2 // 2):
        _vae_err('vae_time_interleave', f'out must be {(2 * T, H, W, C2 // 2)}, got {tuple(out.shape)}')
    lib.call('mg_vae_time_interleave_f32', _p(x), T, H * W, C2 // 2, _p(out), _st())
    return out


def vae_conv_strided_out_shape(x_shape, kernel, stride, pad_t0, pad_h, pad_w):
    """[To, Ho, Wo] of vae_conv_strided: n_out = (n + pad0 + pad1 - k) // stride + 1 per axis."""
    T, H, W = x_shape[:3]
    (kt, kh, kw), (st, sh, sw) = kernel, stride
    return [(T + pad_t0 - kt) // st + 1, (H + pad_h[0] + pad_h[1] - kh) // sh + 1, (W + pad_w[0] + pad_w[1] - kw) // sw + 1]


def vae_conv_strided(x, w, bias, out, stride, pad_t0=0, pad_h=(0, 0), pad_w=(0, 0), cache=None, mode=VAE_EXACT):
    """x [T,H,W,Cin]; w [Cout,kt,kh,kw,Cin]; out [To,Ho,Wo,Cout] (vae_conv_strided_out_shape): the encoder's down-sampling
    convolutions — stride per axis, zero rows / columns pad_h / pad_w = (before, behind), pad_t0 frames before the chunk
    from `cache` (its last frames)."""
    for n, t in (('x', x), ('w', w), ('bias', bias), ('out', out), ('cache', cache)):
        _chk(t, torch.float32, n)
    T, H, W, Cin = x.shape
    Cout, kt, kh, kw, wc = w.shape
    want = vae_conv_strided_out_shape(x.shape, (kt, kh, kw), stride, pad_t0, pad_h, pad_w) + [Cout]
    if wc != Cin or list(out.shape) != want or not out.is_contiguous() or not x.is_contiguous() or not w.is_contiguous():
        raise lib.MoviigenHipError(f'vae_conv_strided: x {tuple(x.shape)}, w {tuple(w.shape)} need a contiguous out {want}, got {tuple(out.shape)}')
    if cache is not None and (tuple(cache.shape[1:]) != tuple(x.shape[1:]) or not cache.is_contiguous()):
        raise lib.MoviigenHipError('vae_conv_strided: the cache must have the frame geometry of x')
    tc = 0 if cache is None else cache.shape[0]
    lib.call('mg_vae_conv_strided_f32', _p(x), _p(cache), tc, T, H, W, Cin, _p(w), _p(bias), Cout, kt, kh, kw, int(stride[0]), int(stride[1]),
             int(stride[2]), int(pad_t0), int(pad_h[0]), int(pad_h[1]), int(pad_w[0]), int(pad_w[1]), _p(out), int(mode), _st())
    return out


def vae_video_in(video, t0, n, out):
    """video [3,T,H,W] fp32, frames [t0, t0 + n) -> out [n,H,W+2,4]: the staged layout of vae_conv_in3 (zero columns 0 and W+1, zero channel 3)."""
    _chk(video, torch.float32, 'video'); _chk(out, torch.float32, 'out')
    if video.dim() != 4 or video.shape[0] != 3 or not video.is_contiguous():
        raise lib.MoviigenHipError('video must be a contiguous [3, T, H, W] tensor')
    _, T, H, W = video.shape
    if tuple(out.shape) != (n, H, W + 2, 4) or not out.is_contiguous():
        raise lib.MoviigenHipError(f'vae_video_in: out must be a contiguous {(n, H, W + 2, 4)} tensor, got {tuple(out.shape)}')
    lib.call('mg_vae_video_in_f32', _p(video), T, H, W, int(t0), int(n), _p(out), _st())
    return out


def vae_conv_in3(xs, w, bias, out, cache=None, mode=VAE_EXACT):
    """the 3 -> Cout causal 3x3x3 input convolution: xs [T,H,W+2,4] from vae_video_in, cache [<= 2,H,W+2,4] staged frames of the
    previous chunk, w [Cout,3,3,3,4] (channel 3 zero), out [T,H,W,Cout]."""
    for n, t in (('xs', xs), ('w', w), ('bias', bias), ('out', out), ('cache', cache)):
        _chk(t, torch.float32, n)
    T, H, Wp, c4 = xs.shape
    Cout = w.shape[0]
    if c4 != 4 or tuple(w.shape) != (Cout, 3, 3, 3, 4) or tuple(out.shape) != (T, H, Wp - 2, Cout) or not (xs.is_contiguous() and w.is_contiguous()
                                                                                                     and out.is_contiguous()):
        raise lib.MoviigenHipError(f'vae_conv_in3: xs {tuple(xs.shape)}, w {tuple(w.shape)}, out {tuple(out.shape)}')
    if cache is not None and (tuple(cache.shape[1:]) != tuple(xs.shape[1:]) or not cache.is_contiguous()):
        raise lib.MoviigenHipError('vae_conv_in3: the cache must have the staged frame geometry of xs')
    tc = 0 if cache is None else cache.shape[0]
    lib.call('mg_vae_conv_in3_f32', _p(xs), _p(cache), tc, T, H, Wp - 2, _p(w), _p(bias), Cout, _p(out), int(mode), _st())
    return out


def vae_latent_out(x, mean, inv_std, out):
    """x [T,H,W,Cx] channels-last -> out [C,T,H,W] = (x[..., :C] - mean) * inv_std (C = out.shape[0] <= Cx)."""
    for n, t in (('x', x), ('mean', mean), ('inv_std', inv_std), ('out', out)):
        _chk(t, torch.float32, n)
    T, H, W, Cx = x.shape
    C = out.shape[0]
    if tuple(out.shape) != (C, T, H, W) or C > Cx or mean.numel() < C or inv_std.numel() < C or not (x.is_contiguous() and out.is_contiguous()):
        raise lib.MoviigenHipError(f'vae_latent_out: x {tuple(x.shape)}, out {tuple(out.shape)}')
    lib.call('mg_vae_latent_out_f32', _p(x), Cx, _p(mean), _p(inv_std), C, T, H, W, _p(out), _st())
    return out


def video_to_u8(video, lo=-1.0, hi=1.0):
    """[3,T,H,W] fp32 -> uint8 frames [T,H,W,3] (reference cache_video arithmetic)."""
    _chk(video, torch.float32, 'video')
    if video.dim() != 4 or video.shape[0] != 3 or not video.is_contiguous():
        raise lib.MoviigenHipError('video must be a contiguous [3, T, H, W] tensor')
    _, T, H, W = video.shape
    out = torch.empty(T, H, W, 3, dtype=torch.uint8, device=video.device)
    lib.call('mg_video_to_u8', _p(video), T, H, W, float(lo), float(hi), _p(out), _st())
    return out


def video_from_u8(frames, H, W, out=None):
    """uint8 RGB frames [T,H0,W0,3] of any size -> the clip [3,T,H,W] fp32 in [-1,1]: resize to cover (antialiased triangle filter),
    centre crop, v / 127.5 - 1 (mg_video_from_u8; the definition is in include/moviigen_hip.h)."""
    _chk(frames, torch.uint8, 'frames'); _chk(out, torch.float32, 'out')
    if frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise lib.MoviigenHipError(f'frames must be a contiguous uint8 [T, H0, W0, 3] tensor, got {tuple(frames.shape)}')
    T, H0, W0, _ = frames.shape
    if out is None:
        out = torch.empty(3, T, int(H), int(W), dtype=torch.float32, device=frames.device)
    elif tuple(out.shape) != (3, T, int(H), int(W)) or not out.is_contiguous():
        raise lib.MoviigenHipError(f'video_from_u8: out must be a contiguous {(3, T, int(H), int(W))} tensor, got {tuple(out.shape)}')
    lib.call('mg_video_from_u8', _p(frames), T, H0, W0, int(H), int(W), _p(out), _st())
    return out


def mask_from_u8(mask, T, H, W, keep_frames=0, out=None):
    """uint8 mask [Tm,H0,W0] (Tm == 1 or >= T; >= 128 after the resize = regenerate) -> the pixel mask [T,H,W] uint8 0/1 through the geometry and
    filter of video_from_u8; frames below keep_frames are 0 = kept (mg_mask_from_u8; the definition is in include/moviigen_hip.h)."""
    _chk(mask, torch.uint8, 'mask'); _chk(out, torch.uint8, 'out')
    if mask.dim() != 3 or not mask.is_contiguous():
        raise lib.MoviigenHipError(f'mask must be a contiguous uint8 [Tm, H0, W0] tensor, got {tuple(mask.shape)}')
    Tm, H0, W0 = mask.shape
    if out is None:
        out = torch.empty(int(T), int(H), int(W), dtype=torch.uint8, device=mask.device)
    elif tuple(out.shape) != (int(T), int(H), int(W)) or not out.is_contiguous():
        raise lib.MoviigenHipError(f'mask_from_u8: out must be a contiguous {(int(T), int(H), int(W))} tensor, got {tuple(out.shape)}')
    lib.call('mg_mask_from_u8', _p(mask), Tm, H0, W0, int(T), int(H), int(W), int(keep_frames), _p(out), _st())
    return out


def mask_to_latent(pm, stride):
    """pixel mask [T,H,W] uint8 -> the latent-grid mask [(T-1)/st+1, H/sh, W/sw] uint8 0/1 of a causal VAE with `stride` = (st, sh, sw): the OR
    over every pixel under a latent cell (mg_mask_to_latent_u8)."""
    _chk(pm, torch.uint8, 'pm')
    if pm.dim() != 3 or not pm.is_contiguous():
        raise lib.MoviigenHipError(f'pm must be a contiguous uint8 [T, H, W] tensor, got {tuple(pm.shape)}')
    T, H, W = pm.shape
    st, sh, sw = (int(v) for v in stride)
    if min(st, sh, sw) <= 0:
        raise lib.MoviigenHipError(f'mask_to_latent: stride must be positive, got {(st, sh, sw)}')
    lm = torch.empty((T - 1) // st + 1, H // sh, W // sw, dtype=torch.uint8, device=pm.device)
    lib.call('mg_mask_to_latent_u8', _p(pm), T, H, W, st, sh, sw, _p(lm), _st())
    return lm


def masked_renoise(latent, z0, noise, lm, c0, c1):
    """latent [C, ...] fp32 IN PLACE: c0 z0 + c1 noise (the bits of lincomb) where lm [...] uint8 is 0, untouched where it is not
    (mg_masked_renoise_f32)."""
    for n, t in (('latent', latent), ('z0', z0), ('noise', noise)):
        _chk(t, torch.float32, n)
    _chk(lm, torch.uint8, 'lm')
    if not (latent.is_contiguous() and z0.is_contiguous() and noise.is_contiguous() and lm.is_contiguous()) or latent.dim() < 2 \
            or z0.shape != latent.shape or noise.shape != latent.shape or lm.numel() * latent.shape[0] != latent.numel():
        raise lib.MoviigenHipError(f'masked_renoise: latent {tuple(latent.shape)}, z0 {tuple(z0.shape)}, noise {tuple(noise.shape)}, lm {tuple(lm.shape)}')
    lib.call('mg_masked_renoise_f32', _p(latent), _p(z0), _p(noise), _p(lm), float(c0), float(c1), latent.shape[0], lm.numel(), _st())
    return latent


def mask_composite(video, src, pm):
    """video [3,T,H,W] fp32 IN PLACE: src where pm [T,H,W] uint8 is 0, untouched where it is not (mg_mask_composite_f32)."""
    _chk(video, torch.float32, 'video'); _chk(src, torch.float32, 'src'); _chk(pm, torch.uint8, 'pm')
    if video.dim() != 4 or video.shape[0] != 3 or src.shape != video.shape or tuple(pm.shape) != tuple(video.shape[1:]) \
            or not (video.is_contiguous() and src.is_contiguous() and pm.is_contiguous()):
        raise lib.MoviigenHipError(f'mask_composite: video {tuple(video.shape)}, src {tuple(src.shape)}, pm {tuple(pm.shape)}')
    T = video.shape[1]
    lib.call('mg_mask_composite_f32', _p(video), _p(src), _p(pm), T, video.shape[2] * video.shape[3], _st())
    return video


def _window_dims(name, whole, win, f0):
    """(C, F, hw, Fw) of a whole clip [C, F, ...] and one window [C, Fw, ...] of it at frames [f0, f0 + Fw), both dense fp32"""
    _chk_flat(whole, torch.float32, name[0]); _chk_flat(win, torch.float32, name[1])
    if whole.dim() < 2 or win.dim() != whole.dim() or win.shape[0] != whole.shape[0] or tuple(win.shape[2:]) != tuple(whole.shape[2:]) \
            or min(whole.shape) < 1 or win.shape[1] < 1 or not 0 <= int(f0) <= whole.shape[1] - win.shape[1]:
        raise lib.MoviigenHipError(f'{name[0]} {tuple(whole.shape)} and {name[1]} {tuple(win.shape)} must be [C, F, ...] and [C, Fw, ...] with '
                                   f'0 <= f0 <= F - Fw, f0 = {f0}')
    C, F, Fw = whole.shape[0], whole.shape[1], win.shape[1]
    return C, F, whole.numel() // (C * F), Fw


def window_gather(x, f0, out):
    """out [C, Fw, ...] <- x[:, f0:f0 + Fw] of the dense fp32 clip x [C, F, ...]: a copy, the bits are unchanged (mg_window_gather_f32)."""
    C, F, hw, Fw = _window_dims(('x', 'out'), x, out, f0)
    lib.call('mg_window_gather_f32', _p(x), C, F, hw, int(f0), Fw, _p(out), _st())
    return out


def window_blend(acc, pred, f0, w, first):
    """acc [C, F, ...] fp32 IN PLACE at frames [f0, f0 + Fw), from the window's prediction pred [C, Fw, ...]: w[j] * pred where first[j]
    is non-zero (a select: acc is not read there and needs no initial value), fma(w[j], pred, acc) where it is zero.  w fp32 [Fw] and
    first uint8 [Fw] live on the device; frames outside the window are not touched (mg_window_blend_f32)."""
    C, F, hw, Fw = _window_dims(('acc', 'pred'), acc, pred, f0)
    _chk_flat(w, torch.float32, 'w'); _chk_flat(first, torch.uint8, 'first')
    if tuple(w.shape) != (Fw,) or tuple(first.shape) != (Fw,):
        raise lib.MoviigenHipError(f'window_blend: w and first must be [{Fw}], got {tuple(w.shape)}, {tuple(first.shape)}')
    lib.call('mg_window_blend_f32', _p(acc), _p(pred), C, F, hw, int(f0), Fw, _p(w), _p(first), _st())
    return acc


def gate_residual(x, y, gate=None):
    """x [rows, dim] fp32 += y [rows, dim] bf16 * gate [dim] fp32 (None = 1)."""
    _chk(x, torch.float32, 'x'); _chk(y, torch.bfloat16, 'y'); _chk(gate, torch.float32, 'gate')
    if x.shape != y.shape:
        raise lib.MoviigenHipError(f'gate_residual shape mismatch x{tuple(x.shape)} y{tuple(y.shape)}')
    lib.call('mg_gate_residual_f32', _p(x), x.stride(0), _p(y), y.stride(0), _p(gate), x.shape[0], x.shape[1], _st())
    return x


def _sp_chk_cols(what, P, cols, col0, w):
    if P < 1 or w < 1 or w % 8 or col0 < 0 or col0 % 8 or cols % 8 or col0 + w > cols:
        raise lib.MoviigenHipError(f'{what}: columns [{col0}, {col0} + {w}) of {P} blocks of {cols} — all multiples of 8 (16-byte vectors), '
                                   'inside the block')


def sp_pack_qkv(q, k, v, P, cols_per_dest, col0, w, send):
    """q, k, v [Lloc, >= P*cols_per_dest] bf16 (column slices ok) -> send [P, Lloc, 3w] (see moviigen_hip.h)."""
    for n, t in (('q', q), ('k', k), ('v', v)):
        _chk_rows(t, torch.bfloat16, n)
    _chk_flat(send, torch.bfloat16, 'send')
    P, cols_per_dest, col0, w = int(P), int(cols_per_dest), int(col0), int(w)
    _sp_chk_cols('sp_pack_qkv', P, cols_per_dest, col0, w)
    Lloc = q.shape[0]
    if k.shape[0] != Lloc or v.shape[0] != Lloc or min(q.shape[1], k.shape[1], v.shape[1]) < P * cols_per_dest:
        raise lib.MoviigenHipError(f'sp_pack_qkv: q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} must have one row count and >= '
                                   f'{P} x {cols_per_dest} columns')
    if send.numel() < P * Lloc * 3 * w:
        raise lib.MoviigenHipError(f'sp_pack_qkv: send {tuple(send.shape)} is smaller than [{P}, {Lloc}, {3 * w}]')
    lib.call('mg_sp_pack_qkv_bf16', _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), Lloc, P, cols_per_dest, col0, w,
             _p(send), _st())
    return send


def sp_unpack_o(recv, P, cols_per_src, col0, w, o):
    """recv [P, Lloc, w] bf16 -> o[:, p*cols_per_src + col0 : +w] for every source rank p."""
    _chk_flat(recv, torch.bfloat16, 'recv'); _chk_rows(o, torch.bfloat16, 'o')
    P, cols_per_src, col0, w = int(P), int(cols_per_src), int(col0), int(w)
    _sp_chk_cols('sp_unpack_o', P, cols_per_src, col0, w)
    Lloc = o.shape[0]
    if o.shape[1] < P * cols_per_src:
        raise lib.MoviigenHipError(f'sp_unpack_o: o {tuple(o.shape)} is narrower than {P} x {cols_per_src} columns')
    if recv.numel() < P * Lloc * w:
        raise lib.MoviigenHipError(f'sp_unpack_o: recv {tuple(recv.shape)} is smaller than [{P}, {Lloc}, {w}]')
    lib.call('mg_sp_unpack_o_bf16', _p(recv), Lloc, P, cols_per_src, col0, w, _p(o), o.stride(0), _st())
    return o


def sp_copy_blocks(src, s_blk, s_row, dst, d_blk, d_row, blocks, rows, width):
    """dst[b][r][:width] = src[b][r][:width] with element strides (*_blk, *_row) from each tensor's first element: the reshapes around an
    all-to-all.  Every element addressed has to lie inside the tensor's storage."""
    _chk(src, torch.bfloat16, 'src'); _chk(dst, torch.bfloat16, 'dst')
    s_blk, s_row, d_blk, d_row, blocks, rows, width = (int(v) for v in (s_blk, s_row, d_blk, d_row, blocks, rows, width))
    if src is None or dst is None or blocks < 0 or rows < 0 or width < 1 or width % 8 or min(s_blk, s_row, d_blk, d_row) < 0:
        raise lib.MoviigenHipError(f'sp_copy_blocks: {blocks} blocks of {rows} rows of {width} (a multiple of 8) with strides '
                                   f'{(s_blk, s_row)} -> {(d_blk, d_row)}')
    for n, t, blk, row in (('src', src, s_blk, s_row), ('dst', dst, d_blk, d_row)):
        last = (blocks - 1) * blk + (rows - 1) * row + width - 1
        if blocks and rows and t.storage_offset() + last >= t.untyped_storage().nbytes() // t.element_size():
            raise lib.MoviigenHipError(f'sp_copy_blocks: element {last} of {n} {tuple(t.shape)} (block {blocks - 1}, row {rows - 1}, column '
                                       f'{width - 1}) lies outside its storage')
    lib.call('mg_sp_copy_blocks_bf16', _p(src), s_blk, s_row, _p(dst), d_blk, d_row, blocks, rows, width, _st())
    return dst


def image_to_u8(image, lo=-1.0, hi=1.0):
    """[3,H,W] fp32 -> uint8 pixels [H,W,3] (reference cache_image / torchvision save_image arithmetic: rounds)."""
    _chk(image, torch.float32, 'image')
    if image.dim() != 3 or image.shape[0] != 3 or not image.is_contiguous():
        raise lib.MoviigenHipError('image must be a contiguous [3, H, W] tensor')
    _, H, W = image.shape
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=image.device)
    lib.call('mg_image_to_u8', _p(image), H, W, float(lo), float(hi), _p(out), _st())
    return out


def attention_merge(acc, lse_acc, part, lse_part, heads, first, out=None):
    """ring attention: fold block result (part bf16, lse_part) into (acc fp32, lse_acc); out = bf16 copy of acc."""
    _chk(acc, torch.float32, 'acc'); _chk(lse_acc, torch.float32, 'lse_acc'); _chk(part, torch.bfloat16, 'part')
    _chk(lse_part, torch.float32, 'lse_part'); _chk(out, torch.bfloat16, 'out')
    lib.call('mg_attn_merge_f32', _p(acc), acc.stride(0), _p(lse_acc), _p(part), part.stride(0), _p(lse_part), _p(out),
             out.stride(0) if out is not None else 0, acc.shape[0], int(heads), int(bool(first)), _st())
    return acc
