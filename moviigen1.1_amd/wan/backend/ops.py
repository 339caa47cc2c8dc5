"""Typed wrappers: torch CUDA tensors in, C-ABI kernel launches out (on torch's current stream); every arithmetic step is a libmoviigen_hip.so kernel.
ops.py checks what the C ABI cannot see: device, dtype, None against required, and that each tensor's memory holds the extent its pointer, stride and counts claim.
The library checks what it is given (MG_ERR_ARG / MG_ERR_SHAPE): alignment, divisibility, ranges of scalars, unsupported sizes.  A failure raises; nothing falls back."""
import ctypes

import torch

from . import lib

BIAS_BF16, BIAS_GELU_BF16, GATE_RESID_F32, BIAS_F32 = 0, 1, 2, 3
F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _epilogue_dtype(epilogue):
    """what a GEMM epilogue writes (MG_EPI_* in include/moviigen_hip.h): bf16 behind bias / bias+GELU, fp32 otherwise"""
    return BF16 if epilogue in (BIAS_BF16, BIAS_GELU_BF16) else F32


# ---- the argument-check vocabulary: every message is built in _fail and begins with the wrapper's name ----
def _fail(op, msg):
    raise lib.MoviigenHipError(f'{op}: {msg}')


def _tensor(op, name, t, dtype, optional=False):
    """device, dtype (one, or a tuple of allowed ones), innermost stride 1; None passes only when optional -> t"""
    if t is None:
        return None if optional else _fail(op, f'{name}: expected a tensor, got None')
    if not torch.is_tensor(t) or not t.is_cuda:
        _fail(op, f'{name}: expected a CUDA (HIP) tensor — the hot path has no CPU fallback')
    if t.dtype != dtype and not (isinstance(dtype, tuple) and t.dtype in dtype):
        _fail(op, f'{name}: expected {dtype}, got {t.dtype}')
    if t.dim() >= 1 and t.stride(-1) != 1:
        _fail(op, f'{name}: innermost dimension must be contiguous')
    return t


def _dense(op, name, t, dtype, shape=None, numel=None, min_numel=None, optional=False):
    """a tensor its kernel reads or writes flat: _tensor, dense row-major, and the exact shape / element count / least element count given"""
    if _tensor(op, name, t, dtype, optional) is None:
        return None
    if not t.is_contiguous():
        _fail(op, f'{name}: must be contiguous, got shape {tuple(t.shape)} with strides {tuple(t.stride())}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        _fail(op, f'{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}')
    if (numel is not None and t.numel() != numel) or (min_numel is not None and t.numel() < min_numel):
        _fail(op, f'{name}: expected {numel if min_numel is None else f"at least {min_numel}"} elements, got {t.numel()} in shape {tuple(t.shape)}')
    return t


def _rows(op, name, t, dtype, rows=None, cols=None, min_rows=None, min_cols=None, optional=False):
    """a [rows, cols] tensor whose row stride goes to the kernel: _tensor, two dimensions, rows that do not overlap, the extents given"""
    if _tensor(op, name, t, dtype, optional) is None:
        return None
    if t.dim() != 2 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        _fail(op, f'{name}: expected [rows, cols] with a row stride >= cols, got shape {tuple(t.shape)} with strides {tuple(t.stride())}')
    r, c = t.shape
    if (rows is not None and r != rows) or (cols is not None and c != cols):
        _fail(op, f'{name}: expected shape ({r if rows is None else rows}, {c if cols is None else cols}), got {tuple(t.shape)}')
    if (min_rows is not None and r < min_rows) or (min_cols is not None and c < min_cols):
        _fail(op, f'{name}: expected at least [{min_rows or 0}, {min_cols or 0}], got {tuple(t.shape)}')
    return t


def ln_modulate(x, scale, shift, add_one, eps, out, round_norm_bf16=False):
    """x [rows, dim] fp32 -> out [rows, dim] (bf16 or fp32)."""
    op = 'ln_modulate'
    rows, dim = _rows(op, 'x', x, F32).shape
    _rows(op, 'out', out, (BF16, F32), rows=rows, cols=dim)
    _dense(op, 'scale', scale, F32, numel=dim, optional=True); _dense(op, 'shift', shift, F32, numel=dim, optional=True)
    lib.call('mg_ln_modulate', _p(x), x.stride(0), rows, dim, _p(scale), _p(shift), int(add_one), float(eps),
             int(round_norm_bf16), _p(out), int(out.dtype == F32), out.stride(0), _st())
    return out


def resid_ln_modulate(x, r, scale, shift, eps, out):
    """out [rows, dim] fp32 = LN(x + r) * (1 + scale) + shift, x and r [rows, dim] fp32 (row strides free), only read: the bits of
    ln_modulate(lincomb(x, r), scale, shift, True, eps, out) in one pass (the step cache's skipped step)."""
    op = 'resid_ln_modulate'
    rows, dim = _rows(op, 'x', x, F32).shape
    _rows(op, 'r', r, F32, rows=rows, cols=dim); _rows(op, 'out', out, F32, rows=rows, cols=dim)
    _dense(op, 'scale', scale, F32, numel=dim, optional=True); _dense(op, 'shift', shift, F32, numel=dim, optional=True)
    lib.call('mg_resid_ln_modulate_f32', _p(x), x.stride(0), _p(r), r.stride(0), rows, dim, _p(scale), _p(shift), float(eps), _p(out),
             out.stride(0), _st())
    return out


def step_resid_partials(device):
    """the caller-owned scratch of step_resid_capture(stats=...): mg_step_resid_partials_bytes() bytes as fp64, no initial value needed"""
    return torch.empty(int(lib.load().mg_step_resid_partials_bytes()) // 8, dtype=torch.float64, device=device)


def step_resid_capture(r, x, xin, stats=None, partials=None):
    """r <- x - xin (contiguous fp32 tensors of equal size, r IN PLACE).  stats: fp64 [2] receiving (sum |r_new - r_old|, sum |r_old|),
    r_old = what r held — deterministic (fixed grid, fixed order); it needs `partials` (step_resid_partials).  None: no reduction."""
    op = 'step_resid_capture'
    n = _dense(op, 'r', r, F32).numel()
    _dense(op, 'x', x, F32, numel=n); _dense(op, 'xin', xin, F32, numel=n)
    if stats is not None:
        _dense(op, 'stats', stats, torch.float64, min_numel=2)
        _dense(op, 'partials', partials, torch.float64, min_numel=int(lib.load().mg_step_resid_partials_bytes()) // 8)
    lib.call('mg_step_resid_capture_f32', _p(r), _p(x), _p(xin), n, _p(stats), _p(partials) if stats is not None else None, _st())
    return r


ATTN_LOG2E = 1.4426950408889634


def rmsnorm_rope(x, weight, eps, head_dim, out, rope_cs=None, grid=(1, 1, 1), pos0=0, out_scale=1.0):
    """x [rows, dim] bf16 (may be a strided column slice) -> out bf16.  out_scale: factor applied before the one
    rounding to bf16 (the attention's scale*log2(e) for a q that goes to attention_hd128(..., prescaled=True)).
    rope_cs: None, or the table of rope_cos_sin(head_dim, grid) — the kernel indexes it by `grid`."""
    op = 'rmsnorm_rope'
    rows, dim = _rows(op, 'x', x, BF16).shape
    _rows(op, 'out', out, BF16, rows=rows, cols=dim)
    _dense(op, 'weight', weight, F32, numel=dim)
    F, H, W = (int(g) for g in grid)
    if rope_cs is not None:
        c = int(head_dim) // 2
        c1 = c // 3
        _dense(op, 'rope_cs', rope_cs, F32, numel=2 * (F * (c - 2 * c1) + (H + W) * c1))
    lib.call('mg_rmsnorm_rope_bf16', _p(x), x.stride(0), _p(out), out.stride(0), rows, dim, _p(weight), float(eps),
             int(head_dim), _p(rope_cs), F, H, W, int(pos0), float(out_scale), _st())
    return out


def packed_kv_numel(L, heads):
    """elements of one packed K (or V) buffer for L keys: heads * ceil(L/64) tiles of 8192."""
    return heads * ((L + 63) // 64) * 8192


def pack_kv(k, v, heads, kp, vp):
    """k, v [L, heads*128] bf16 (strided column slices ok; either may be None) -> packed 64-key tiles
    kp / vp (flat bf16 buffers of packed_kv_numel elements) for attention_hd128."""
    op = 'pack_kv'
    L = None
    for name, t in (('k', k), ('v', v)):
        if _rows(op, name, t, BF16, rows=L, min_cols=int(heads) * 128, optional=True) is not None:
            L = t.shape[0]
    if L is None:
        _fail(op, 'k and v are both None')
    _dense(op, 'kp', kp, BF16, min_numel=packed_kv_numel(L, heads) if k is not None else None, optional=k is None)
    _dense(op, 'vp', vp, BF16, min_numel=packed_kv_numel(L, heads) if v is not None else None, optional=v is None)
    lib.call('mg_pack_kv_bf16', _p(k), 0 if k is None else k.stride(0), _p(v), 0 if v is None else v.stride(0), L,
             int(heads), 128, _p(kp), _p(vp), _st())


def gemm(a, w, bias, epilogue, out, gate=None):
    """out[M,N] (+)= a[M,K] @ w[N,K]^T (+bias ...) — see MG_EPI_* in include/moviigen_hip.h."""
    op = 'gemm'
    M, K = _rows(op, 'a', a, BF16).shape
    N = _rows(op, 'w', w, BF16, cols=K).shape[0]
    _rows(op, 'out', out, _epilogue_dtype(epilogue), rows=M, cols=N)
    _dense(op, 'bias', bias, F32, numel=N, optional=True); _dense(op, 'gate', gate, F32, numel=N, optional=True)
    lib.call('mg_gemm_bf16', _p(a), a.stride(0), _p(w), w.stride(0), _p(bias), M, N, K, int(epilogue), _p(out),
             out.stride(0), _p(gate), _st())
    return out


def quant_mxfp8(x, q=None, scales=None):
    """x [rows, K] bf16 (row stride free) -> (q uint8 [rows, K] e4m3fn bytes, scales uint8 [rows, K/32] E8M0 bytes): OCP MXFP8
    with the project's saturating definition (include/moviigen_hip.h).  q / scales are allocated when not given."""
    op = 'quant_mxfp8'
    rows, K = _rows(op, 'x', x, BF16).shape
    if q is None:
        q = torch.empty(rows, K, dtype=U8, device=x.device)
    if scales is None:
        scales = torch.empty(rows, K // 32, dtype=U8, device=x.device)
    _rows(op, 'q', q, U8, rows=rows, cols=K); _rows(op, 'scales', scales, U8, rows=rows, cols=K // 32)
    lib.call('mg_quant_mxfp8_rows', _p(x), x.stride(0), rows, K, _p(q), q.stride(0), _p(scales), scales.stride(0), _st())
    return q, scales


def _mxfp8_operands(op, aq, a_scales, wq, w_scales, bias):
    """the operands the MXFP8 GEMMs share: bytes [M, K] and [N, K], scale bytes [M, K/32] and [N, K/32], bias of N floats -> (M, N, K)"""
    M, K = _rows(op, 'aq', aq, U8).shape
    N = _rows(op, 'wq', wq, U8, cols=K).shape[0]
    _rows(op, 'a_scales', a_scales, U8, rows=M, cols=K // 32); _rows(op, 'w_scales', w_scales, U8, rows=N, cols=K // 32)
    _dense(op, 'bias', bias, F32, numel=N, optional=True)
    return M, N, K


def gemm_mxfp8(aq, a_scales, wq, w_scales, bias, epilogue, out, gate=None):
    """out[M,N] (+)= dequant(aq, a_scales)[M,K] @ dequant(wq, w_scales)[N,K]^T (+bias ...) on the block-scaled MFMA; the epilogues
    of `gemm` (MG_EPI_* in include/moviigen_hip.h)."""
    op = 'gemm_mxfp8'
    M, N, K = _mxfp8_operands(op, aq, a_scales, wq, w_scales, bias)
    _rows(op, 'out', out, _epilogue_dtype(epilogue), rows=M, cols=N)
    _dense(op, 'gate', gate, F32, numel=N, optional=True)
    lib.call('mg_gemm_mxfp8', _p(aq), aq.stride(0), _p(a_scales), a_scales.stride(0), _p(wq), wq.stride(0), _p(w_scales),
             w_scales.stride(0), _p(bias), M, N, K, int(epilogue), _p(out), out.stride(0), _p(gate), _st())
    return out


def ln_modulate_mxfp8(x, scale, shift, add_one, eps, q, scales, out=None, round_norm_bf16=False):
    """ln_modulate (bf16 result) leaving as MXFP8: x [rows, dim] fp32 -> q uint8 [rows, dim] + scales uint8 [rows, dim/32], the bytes
    quant_mxfp8 makes of ln_modulate's bf16 output; `out` (bf16 [rows, dim]) receives that output as well when given."""
    op = 'ln_modulate_mxfp8'
    rows, dim = _rows(op, 'x', x, F32).shape
    _rows(op, 'q', q, U8, rows=rows, cols=dim); _rows(op, 'scales', scales, U8, rows=rows, cols=dim // 32)
    _rows(op, 'out', out, BF16, rows=rows, cols=dim, optional=True)
    _dense(op, 'scale', scale, F32, numel=dim, optional=True); _dense(op, 'shift', shift, F32, numel=dim, optional=True)
    lib.call('mg_ln_modulate_mxfp8', _p(x), x.stride(0), rows, dim, _p(scale), _p(shift), int(add_one), float(eps),
             int(round_norm_bf16), _p(out), 0 if out is None else out.stride(0), _p(q), q.stride(0), _p(scales), scales.stride(0), _st())
    return q, scales


def gemm_mxfp8_gelu_q(aq, a_scales, wq, w_scales, bias, oq, o_scales):
    """gemm_mxfp8 with the BIAS_GELU_BF16 epilogue whose bf16 result leaves as MXFP8: oq uint8 [M, N] + o_scales uint8 [M, N/32], the
    bytes quant_mxfp8 makes of that epilogue's output."""
    op = 'gemm_mxfp8_gelu_q'
    M, N, K = _mxfp8_operands(op, aq, a_scales, wq, w_scales, bias)
    _rows(op, 'oq', oq, U8, rows=M, cols=N); _rows(op, 'o_scales', o_scales, U8, rows=M, cols=N // 32)
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
            ws = torch.zeros(int(lib.load().mg_attn_workspace_bytes()), dtype=U8, device=f'cuda:{dev}')
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
    op = 'attention_hd128'
    lk, heads = int(lk), int(heads)
    Lq = _rows(op, 'q', q, BF16, min_cols=heads * 128).shape[0]
    _rows(op, 'out', out, BF16, min_rows=Lq, min_cols=heads * 128)
    _dense(op, 'kp', kp, BF16, min_numel=packed_kv_numel(lk, heads)); _dense(op, 'vp', vp, BF16, min_numel=packed_kv_numel(lk, heads))
    _dense(op, 'lse', lse, F32, min_numel=heads * Lq, optional=True)
    ws = attention_workspace(q.device) if isinstance(workspace, str) else \
        _dense(op, 'workspace', workspace, U8, min_numel=int(lib.load().mg_attn_workspace_bytes()), optional=True)
    head = (_p(q), q.stride(0), _p(kp), _p(vp), _p(out), out.stride(0))
    if prescaled:
        lib.call('mg_attn_fwd_bf16_hd128_prescaled', *head, _p(lse), Lq, lk, heads, int(reserve_cus), _p(ws), _st())
    elif lse is not None:
        lib.call('mg_attn_fwd_bf16_hd128_lse', *head, _p(lse), Lq, lk, heads, float(scale), _p(ws), _st())
    else:
        lib.call('mg_attn_fwd_bf16_hd128', *head, Lq, lk, heads, float(scale), _p(ws), _st())
    return out


_attention_hd128 = attention_hd128      # the engine's own function, whatever a caller binds to the public name (bench.py times that one)


def attention_hd128_lse(q, kp, vp, out, lse, lk, heads, scale, prescaled=False):
    """attention_hd128(..., lse=lse) -> (out, lse)"""
    return _attention_hd128(q, kp, vp, out, lk, heads, scale, prescaled=prescaled, lse=lse), lse


def attention_generic(q, k, v, out, lk, heads, head_dim, scale):
    """q [Lq, >=heads*head_dim], k and v [>=lk, >=heads*head_dim] row-major bf16 (row strides free) -> out [>=Lq, >=heads*head_dim]."""
    op = 'attention_generic'
    lk, heads, head_dim = int(lk), int(heads), int(head_dim)
    Lq = _rows(op, 'q', q, BF16, min_cols=heads * head_dim).shape[0]
    _rows(op, 'k', k, BF16, min_rows=lk, min_cols=heads * head_dim); _rows(op, 'v', v, BF16, min_rows=lk, min_cols=heads * head_dim)
    _rows(op, 'out', out, BF16, min_rows=Lq, min_cols=heads * head_dim)
    lib.call('mg_attn_fwd_bf16_generic', _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(out),
             out.stride(0), Lq, lk, heads, head_dim, float(scale), _st())
    return out


def sinusoid_embed(t, dim, out):
    """t [n] int64 / fp32 / fp64 positions -> out [n, dim] fp32 = cos(t w_j) | sin(t w_j), w_j = 10000^(-j / (dim/2)), evaluated in fp64."""
    op = 'sinusoid_embed'
    codes = {torch.int64: 0, F32: 1, torch.float64: 2}
    _dense(op, 't', t, tuple(codes))
    dim = int(dim)
    if dim <= 0 or dim % 2:
        _fail(op, f'dim {dim} must be positive and even')
    _dense(op, 'out', out, F32, numel=t.numel() * dim)
    lib.call('mg_sinusoid_embed', _p(t), codes[t.dtype], t.numel(), dim, _p(out), _st())
    return out


def gemv(w, bias, x, y, silu_in=False):
    """y [N] = w [N, K] @ (silu(x) if silu_in else x) [K] + bias [N] (None = 0): dense fp32 tensors, K a multiple of 4."""
    op = 'gemv'
    _dense(op, 'w', w, F32)
    if w.dim() != 2 or w.shape[1] % 4:
        _fail(op, f'w must be [N, K] with K a multiple of 4, got {tuple(w.shape)}')
    N, K = w.shape
    _dense(op, 'bias', bias, F32, numel=N, optional=True); _dense(op, 'x', x, F32, numel=K); _dense(op, 'y', y, F32, numel=N)
    lib.call('mg_gemv_f32', _p(w), _p(bias), _p(x), _p(y), N, K, int(silu_in), _st())
    return y


def add_rows(a, b, out, period):
    """out [rows, dim] = a [rows, dim] + b [>= period, dim] with row r of a meeting row r % period of b: dense fp32 tensors."""
    op = 'add_rows'
    _dense(op, 'a', a, F32); _dense(op, 'b', b, F32); _dense(op, 'out', out, F32, shape=a.shape)
    period = int(period)
    if a.dim() != 2 or b.dim() != 2 or period < 1 or b.shape[0] < period or b.shape[1] != a.shape[1]:
        _fail(op, f'shape mismatch a{tuple(a.shape)} b{tuple(b.shape)} period {period}')
    rows, dim = a.shape
    lib.call('mg_add_rows_f32', _p(a), _p(b), _p(out), rows, dim, period, _st())
    return out


def head_gemm(x, w, bias, out):
    """out [M, N <= 64] = x [M, K] @ w [N, K]^T + bias [N] (None = 0) in fp32: x may be a column slice (row stride free), w and out are dense."""
    op = 'head_gemm'
    M, K = _rows(op, 'x', x, F32).shape
    _dense(op, 'w', w, F32)
    if w.dim() != 2 or w.shape[0] > 64 or w.shape[1] != K:
        _fail(op, f'w must be [N <= 64, {K}], got {tuple(w.shape)}')
    N = w.shape[0]
    _dense(op, 'bias', bias, F32, numel=N, optional=True); _dense(op, 'out', out, F32, shape=(M, N))
    lib.call('mg_head_gemm_f32', _p(x), x.stride(0), _p(w), _p(bias), _p(out), M, N, K, _st())
    return out


def patchify(lat, ph, pw, out):
    """lat [C, F, H, W] fp32 dense -> out [>= F (H/ph) (W/pw), >= C ph pw] bf16 (row stride free): row = patch in (f, h, w) order,
    column = (c, i, j); columns behind C ph pw are not written."""
    op = 'patchify'
    _dense(op, 'lat', lat, F32)
    ph, pw = int(ph), int(pw)
    if lat.dim() != 4 or ph < 1 or pw < 1 or lat.shape[2] % ph or lat.shape[3] % pw:
        _fail(op, f'lat {tuple(lat.shape)} is not [C, F, H, W] with H, W multiples of the patch {(ph, pw)}')
    C, F, H, W = lat.shape
    _rows(op, 'out', out, BF16, min_rows=F * (H // ph) * (W // pw), min_cols=C * ph * pw)
    lib.call('mg_patchify_bf16', _p(lat), C, F, H, W, ph, pw, _p(out), out.stride(0), _st())
    return out


def unpatchify(tok, C, F, Hg, Wg, ph, pw, lat):
    """tok [>= F Hg Wg, >= ph pw C] fp32 (row stride free), column = (i, j, c) -> lat [C, F, Hg ph, Wg pw] fp32 dense."""
    op = 'unpatchify'
    C, F, Hg, Wg, ph, pw = (int(v) for v in (C, F, Hg, Wg, ph, pw))
    if min(C, F, Hg, Wg, ph, pw) < 1:
        _fail(op, f'(C, F, Hg, Wg, ph, pw) = {(C, F, Hg, Wg, ph, pw)} must be positive')
    _rows(op, 'tok', tok, F32, min_rows=F * Hg * Wg, min_cols=ph * pw * C)
    _dense(op, 'lat', lat, F32, numel=C * F * Hg * ph * Wg * pw)
    lib.call('mg_unpatchify_f32', _p(tok), tok.stride(0), C, F, Hg, Wg, ph, pw, _p(lat), _st())
    return lat


def lincomb(out, terms):
    """out = sum(c_i * x_i) for 1 to 4 (tensor, coef) terms: dense fp32 tensors of out's size."""
    op = 'lincomb'
    terms = list(terms)
    _dense(op, 'out', out, F32)
    if not 1 <= len(terms) <= 4:
        _fail(op, f'takes 1 to 4 terms, got {len(terms)}')
    args = []
    for i, (x, c) in enumerate(terms):
        _dense(op, f'x{i}', x, F32, numel=out.numel())
        args += [_p(x), float(c)]
    args += [None, 0.0] * (4 - len(terms))
    lib.call('mg_lincomb4_f32', _p(out), out.numel(), *args, _st())
    return out


def lora_merge(w, up, down):
    """w [N, K] bf16 or fp32, IN PLACE: w <- round(w + up [N, R] fp32 @ down [R, K] fp32), fp32 products and sums, one rounding for
    bf16 storage (include/moviigen_hip.h).  w may be a row slice or a column view of a larger matrix (row stride free, a multiple of
    16 bytes): nothing outside [N, K] is written."""
    op = 'lora_merge'
    _tensor(op, 'w', w, (BF16, F32)); _tensor(op, 'up', up, F32); _tensor(op, 'down', down, F32)
    if w.dim() != 2 or up.dim() != 2 or down.dim() != 2 or up.shape[0] != w.shape[0] or down.shape[1] != w.shape[1] \
            or up.shape[1] != down.shape[0]:
        _fail(op, f'shape mismatch w{tuple(w.shape)} up{tuple(up.shape)} down{tuple(down.shape)}')
    N, K = w.shape
    lib.call('mg_lora_merge', _p(w), int(w.dtype == F32), w.stride(0), N, K, _p(up), up.stride(0), _p(down),
             down.stride(0), up.shape[1], _st())
    return w


def cfg_combine(out, uncond, cond, g):
    """out = uncond + g * (cond - uncond): dense fp32 tensors of one size."""
    op = 'cfg_combine'
    n = _dense(op, 'out', out, F32).numel()
    _dense(op, 'uncond', uncond, F32, numel=n); _dense(op, 'cond', cond, F32, numel=n)
    lib.call('mg_cfg_combine_f32', _p(out), _p(uncond), _p(cond), float(g), n, _st())
    return out


def cfg_stats_partials(device):
    """the caller-owned scratch of cfg_stats: mg_cfg_stats_partials_bytes() bytes as fp64, no initial value needed"""
    return torch.empty(int(lib.load().mg_cfg_stats_partials_bytes()) // 8, dtype=torch.float64, device=device)


def _aligned16(op, **tensors):
    for name, t in tensors.items():
        if t.data_ptr() % 16:
            _fail(op, f'{name}: must be 16-byte aligned (a view that starts inside a row is not)')


def cfg_stats(uncond, cond, stats, partials):
    """stats fp64 [5] <- (sum u, sum c, sum u^2, sum c^2, sum u c) over the dense fp32 tensors uncond (u) and cond (c) of one size:
    fp64 products and sums in a fixed order (the same inputs give the same 40 bytes), no host read; partials: cfg_stats_partials(device).
    The inputs are only read.  DESIGN.md 3.8."""
    op = 'cfg_stats'
    n = _dense(op, 'uncond', uncond, F32).numel()
    _dense(op, 'cond', cond, F32, numel=n)
    if n < 1:
        _fail(op, 'uncond and cond need at least one element')
    _dense(op, 'stats', stats, torch.float64, numel=5)
    _dense(op, 'partials', partials, torch.float64, min_numel=int(lib.load().mg_cfg_stats_partials_bytes()) // 8)
    _aligned16(op, uncond=uncond, cond=cond)
    lib.call('mg_cfg_stats_f32', _p(uncond), _p(cond), n, _p(stats), _p(partials), _st())
    return stats


def cfg_coefficients(stats, n, g, zero_star, rescale, coef):
    """coef fp32 [2] <- (a_u, a_c) of the guided prediction a_u u + a_c c from cfg_stats' sums over n elements: guide scale g, CFG-Zero*'s
    projection when zero_star, guidance rescale by `rescale` in [0, 1] (0 = off) — on the device, in fp64 (include/moviigen_hip.h)."""
    op = 'cfg_coefficients'
    _dense(op, 'stats', stats, torch.float64, numel=5); _dense(op, 'coef', coef, F32, numel=2)
    g, rescale = float(g), float(rescale)
    if int(n) < 1 or g != g or abs(g) == float('inf') or not 0.0 <= rescale <= 1.0:
        _fail(op, f'n >= 1, g finite and rescale in [0, 1]; got {n}, {g}, {rescale}')
    lib.call('mg_cfg_coef_f32', _p(stats), int(n), g, int(bool(zero_star)), rescale, _p(coef), _st())
    return coef


def cfg_combine_coef(out, uncond, cond, coef):
    """out = a_u * uncond + a_c * cond with (a_u, a_c) = coef fp32 [2] ON THE DEVICE (cfg_coefficients): the bits of
    lincomb(out, [(uncond, a_u), (cond, a_c)]).  Dense fp32 tensors of one size; out may be uncond or cond."""
    op = 'cfg_combine_coef'
    n = _dense(op, 'out', out, F32).numel()
    _dense(op, 'uncond', uncond, F32, numel=n); _dense(op, 'cond', cond, F32, numel=n); _dense(op, 'coef', coef, F32, numel=2)
    _aligned16(op, out=out, uncond=uncond, cond=cond)
    lib.call('mg_cfg_combine_coef_f32', _p(out), _p(uncond), _p(cond), n, _p(coef), _st())
    return out


def nag_combine(zp, zn, out, scale, tau, alpha):
    """out [rows, dim] bf16 <- the normalized-attention-guidance mix of the cross-attention outputs zp (positive prompt) and zn (negative
    prompt), per row: g = scale zp - (scale - 1) zn, clipped to tau times zp's L1 norm, blended with zp by alpha (include/moviigen_hip.h,
    DESIGN.md 3.11).  Row strides are free (multiples of 8); out may be zp itself, not zn.  1 <= scale <= 64, tau >= 1, 0 <= alpha <= 1."""
    op = 'nag_combine'
    rows, dim = _rows(op, 'zp', zp, BF16).shape
    _rows(op, 'zn', zn, BF16, rows=rows, cols=dim); _rows(op, 'out', out, BF16, rows=rows, cols=dim)
    if dim < 8 or dim % 8 or dim > 8192:
        _fail(op, f'dim must be a multiple of 8 in [8, 8192], got {dim}')
    for name, t in (('zp', zp), ('zn', zn), ('out', out)):
        if t.stride(0) % 8 or (rows == 1 and t.stride(0) < dim):
            _fail(op, f'{name} needs a row stride that is a multiple of 8 and >= dim, got {t.stride(0)}')
    _aligned16(op, zp=zp, zn=zn, out=out)
    scale, tau, alpha = float(scale), float(tau), float(alpha)
    if not (1.0 <= scale <= 64.0 and 1.0 <= tau < float('inf') and 0.0 <= alpha <= 1.0):
        _fail(op, f'1 <= scale <= 64, 1 <= tau < inf, 0 <= alpha <= 1; got {scale}, {tau}, {alpha}')
    if rows == 0:
        return out
    lib.call('mg_nag_combine_bf16', _p(zp), zp.stride(0), _p(zn), zn.stride(0), _p(out), out.stride(0), rows, dim, scale, tau, alpha, _st())
    return out


# ---- umT5 encoder glue ---------------------------------------------------------------------------
def embed_rows(table, ids, out):
    """out [n, dim] = table [vocab, dim][ids [n]] (ids clamped to the table): dense bf16 / int64 tensors, dim a multiple of 8."""
    op = 'embed_rows'
    _dense(op, 'table', table, BF16); _dense(op, 'ids', ids, torch.int64)
    if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] % 8:
        _fail(op, f'table must be [vocab >= 1, dim a multiple of 8], got {tuple(table.shape)}')
    _dense(op, 'out', out, BF16, shape=(ids.numel(), table.shape[1]))
    lib.call('mg_embed_rows_bf16', _p(table), table.shape[0], table.shape[1], _p(ids), ids.numel(), _p(out), _st())
    return out


def ew_bf16(a, b, out, mode):
    """mode 0: a + b; mode 1: a * gelu_tanh(b) — contiguous bf16 tensors of equal size."""
    op = 'ew_bf16'
    n = _dense(op, 'out', out, BF16).numel()
    _dense(op, 'a', a, BF16, numel=n); _dense(op, 'b', b, BF16, numel=n)
    if int(mode) not in (0, 1):
        _fail(op, f'mode must be 0 (a + b) or 1 (a * gelu_tanh(b)), got {mode}')
    lib.call('mg_ew_bf16', _p(a), _p(b), _p(out), n, int(mode), _st())
    return out


def t5_attention(q, k, v, rel_emb, rel_bucket, out, lk, heads, head_dim):
    """q, k, v: column slices of one [L, 3*heads*head_dim] buffer (same row stride)."""
    op = 't5_attention'
    lk, heads, head_dim = int(lk), int(heads), int(head_dim)
    Lq = _rows(op, 'q', q, BF16).shape[0]
    _rows(op, 'k', k, BF16, min_rows=lk); _rows(op, 'v', v, BF16, min_rows=lk)
    _tensor(op, 'rel_emb', rel_emb, BF16); _tensor(op, 'rel_bucket', rel_bucket, torch.int32)
    _rows(op, 'out', out, BF16, min_rows=Lq, min_cols=heads * head_dim)
    if not (q.stride(0) == k.stride(0) == v.stride(0)):
        _fail(op, 'q, k, v must share a row stride')
    if rel_bucket.numel() != Lq + lk - 1:
        _fail(op, 'rel_bucket must have Lq + Lk - 1 entries')
    lib.call('mg_t5_attn_bf16', _p(q), _p(k), _p(v), q.stride(0), _p(rel_emb), _p(rel_bucket), _p(out), out.stride(0),
             Lq, lk, heads, head_dim, _st())
    return out


# ---- VAE (fp32, channels-last) -------------------------------------------------------------------
VAE_EXACT, VAE_BF16X3 = 0, 1     # MG_VAE_EXACT / MG_VAE_BF16X3 (include/moviigen_hip.h): the arithmetic of one convolution call


def _vae_conv_geometry(op, x, w, bias, cache, kernel):
    """the operands every VAE convolution shares: x [T,H,W,Cin] dense; w dense, [Cout,kt,kh,kw,Cin] for kernel = (kt, kh, kw) or the folded
    [4,Cout,2,2,Cin] for kernel = 'phases'; bias of Cout floats; cache dense, at most kt - 1 frames of x's geometry.
    -> (T, H, W, Cin, Cout, tc)"""
    _dense(op, 'x', x, F32); _dense(op, 'w', w, F32)
    if x.dim() != 4 or w.dim() != 5:
        _fail(op, f'x must be [T, H, W, Cin] and w have five dimensions, got {tuple(x.shape)} and {tuple(w.shape)}')
    T, H, W, Cin = x.shape
    if kernel == 'phases':
        Cout, kt = w.shape[1], 1
        want = (4, Cout, 2, 2, Cin)
    else:
        Cout, kt = w.shape[0], kernel[0]
        want = (Cout, *kernel, Cin)
    if tuple(w.shape) != want:
        _fail(op, f'w must be {want} for x {tuple(x.shape)}, got {tuple(w.shape)}')
    if Cout > 4 and Cout % 4:
        _fail(op, f'Cout = {Cout}: more than 4 output channels have to be a multiple of 4 (the rows of out and residual move as float4)')
    _dense(op, 'bias', bias, F32, numel=Cout, optional=True)
    tc = 0
    if _dense(op, 'cache', cache, F32, optional=True) is not None:
        if cache.dim() != 4 or tuple(cache.shape[1:]) != (H, W, Cin) or cache.shape[0] > kt - 1:
            _fail(op, f'the cache must be at most {kt - 1} frames with the frame geometry of x {tuple(x.shape)}, got {tuple(cache.shape)}')
        tc = cache.shape[0]
    return T, H, W, Cin, Cout, tc


def vae_conv(x, w, bias, out, kt, kh, kw, cache=None, up2=False, residual=None, mode=VAE_EXACT):
    """x [T,H,W,Cin]; w [Cout,kt,kh,kw,Cin]; out [T,Ho,Wo,Cout]."""
    op = 'vae_conv'
    kt, kh, kw = int(kt), int(kh), int(kw)
    T, H, W, Cin, Cout, tc = _vae_conv_geometry(op, x, w, bias, cache, (kt, kh, kw))
    want = (T, 2 * H, 2 * W, Cout) if up2 else (T, H, W, Cout)
    _dense(op, 'out', out, F32, shape=want); _dense(op, 'residual', residual, F32, shape=want, optional=True)
    lib.call('mg_vae_conv_f32', _p(x), _p(cache), tc, T, H, W, Cin, _p(w), _p(bias), Cout, kt, kh, kw,
             int(up2), _p(residual), _p(out), int(mode), _st())
    return out


def vae_conv_cols(x, w, bias, out, kt, kh, kw, col0, cache=None, residual=None, mode=VAE_EXACT):
    """the W-band form: x [T,H,W,Cin] and cache carry the neighbours' halo columns; out (and residual) [T,H,cols,Cout] compact =
    the output columns [col0, col0 + cols) of vae_conv on the whole image."""
    op = 'vae_conv_cols'
    kt, kh, kw, col0 = int(kt), int(kh), int(kw), int(col0)
    T, H, W, Cin, Cout, tc = _vae_conv_geometry(op, x, w, bias, cache, (kt, kh, kw))
    cols = out.shape[2] if _dense(op, 'out', out, F32).dim() == 4 else 0
    if col0 < 0 or cols < 1 or col0 + cols > W:
        _fail(op, f'columns [{col0}, {col0} + {cols}) of out {tuple(out.shape)} are not inside x {tuple(x.shape)}')
    if tuple(out.shape) != (T, H, cols, Cout):
        _fail(op, f'out: expected shape {(T, H, cols, Cout)}, got {tuple(out.shape)}')
    _dense(op, 'residual', residual, F32, shape=(T, H, cols, Cout), optional=True)
    lib.call('mg_vae_conv_cols_f32', _p(x), _p(cache), tc, T, H, W, Cin, _p(w), _p(bias), Cout, kt, kh, kw,
             _p(residual), _p(out), col0, int(cols), int(mode), _st())
    return out


def vae_upconv_fold_weights(w):
    """w [Cout,1,3,3,Cin] (the conv behind a nearest-2x upsample) -> [4,Cout,2,2,Cin]: one 2x2 kernel per output parity."""
    op = 'vae_upconv_fold_weights'
    _dense(op, 'w', w, F32)
    if w.dim() != 5:
        _fail(op, f'w must be [Cout, 1, 3, 3, Cin], got {tuple(w.shape)}')
    Cout, kt, kh, kw, Cin = w.shape
    if (kt, kh, kw) != (1, 3, 3):
        raise ValueError(f'the phase decomposition is defined for 1x3x3 kernels, got {kt}x{kh}x{kw}')
    wp = torch.empty(4, Cout, 2, 2, Cin, dtype=F32, device=w.device)
    lib.call('mg_vae_upconv_fold_weights_f32', _p(w), Cout, Cin, _p(wp), _st())
    return wp


def vae_upconv_phases(x, wp, bias, out, mode=VAE_EXACT):
    """x [T,H,W,Cin]; wp from vae_upconv_fold_weights; out [T,2H,2W,Cout] = conv3x3(nearest-2x(x))."""
    op = 'vae_upconv_phases'
    T, H, W, Cin, Cout, _ = _vae_conv_geometry(op, x, wp, bias, None, 'phases')
    _dense(op, 'out', out, F32, shape=(T, 2 * H, 2 * W, Cout))
    lib.call('mg_vae_upconv_phases_f32', _p(x), T, H, W, Cin, _p(wp), _p(bias), Cout, _p(out), int(mode), _st())
    return out


def vae_upconv_phases_cols(x, wp, bias, out, col0, mode=VAE_EXACT):
    """the W-band form of vae_upconv_phases: x [T,H,W,Cin] with halo columns, out [T,2H,2 cols,Cout] compact."""
    op = 'vae_upconv_phases_cols'
    col0 = int(col0)
    T, H, W, Cin, Cout, _ = _vae_conv_geometry(op, x, wp, bias, None, 'phases')
    cols2 = out.shape[2] if _dense(op, 'out', out, F32).dim() == 4 else 1
    cols = cols2 // 2
    if cols2 % 2 or col0 < 0 or cols < 1 or col0 + cols > W or tuple(out.shape) != (T, 2 * H, 2 * cols, Cout):
        _fail(op, f'out {tuple(out.shape)} is not [{T}, {2 * H}, 2 cols, {Cout}] for columns [{col0}, {col0} + cols) inside x {tuple(x.shape)}')
    lib.call('mg_vae_upconv_phases_cols_f32', _p(x), T, H, W, Cin, _p(wp), _p(bias), Cout, _p(out), col0, cols, int(mode), _st())
    return out


def vae_rmsnorm_silu(x, gamma, out, do_silu=True):
    """x [..., C] -> out of the same shape: x / max(|x|, 1e-12) * sqrt(C) * gamma over the last dimension, then SiLU when do_silu."""
    op = 'vae_rmsnorm_silu'
    _dense(op, 'x', x, F32)
    if x.dim() < 1 or x.shape[-1] < 1:
        _fail(op, f'x must be [..., C], got {tuple(x.shape)}')
    C = x.shape[-1]
    _dense(op, 'gamma', gamma, F32, numel=C); _dense(op, 'out', out, F32, shape=x.shape)
    lib.call('mg_vae_rmsnorm_silu_f32', _p(x), _p(gamma), _p(out), x.numel() // C, C, int(do_silu), _st())
    return out


def vae_attn_workspace_floats(L, C):
    return int(lib.load().mg_vae_attn_workspace_floats(int(L), int(C)))


def vae_attn(qkv, out, workspace):
    """qkv [frames, L, 3C] = q | k | v per pixel, out [frames, L, C] = softmax(q k^T / sqrt(C)) v per frame."""
    op = 'vae_attn'
    _dense(op, 'qkv', qkv, F32)
    if qkv.dim() != 3 or qkv.shape[2] % 3 or qkv.shape[2] == 0:
        _fail(op, f'qkv must be [frames, L, 3C], got {tuple(qkv.shape)}')
    frames, L, C3 = qkv.shape
    C = C3 // 3
    _dense(op, 'out', out, F32, shape=(frames, L, C)); _dense(op, 'workspace', workspace, F32, min_numel=vae_attn_workspace_floats(L, C))
    lib.call('mg_vae_attn_f32', _p(qkv), _p(out), frames, L, C, _p(workspace), _st())
    return out


def vae_attn_rows(q, kv, out, workspace):
    """q [frames, Lq, >= C] (a column slice of the band's q|k|v is fine), kv [frames, Lk, 2C] = k | v of ALL pixels of the frame in image
    order, out [frames, Lq, C]: the band's rows of vae_attn, same bits."""
    op = 'vae_attn_rows'
    _tensor(op, 'q', q, F32); _dense(op, 'kv', kv, F32)
    if q.dim() != 3 or kv.dim() != 3 or kv.shape[2] % 2 or kv.shape[2] == 0:
        _fail(op, f'q must be [frames, Lq, >= C] and kv [frames, Lk, 2C], got {tuple(q.shape)} and {tuple(kv.shape)}')
    frames, Lq = q.shape[:2]
    Lk, C = kv.shape[1], kv.shape[2] // 2
    if Lq > Lk:
        _fail(op, f'Lq = {Lq} query rows exceed the Lk = {Lk} keys: the queries are a subset of the frame\'s pixels')
    if kv.shape[0] != frames or q.shape[2] < C or q.stride(1) < q.shape[2] or q.stride(0) != Lq * q.stride(1):
        _fail(op, f'shapes: q {tuple(q.shape)} with strides {tuple(q.stride())}, kv {tuple(kv.shape)}')
    _dense(op, 'out', out, F32, shape=(frames, Lq, C)); _dense(op, 'workspace', workspace, F32, min_numel=vae_attn_workspace_floats(Lk, C))
    lib.call('mg_vae_attn_rows_f32', _p(q), q.stride(1), _p(kv), ctypes.c_void_p(kv.data_ptr() + 4 * C), 2 * C, _p(out), frames, Lq, Lk, C,
             _p(workspace), _st())
    return out


def vae_latent_in(z, mean, inv_std, out):
    """z [C,T,H,W] -> out [T,H,W,C] = z / inv_std + mean per channel."""
    op = 'vae_latent_in'
    _dense(op, 'z', z, F32)
    if z.dim() != 4:
        _fail(op, f'z must be [C, T, H, W], got {tuple(z.shape)}')
    C, T, H, W = z.shape
    _dense(op, 'mean', mean, F32, min_numel=C); _dense(op, 'inv_std', inv_std, F32, min_numel=C); _dense(op, 'out', out, F32, shape=(T, H, W, C))
    lib.call('mg_vae_latent_in_f32', _p(z), _p(mean), _p(inv_std), C, T, H, W, _p(out), _st())
    return out


def vae_video_out(x, out, t_off):
    """x [T,H,W,C] -> out[:, t_off:t_off + T] of out [C,T_total,H,W], clamped to [-1, 1] (NaN becomes -1)."""
    op = 'vae_video_out'
    _dense(op, 'x', x, F32); _dense(op, 'out', out, F32)
    if x.dim() != 4 or out.dim() != 4:
        _fail(op, f'x must be [T, H, W, C] and out [C, T_total, H, W], got {tuple(x.shape)} and {tuple(out.shape)}')
    T, H, W, C = x.shape
    t_off = int(t_off)
    if (out.shape[0], out.shape[2], out.shape[3]) != (C, H, W) or t_off < 0 or t_off + T > out.shape[1]:
        _fail(op, f'frames [{t_off}, {t_off} + {T}) of x {tuple(x.shape)} do not fit out {tuple(out.shape)}')
    lib.call('mg_vae_video_out_f32', _p(x), C, T, H, W, _p(out), t_off, out.shape[1], _st())
    return out


def vae_time_interleave(x, out):
    """x [T,H,W,2C] -> out [2T,H,W,C]: frame 2t from channels [0, C), frame 2t + 1 from [C, 2C)."""
    op = 'vae_time_interleave'
    _dense(op, 'x', x, F32)
    if x.dim() != 4 or x.shape[3] % 2 or x.shape[3] == 0:
        _fail(op, f'x must be [T, H, W, 2C], got {tuple(x.shape)}')
    T, H, W, C2 = x.shape
    _dense(op, 'out', out, F32, shape=(2 * T, H, W, C2 // 2))
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
    op = 'vae_conv_strided'
    T, H, W, Cin = _dense(op, 'x', x, F32).shape
    Cout, kt, kh, kw, wc = _dense(op, 'w', w, F32).shape
    _tensor(op, 'bias', bias, F32, optional=True)
    if wc != Cin:
        _fail(op, f'x {tuple(x.shape)} and w {tuple(w.shape)} differ in Cin')
    _dense(op, 'out', out, F32, shape=vae_conv_strided_out_shape(x.shape, (kt, kh, kw), stride, pad_t0, pad_h, pad_w) + [Cout])
    if _dense(op, 'cache', cache, F32, optional=True) is not None and tuple(cache.shape[1:]) != tuple(x.shape[1:]):
        _fail(op, f'the cache must have the frame geometry of x {tuple(x.shape)}, got {tuple(cache.shape)}')
    tc = 0 if cache is None else cache.shape[0]
    lib.call('mg_vae_conv_strided_f32', _p(x), _p(cache), tc, T, H, W, Cin, _p(w), _p(bias), Cout, kt, kh, kw, int(stride[0]), int(stride[1]),
             int(stride[2]), int(pad_t0), int(pad_h[0]), int(pad_h[1]), int(pad_w[0]), int(pad_w[1]), _p(out), int(mode), _st())
    return out


def vae_video_in(video, t0, n, out):
    """video [3,T,H,W] fp32, frames [t0, t0 + n) -> out [n,H,W+2,4]: the staged layout of vae_conv_in3 (zero columns 0 and W+1, zero channel 3)."""
    op = 'vae_video_in'
    _dense(op, 'video', video, F32)
    if video.dim() != 4 or video.shape[0] != 3:
        _fail(op, f'video must be [3, T, H, W], got {tuple(video.shape)}')
    _, T, H, W = video.shape
    _dense(op, 'out', out, F32, shape=(n, H, W + 2, 4))
    lib.call('mg_vae_video_in_f32', _p(video), T, H, W, int(t0), int(n), _p(out), _st())
    return out


def vae_conv_in3(xs, w, bias, out, cache=None, mode=VAE_EXACT):
    """the 3 -> Cout causal 3x3x3 input convolution: xs [T,H,W+2,4] from vae_video_in, cache [<= 2,H,W+2,4] staged frames of the
    previous chunk, w [Cout,3,3,3,4] (channel 3 zero), out [T,H,W,Cout]."""
    op = 'vae_conv_in3'
    T, H, Wp, c4 = _dense(op, 'xs', xs, F32).shape
    Cout = _dense(op, 'w', w, F32).shape[0]
    _tensor(op, 'bias', bias, F32, optional=True)
    if c4 != 4 or tuple(w.shape) != (Cout, 3, 3, 3, 4):
        _fail(op, f'xs {tuple(xs.shape)} must be [T, H, W + 2, 4] and w {tuple(w.shape)} [Cout, 3, 3, 3, 4]')
    _dense(op, 'out', out, F32, shape=(T, H, Wp - 2, Cout))
    if _dense(op, 'cache', cache, F32, optional=True) is not None and tuple(cache.shape[1:]) != tuple(xs.shape[1:]):
        _fail(op, f'the cache must have the frame geometry of xs {tuple(xs.shape)}, got {tuple(cache.shape)}')
    tc = 0 if cache is None else cache.shape[0]
    lib.call('mg_vae_conv_in3_f32', _p(xs), _p(cache), tc, T, H, Wp - 2, _p(w), _p(bias), Cout, _p(out), int(mode), _st())
    return out


def vae_latent_out(x, mean, inv_std, out):
    """x [T,H,W,Cx] channels-last -> out [C,T,H,W] = (x[..., :C] - mean) * inv_std (C = out.shape[0] <= Cx)."""
    op = 'vae_latent_out'
    T, H, W, Cx = _dense(op, 'x', x, F32).shape
    C = _dense(op, 'out', out, F32).shape[0]
    if tuple(out.shape) != (C, T, H, W) or C > Cx:
        _fail(op, f'x {tuple(x.shape)} needs an out [C <= {Cx}, {T}, {H}, {W}], got {tuple(out.shape)}')
    _tensor(op, 'mean', mean, F32); _tensor(op, 'inv_std', inv_std, F32)
    if mean.numel() < C or inv_std.numel() < C:
        _fail(op, f'{C} channels need as many means and scales, got {mean.numel()} and {inv_std.numel()}')
    lib.call('mg_vae_latent_out_f32', _p(x), Cx, _p(mean), _p(inv_std), C, T, H, W, _p(out), _st())
    return out


def _rgb_planes(op, name, t, dims):
    """a dense fp32 [3, ...] tensor of `dims` dimensions -> its shape behind the channel axis"""
    if _dense(op, name, t, F32).dim() != dims or t.shape[0] != 3:
        _fail(op, f'{name} must be [3, {"T, " if dims == 4 else ""}H, W], got {tuple(t.shape)}')
    return t.shape[1:]


def video_to_u8(video, lo=-1.0, hi=1.0):
    """[3,T,H,W] fp32 -> uint8 frames [T,H,W,3] (reference cache_video arithmetic)."""
    T, H, W = _rgb_planes('video_to_u8', 'video', video, 4)
    out = torch.empty(T, H, W, 3, dtype=U8, device=video.device)
    lib.call('mg_video_to_u8', _p(video), T, H, W, float(lo), float(hi), _p(out), _st())
    return out


def video_from_u8(frames, H, W, out=None):
    """uint8 RGB frames [T,H0,W0,3] of any size -> the clip [3,T,H,W] fp32 in [-1,1]: resize to cover (antialiased triangle filter),
    centre crop, v / 127.5 - 1 (mg_video_from_u8; the definition is in include/moviigen_hip.h)."""
    op = 'video_from_u8'
    if _dense(op, 'frames', frames, U8).dim() != 4 or frames.shape[3] != 3:
        _fail(op, f'frames must be [T, H0, W0, 3], got {tuple(frames.shape)}')
    T, H0, W0, _ = frames.shape
    if out is None:
        out = torch.empty(3, T, int(H), int(W), dtype=F32, device=frames.device)
    _dense(op, 'out', out, F32, shape=(3, T, int(H), int(W)))
    lib.call('mg_video_from_u8', _p(frames), T, H0, W0, int(H), int(W), _p(out), _st())
    return out


def mask_from_u8(mask, T, H, W, keep_frames=0, out=None):
    """uint8 mask [Tm,H0,W0] (Tm == 1 or >= T; >= 128 after the resize = regenerate) -> the pixel mask [T,H,W] uint8 0/1 through the geometry and
    filter of video_from_u8; frames below keep_frames are 0 = kept (mg_mask_from_u8; the definition is in include/moviigen_hip.h)."""
    op = 'mask_from_u8'
    if _dense(op, 'mask', mask, U8).dim() != 3:
        _fail(op, f'mask must be [Tm, H0, W0], got {tuple(mask.shape)}')
    Tm, H0, W0 = mask.shape
    if out is None:
        out = torch.empty(int(T), int(H), int(W), dtype=U8, device=mask.device)
    _dense(op, 'out', out, U8, shape=(int(T), int(H), int(W)))
    lib.call('mg_mask_from_u8', _p(mask), Tm, H0, W0, int(T), int(H), int(W), int(keep_frames), _p(out), _st())
    return out


def mask_to_latent(pm, stride):
    """pixel mask [T,H,W] uint8 -> the latent-grid mask [(T-1)/st+1, H/sh, W/sw] uint8 0/1 of a causal VAE with `stride` = (st, sh, sw): the OR
    over every pixel under a latent cell (mg_mask_to_latent_u8)."""
    op = 'mask_to_latent'
    if _dense(op, 'pm', pm, U8).dim() != 3:
        _fail(op, f'pm must be [T, H, W], got {tuple(pm.shape)}')
    T, H, W = pm.shape
    st, sh, sw = (int(v) for v in stride)
    if min(st, sh, sw) <= 0:
        _fail(op, f'stride must be positive, got {(st, sh, sw)}')
    lm = torch.empty((T - 1) // st + 1, H // sh, W // sw, dtype=U8, device=pm.device)
    lib.call('mg_mask_to_latent_u8', _p(pm), T, H, W, st, sh, sw, _p(lm), _st())
    return lm


def masked_renoise(latent, z0, noise, lm, c0, c1):
    """latent [C, ...] fp32 IN PLACE: c0 z0 + c1 noise (the bits of lincomb) where lm [...] uint8 is 0, untouched where it is not
    (mg_masked_renoise_f32)."""
    op = 'masked_renoise'
    if _dense(op, 'latent', latent, F32).dim() < 2:
        _fail(op, f'latent must be [C, ...], got {tuple(latent.shape)}')
    _dense(op, 'z0', z0, F32, shape=latent.shape); _dense(op, 'noise', noise, F32, shape=latent.shape)
    if _dense(op, 'lm', lm, U8).numel() * latent.shape[0] != latent.numel():
        _fail(op, f'lm {tuple(lm.shape)} must hold one element per latent cell of {tuple(latent.shape)}')
    lib.call('mg_masked_renoise_f32', _p(latent), _p(z0), _p(noise), _p(lm), float(c0), float(c1), latent.shape[0], lm.numel(), _st())
    return latent


def mask_composite(video, src, pm):
    """video [3,T,H,W] fp32 IN PLACE: src where pm [T,H,W] uint8 is 0, untouched where it is not (mg_mask_composite_f32)."""
    op = 'mask_composite'
    T, H, W = _rgb_planes(op, 'video', video, 4)
    _dense(op, 'src', src, F32, shape=video.shape); _dense(op, 'pm', pm, U8, shape=(T, H, W))
    lib.call('mg_mask_composite_f32', _p(video), _p(src), _p(pm), T, H * W, _st())
    return video


def _window_dims(op, name, whole, win, f0):
    """(C, F, hw, Fw) of a whole clip [C, F, ...] and one window [C, Fw, ...] of it at frames [f0, f0 + Fw), both dense fp32"""
    _dense(op, name[0], whole, F32); _dense(op, name[1], win, F32)
    if whole.dim() < 2 or win.dim() != whole.dim() or win.shape[0] != whole.shape[0] or tuple(win.shape[2:]) != tuple(whole.shape[2:]) \
            or min(whole.shape) < 1 or win.shape[1] < 1 or not 0 <= int(f0) <= whole.shape[1] - win.shape[1]:
        _fail(op, f'{name[0]} {tuple(whole.shape)} and {name[1]} {tuple(win.shape)} must be [C, F, ...] and [C, Fw, ...] with '
                  f'0 <= f0 <= F - Fw, f0 = {f0}')
    C, F, Fw = whole.shape[0], whole.shape[1], win.shape[1]
    return C, F, whole.numel() // (C * F), Fw


def window_gather(x, f0, out):
    """out [C, Fw, ...] <- x[:, f0:f0 + Fw] of the dense fp32 clip x [C, F, ...]: a copy, the bits are unchanged (mg_window_gather_f32)."""
    C, F, hw, Fw = _window_dims('window_gather', ('x', 'out'), x, out, f0)
    lib.call('mg_window_gather_f32', _p(x), C, F, hw, int(f0), Fw, _p(out), _st())
    return out


def window_blend(acc, pred, f0, w, first):
    """acc [C, F, ...] fp32 IN PLACE at frames [f0, f0 + Fw), from the window's prediction pred [C, Fw, ...]: w[j] * pred where first[j]
    is non-zero (a select: acc is not read there and needs no initial value), fma(w[j], pred, acc) where it is zero.  w fp32 [Fw] and
    first uint8 [Fw] live on the device; frames outside the window are not touched (mg_window_blend_f32)."""
    op = 'window_blend'
    C, F, hw, Fw = _window_dims(op, ('acc', 'pred'), acc, pred, f0)
    _dense(op, 'w', w, F32, shape=(Fw,)); _dense(op, 'first', first, U8, shape=(Fw,))
    lib.call('mg_window_blend_f32', _p(acc), _p(pred), C, F, hw, int(f0), Fw, _p(w), _p(first), _st())
    return acc


def gate_residual(x, y, gate=None):
    """x [rows, dim] fp32 += y [rows, dim] bf16 * gate [dim] fp32 (None = 1)."""
    op = 'gate_residual'
    rows, dim = _rows(op, 'x', x, F32).shape
    _rows(op, 'y', y, BF16, rows=rows, cols=dim); _dense(op, 'gate', gate, F32, numel=dim, optional=True)
    lib.call('mg_gate_residual_f32', _p(x), x.stride(0), _p(y), y.stride(0), _p(gate), rows, dim, _st())
    return x


def _sp_chk_cols(op, P, cols, col0, w):
    if P < 1 or w < 1 or w % 8 or col0 < 0 or col0 % 8 or cols % 8 or col0 + w > cols:
        _fail(op, f'columns [{col0}, {col0} + {w}) of {P} blocks of {cols} — all multiples of 8 (16-byte vectors), inside the block')


def sp_pack_qkv(q, k, v, P, cols_per_dest, col0, w, send):
    """q, k, v [Lloc, >= P*cols_per_dest] bf16 (column slices ok) -> send [P, Lloc, 3w] (see moviigen_hip.h)."""
    op = 'sp_pack_qkv'
    P, cols_per_dest, col0, w = int(P), int(cols_per_dest), int(col0), int(w)
    _sp_chk_cols(op, P, cols_per_dest, col0, w)
    Lloc = _rows(op, 'q', q, BF16, min_cols=P * cols_per_dest).shape[0]
    _rows(op, 'k', k, BF16, rows=Lloc, min_cols=P * cols_per_dest); _rows(op, 'v', v, BF16, rows=Lloc, min_cols=P * cols_per_dest)
    _dense(op, 'send', send, BF16, min_numel=P * Lloc * 3 * w)
    lib.call('mg_sp_pack_qkv_bf16', _p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), Lloc, P, cols_per_dest, col0, w,
             _p(send), _st())
    return send


def sp_unpack_o(recv, P, cols_per_src, col0, w, o):
    """recv [P, Lloc, w] bf16 -> o[:, p*cols_per_src + col0 : +w] for every source rank p."""
    op = 'sp_unpack_o'
    P, cols_per_src, col0, w = int(P), int(cols_per_src), int(col0), int(w)
    _sp_chk_cols(op, P, cols_per_src, col0, w)
    Lloc = _rows(op, 'o', o, BF16, min_cols=P * cols_per_src).shape[0]
    _dense(op, 'recv', recv, BF16, min_numel=P * Lloc * w)
    lib.call('mg_sp_unpack_o_bf16', _p(recv), Lloc, P, cols_per_src, col0, w, _p(o), o.stride(0), _st())
    return o


def sp_copy_blocks(src, s_blk, s_row, dst, d_blk, d_row, blocks, rows, width):
    """dst[b][r][:width] = src[b][r][:width] with element strides (*_blk, *_row) from each tensor's first element: the reshapes around an
    all-to-all.  Every element addressed has to lie inside the tensor's storage."""
    op = 'sp_copy_blocks'
    _tensor(op, 'src', src, BF16); _tensor(op, 'dst', dst, BF16)
    s_blk, s_row, d_blk, d_row, blocks, rows, width = (int(v) for v in (s_blk, s_row, d_blk, d_row, blocks, rows, width))
    if blocks < 0 or rows < 0 or width < 1 or width % 8 or min(s_blk, s_row, d_blk, d_row) < 0:
        _fail(op, f'{blocks} blocks of {rows} rows of {width} (a multiple of 8) with strides {(s_blk, s_row)} -> {(d_blk, d_row)}')
    for n, t, blk, row in (('src', src, s_blk, s_row), ('dst', dst, d_blk, d_row)):
        last = (blocks - 1) * blk + (rows - 1) * row + width - 1
        if blocks and rows and t.storage_offset() + last >= t.untyped_storage().nbytes() // t.element_size():
            _fail(op, f'element {last} of {n} {tuple(t.shape)} (block {blocks - 1}, row {rows - 1}, column {width - 1}) lies outside its storage')
    lib.call('mg_sp_copy_blocks_bf16', _p(src), s_blk, s_row, _p(dst), d_blk, d_row, blocks, rows, width, _st())
    return dst


def image_to_u8(image, lo=-1.0, hi=1.0):
    """[3,H,W] fp32 -> uint8 pixels [H,W,3] (reference cache_image / torchvision save_image arithmetic: rounds)."""
    H, W = _rgb_planes('image_to_u8', 'image', image, 3)
    out = torch.empty(H, W, 3, dtype=U8, device=image.device)
    lib.call('mg_image_to_u8', _p(image), H, W, float(lo), float(hi), _p(out), _st())
    return out


def attention_merge(acc, lse_acc, part, lse_part, heads, first, out=None):
    """ring attention: fold block result (part bf16, lse_part) into (acc fp32, lse_acc); out = bf16 copy of acc."""
    op = 'attention_merge'
    rows, cols = _rows(op, 'acc', acc, F32, min_cols=int(heads) * 128).shape
    _rows(op, 'part', part, BF16, rows=rows, cols=cols); _rows(op, 'out', out, BF16, min_rows=rows, min_cols=cols, optional=True)
    _dense(op, 'lse_acc', lse_acc, F32, min_numel=int(heads) * rows); _dense(op, 'lse_part', lse_part, F32, min_numel=int(heads) * rows)
    lib.call('mg_attn_merge_f32', _p(acc), acc.stride(0), _p(lse_acc), _p(part), part.stride(0), _p(lse_part), _p(out),
             out.stride(0) if out is not None else 0, rows, int(heads), int(bool(first)), _st())
    return acc
