"""MXFP8 where the activation is produced: mg_ln_modulate_mxfp8 (csrc/dit_elementwise.hip) and mg_gemm_mxfp8_gelu_q
(csrc/gemm_mxfp8.hip, gemm_epilogue.h) against the unfused pair they replace — the existing bf16 producer followed by the format's
reference quantiser (tests/mxfp8_ref.py) — bit for bit, and WanModel's 'mxfp8' mode with and without them."""
import ctypes
import functools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_ref as R  # noqa: E402
import weights as W  # noqa: E402
from abi_ref import header_declarations  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
POISON = 0xA5


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------
# CPU: the ABI
# ------------------------------------------------------------------------------------------------
def test_fused_entry_points_are_declared():
    from wan.backend import lib
    decl = header_declarations()
    for name, nargs in (('mg_ln_modulate_mxfp8', 16), ('mg_gemm_mxfp8_gelu_q', 17)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name]) == nargs       # (SIGNATURES: the product section's table)
        assert name in decl, name
        assert decl[name] == (lib.c_int, lib.SIGNATURES[name]) and len(decl[name][1]) == nargs


# ------------------------------------------------------------------------------------------------
# GPU: LayerNorm + modulate emitting MXFP8, bit-exact
# ------------------------------------------------------------------------------------------------
LN_ROWS = 37
LN_FORMS = {'modulate': dict(add_one=True, round_norm_bf16=False),      # norm1 / norm2: y * (1 + scale) + shift
            'affine': dict(add_one=False, round_norm_bf16=False),       # norm3: y * weight + bias
            'block0': dict(add_one=True, round_norm_bf16=True)}         # block 0: y rounded to bf16 first


@functools.lru_cache(maxsize=None)
def _ln_inputs(dim):
    """x [37, dim + 8] (the row is its first dim columns), scale, shift.  Row 0 is constant and the shift is zero over the first 64
    features: two all-zero blocks.  Rows 1 / 2 are scaled by 2^40 / 2^-40."""
    x = W.randn((LN_ROWS, dim + 8), 300 + dim)
    x[0] = 1.0
    x[1] *= 2.0 ** 40
    x[2] *= 2.0 ** -40
    scale = W.randn((dim,), 301 + dim) * 0.5
    shift = W.randn((dim,), 302 + dim)
    shift[:64] = 0
    return x, scale, shift


@gpu
@pytest.mark.parametrize('form', list(LN_FORMS))
@pytest.mark.parametrize('dim', [256, 1536, 5120, 8192])     # MAXV 2, 2, 5, 8; 1536 and 5120 are no multiples of 1024
def test_ln_modulate_mxfp8_matches_unfused_bytes(dev, dim, form):
    from wan.backend import ops
    kw = LN_FORMS[form]
    x, scale, shift = _ln_inputs(dim)
    xd = x.to(dev)[:, :dim]
    assert xd.stride(0) == dim + 8                                                      # ldx > dim
    sc, sh = scale.to(dev), shift.to(dev)
    ref_bf = ops.ln_modulate(xd, sc, sh, kw['add_one'], 1e-6, torch.empty(LN_ROWS, dim, dtype=torch.bfloat16, device=dev),
                             round_norm_bf16=kw['round_norm_bf16'])
    qr, sr = R.quant(ref_bf.cpu())
    # the cases the reference must really contain
    assert int(sr[0, 0]) == 0 and int(sr[0, 1]) == 0 and int(qr[0, :64].max()) == 0, 'no all-zero block in the constant row'
    assert bool(((qr == 0x7E) | (qr == 0xFE)).any()), 'no block whose maximum rounds into the saturating code'

    qbuf = torch.full((LN_ROWS, dim + 16), POISON, dtype=torch.uint8, device=dev)       # ldq > dim
    sbuf = torch.full((LN_ROWS, dim // 32 + 4), POISON, dtype=torch.uint8, device=dev)  # lds > dim / 32
    poisoned = torch.full((LN_ROWS, dim), -7.0, dtype=torch.bfloat16, device=dev)
    q, s = qbuf[:, :dim], sbuf[:, :dim // 32]
    ops.ln_modulate_mxfp8(xd, sc, sh, kw['add_one'], 1e-6, q, s, round_norm_bf16=kw['round_norm_bf16'])
    assert torch.equal(s.cpu(), sr), int((s.cpu() != sr).sum())
    assert torch.equal(q.cpu(), qr), int((q.cpu() != qr).sum())
    assert bool((qbuf[:, dim:] == POISON).all()) and bool((sbuf[:, dim // 32:] == POISON).all())
    assert bool((poisoned == -7.0).all())                                               # out = None: no bf16 row is written anywhere

    # with a bf16 `out`: the same bytes, and the bf16 row of the unfused kernel bit for bit
    qbuf.fill_(POISON)
    sbuf.fill_(POISON)
    obuf = torch.full((LN_ROWS, dim + 8), -7.0, dtype=torch.bfloat16, device=dev)
    ops.ln_modulate_mxfp8(xd, sc, sh, kw['add_one'], 1e-6, q, s, out=obuf[:, :dim], round_norm_bf16=kw['round_norm_bf16'])
    assert torch.equal(obuf[:, :dim].view(torch.int16), ref_bf.view(torch.int16))
    assert bool((obuf[:, dim:] == -7.0).all())
    assert torch.equal(s.cpu(), sr) and torch.equal(q.cpu(), qr)


# ------------------------------------------------------------------------------------------------
# GPU: the GELU epilogue emitting MXFP8, bit-exact
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gelu_case(M, N, K):
    """N(0,1) activations with one x50 channel against N(0, 0.02^2) weights, quantised by the reference (test_gemm_mxfp8's
    _random_case at this shape); computed once per shape, never modified."""
    a = W.randn((M, K), 60 + M + N + K)
    a[:, 7] *= 50.0
    w = W.randn((N, K), 61 + M + N + K) * 0.02
    bias = W.randn((N,), 62 + N)
    return R.quant(a) + R.quant(w) + (bias,)


# the tile is 256 x 256, a wave's share 128 x 128: N = 32 is a wave with one block of four, 288 a second N tile 32 wide, 544 two
# tiles and a 32-wide tail; M = 1, 37, 261, 600 are M tails of one, two and three tiles
@gpu
@pytest.mark.parametrize('M,N,K', [(M, N, K) for M in (1, 37, 261) for N in (32, 288) for K in (128, 384)] + [(600, 544, 256)])
def test_gemm_gelu_q_matches_unfused_bytes(dev, M, N, K):
    from wan.backend import ops
    aq, a_s, wq, w_s, bias = (t.to(dev) for t in _gelu_case(M, N, K))
    ref_bf = ops.gemm_mxfp8(aq, a_s, wq, w_s, bias, ops.BIAS_GELU_BF16, torch.empty(M, N, dtype=torch.bfloat16, device=dev))
    assert torch.isfinite(ref_bf.float()).all()
    qr, sr = R.quant(ref_bf.cpu())
    qbuf = torch.full((M, N + 48), POISON, dtype=torch.uint8, device=dev)               # ldoq > N
    sbuf = torch.full((M, (N // 32 + 3) // 4 * 4 + 8), POISON, dtype=torch.uint8, device=dev)     # ldos > N / 32, a multiple of 4
    q, s = ops.gemm_mxfp8_gelu_q(aq, a_s, wq, w_s, bias, qbuf[:, :N], sbuf[:, :N // 32])
    assert torch.equal(s.cpu(), sr), int((s.cpu() != sr).sum())
    assert torch.equal(q.cpu(), qr), int((q.cpu() != qr).sum())
    assert bool((qbuf[:, N:] == POISON).all()) and bool((sbuf[:, N // 32:] == POISON).all())


# ------------------------------------------------------------------------------------------------
# GPU: refusals
# ------------------------------------------------------------------------------------------------
@gpu
def test_fused_shape_refusals(dev):
    from wan.backend import lib
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    xf = torch.zeros(1 << 12, dtype=torch.float32, device=dev)
    p, x = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(xf.data_ptr())
    oq, osc = ctypes.c_void_p(buf.data_ptr() + (1 << 15)), ctypes.c_void_p(buf.data_ptr() + (3 << 14))     # outputs apart from the inputs
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ln(dim):
        lib.call('mg_ln_modulate_mxfp8', x, 256, 4, dim, None, None, 1, 1e-6, 0, None, 0, oq, 256, osc, 8, st)

    def gemm(N):
        lib.call('mg_gemm_mxfp8_gelu_q', p, 256, p, 8, p, 256, p, 8, None, 4, N, 128, oq, 256, osc, 8, st)

    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ln(96)
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        gemm(16)
    ln(128)                                                                             # the same calls with legal shapes
    gemm(32)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# GPU: the model
# ------------------------------------------------------------------------------------------------
ALL_SITES = {'wqkv': True, 'self_attn.o': True, 'cross_attn.q': True, 'cross_attn.o': True, 'ffn.0': True, 'ffn.2': True}


@gpu
def test_model_fused_producers_equal_unfused(dev, monkeypatch):
    import wan
    from wan.backend import ops
    from wan.modules import model as M
    cfg = W.SMALL_DIT_HD128                       # head_dim 128, dim 256, ffn_dim 512, 2 layers
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(W.make_dit_params(cfg, 0))
    m.to(dev)
    lat = W.randn((16, 5, 16, 16), 20).to(dev)    # 5 x 8 x 8 = 320 tokens: two 256-row tiles, the second a tail
    c1, c2 = W.randn((33, 128), 30).to(dev), W.randn((9, 128), 31).to(dev)
    t = torch.tensor([700], device=dev)
    fwd = lambda c=c1: m([lat], t=t, context=[c], seq_len=320)[0].clone()  # noqa: E731
    ref_bf16 = fwd()                              # before the mode was ever switched
    assert m._mx_fuse is True

    # both producers wired in, whatever the shipped MXFP8_FUSED_PRODUCERS says (a producer that lost its measurement stays covered)
    monkeypatch.setattr(M, 'MXFP8_FUSED_PRODUCERS', {'ln_modulate': True, 'gelu': True})
    calls = []
    real_quant = ops.quant_mxfp8

    def counting_quant(x, q=None, scales=None):
        calls.append(x.data_ptr())
        return real_quant(x, q, scales)
    monkeypatch.setattr(ops, 'quant_mxfp8', counting_quant)

    def both(sites):
        """(fused, unfused) forwards and forward_pairs under `sites`, and the activations the fused forward quantised by itself"""
        monkeypatch.setattr(M, 'MXFP8_SITES', sites)
        m._mx = None
        m.set_gemm_precision('mxfp8')
        m._mx_fuse = True
        fwd()                                     # quantises the weights (also through ops.quant_mxfp8)
        calls.clear()
        fused = fwd()
        fused_calls = list(calls)
        pair = m.forward_pair([lat], t, [c1], [c2], 320)
        pair = (pair[0][0].clone(), pair[1][0].clone())
        m._mx_fuse = False
        calls.clear()
        plain = fwd()
        n_plain = len(calls)
        pair_plain = m.forward_pair([lat], t, [c1], [c2], 320)
        assert torch.isfinite(fused).all() and not torch.equal(fused, ref_bf16)
        assert torch.equal(fused, plain)
        assert torch.equal(pair[0], pair_plain[0][0]) and torch.equal(pair[1], pair_plain[1][0])
        assert torch.equal(pair[0], fused)
        m._mx_fuse = True
        return fused_calls, n_plain

    attn_out = lambda: next(iter(m._ws.values()))['a'].data_ptr()  # noqa: E731
    layers = cfg['num_layers']
    # the shipped table: the stand-alone quantiser runs only in front of the sites an attention output feeds
    shipped = dict(M.MXFP8_SITES)
    fused_calls, n_plain = both(shipped)
    n_fp8 = sum(shipped.values())
    n_attn = int(shipped['self_attn.o']) + int(shipped['cross_attn.o'])
    assert n_plain == layers * n_fp8
    assert len(fused_calls) == layers * n_attn and all(p == attn_out() for p in fused_calls)
    # all six sites on fp8: cross_attn.q takes the fused LayerNorm too
    fused_calls, n_plain = both(ALL_SITES)
    assert n_plain == layers * 6
    assert len(fused_calls) == layers * 2 and all(p == attn_out() for p in fused_calls)

    # a replaced self-attention forward of block 0 reads the bf16 h (operator seam 2): fused equals unfused there as well
    def my_attn(self, x, seq_lens, grid_sizes, freqs):
        return type(self).forward(self, x, seq_lens, grid_sizes, freqs)
    monkeypatch.setattr(M, 'MXFP8_SITES', shipped)
    m._mx = None
    m.blocks[0].self_attn.forward = types.MethodType(my_attn, m.blocks[0].self_attn)
    m._mx_fuse = True
    seam_fused = fwd()
    m._mx_fuse = False
    assert torch.equal(seam_fused, fwd())
    del m.blocks[0].self_attn.forward
    m._mx_fuse = True

    m.set_gemm_precision('bf16')
    assert torch.equal(fwd(), ref_bf16)
