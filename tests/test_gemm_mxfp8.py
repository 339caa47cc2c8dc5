"""Opt-in MXFP8 GEMMs of the DiT linear layers: the format's reference (tests/mxfp8_ref.py), the quantiser and the block-scaled
GEMM (csrc/gemm_mxfp8.hip) against it, and WanModel.set_gemm_precision('mxfp8')."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp8_ref as R  # noqa: E402
import weights as W  # noqa: E402
from abi_ref import header_declarations  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------
# CPU: the reference's own properties, and the ABI
# ------------------------------------------------------------------------------------------------
def test_ref_dequant_quant_is_identity_on_representable_values():
    g = torch.Generator().manual_seed(1)
    q = torch.randint(0, 256, (64, 256), generator=g, dtype=torch.int64)
    q = torch.where((q & 0x7f) == 0x7f, q & 0x80, q)                 # no NaN codes
    # every block holds one element of the top binade (256 .. 448): its scale is then the only one that represents the block
    q[:, ::32] = torch.randint(0x78, 0x7f, (64, 8), generator=g) | (torch.randint(0, 2, (64, 8), generator=g) << 7)
    q = q.to(torch.uint8)
    s = torch.randint(10, 246, (64, 8), generator=g).to(torch.uint8)
    x = R.dequant(q, s)
    assert torch.isfinite(x).all()
    q2, s2 = R.quant(x)
    assert torch.equal(s2, s) and torch.equal(q2, q)
    assert torch.equal(R.dequant(q2, s2), x)


def test_ref_saturates_instead_of_nan():
    x = torch.zeros(1, 64)
    x[0, 3], x[0, 4], x[0, 5] = 500.0, -500.0, 1.0
    q, s = R.quant(x)
    d = R.dequant(q, s)
    assert s[0, 0].item() == 127                                     # floor(log2 500) = 8 -> e = 0
    assert not torch.isnan(d).any()
    assert d[0, 3].item() == 448.0 and d[0, 4].item() == -448.0 and d[0, 5].item() == 1.0
    assert torch.isnan(torch.tensor(500.0).to(torch.float8_e4m3fn).float())      # what the definition avoids


def test_ref_zero_block():
    x = torch.randn(2, 64)
    x[1, 32:] = 0
    q, s = R.quant(x)
    assert s[1, 1].item() == 0 and int(q[1, 32:].max()) == 0
    assert torch.equal(R.dequant(q, s)[1, 32:], torch.zeros(32))


def test_ref_scale_byte_table():
    mags = [m * 2.0 ** p for p in range(-100, 101) for m in (1.0, 1.5, 1.984375)]
    x = torch.zeros(len(mags), 32)
    x[:, 7] = torch.tensor(mags, dtype=torch.float64).float()
    x[:, 8] = -0.25 * x[:, 7]
    _, s = R.quant(x)
    want = [math.frexp(m)[1] - 1 + 119 for m in mags]                # floor(log2 amax) + 119
    assert s[:, 0].tolist() == want


def test_mxfp8_entry_points_are_declared():
    from wan.backend import lib
    decl = header_declarations()
    for name, nargs in (('mg_quant_mxfp8_rows', 9), ('mg_gemm_mxfp8', 17)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name]) == nargs
        assert name in decl and decl[name] == (lib.c_int, lib.SIGNATURES[name]), name


# ------------------------------------------------------------------------------------------------
# GPU: quantiser, bit-exact
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('K', [256, 384])
def test_quantiser_matches_reference_bytes(dev, K):
    from wan.backend import ops
    rows = 37
    x = W.randn((rows, K), 40 + K)
    x[0, :32] = 0                                                     # a zero block
    x[1, 32:64] *= 0.1
    x[1, 37] = 500.0                                                  # amax 500: saturates to 448
    x[2, :32] = x[2, :32].clamp(-3.0, 3.0)
    x[2, 11] = -4.0                                                   # amax exactly a power of two
    x[3] *= 2.0 ** -60
    x[4] *= 2.0 ** 60
    wide = torch.zeros(rows, K + 64, dtype=torch.bfloat16)
    wide[:, :K] = x.bfloat16()
    xd = wide.to(dev)[:, :K]                                          # ldx > K
    assert xd.stride(0) == K + 64
    q, s = ops.quant_mxfp8(xd)
    qr, sr = R.quant(wide[:, :K])
    assert torch.equal(s.cpu(), sr), (s.cpu().int() - sr.int()).abs().max()
    assert torch.equal(q.cpu(), qr), int((q.cpu() != qr).sum())
    assert sr[0, 0].item() == 0 and R.dequant(qr, sr)[1, 37].item() == 448.0


# ------------------------------------------------------------------------------------------------
# GPU: GEMM on exact data, bit for bit against mg_gemm_bf16 on the dequantised operands
# ------------------------------------------------------------------------------------------------
def _exact_operands(M, N, K, seed):
    """integers in [-8, 8] as e4m3, scale bytes 125..129 that differ per row and per 32-block and differently on the two sides:
    every product is a multiple of 2^-4 below 2^10 and every partial sum stays below 2^24 units, so fp32 accumulation is exact in
    any order and a swapped row/column or a misplaced scale cannot cancel."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-8, 9, (M, K), generator=g).float()
    w = torch.randint(-8, 9, (N, K), generator=g).float()
    kb = torch.arange(K // 32)
    a_s = (125 + (torch.arange(M)[:, None] + 2 * kb[None, :]) % 5).to(torch.uint8)
    w_s = (125 + (3 * torch.arange(N)[:, None] + kb[None, :]) % 5).to(torch.uint8)
    aq, wq = a.to(torch.float8_e4m3fn).view(torch.uint8), w.to(torch.float8_e4m3fn).view(torch.uint8)
    return aq, a_s, wq, w_s


def _run_pair(dev, ops, aq, a_s, wq, w_s, bias, gate, r0, epi):
    """(mg_gemm_mxfp8, mg_gemm_bf16 on the dequantised operands) for one epilogue"""
    M, N = aq.shape[0], wq.shape[0]
    ad, wd = R.dequant(aq, a_s), R.dequant(wq, w_s)
    assert torch.equal(ad.bfloat16().float(), ad) and torch.equal(wd.bfloat16().float(), wd)     # exactly bf16 values
    outs = []
    for fp8 in (True, False):
        if epi == ops.GATE_RESID_F32:
            out = r0.to(dev).clone()
        else:
            out = torch.empty(M, N, dtype=torch.bfloat16 if epi in (0, 1) else torch.float32, device=dev)
        gt = gate.to(dev) if epi == ops.GATE_RESID_F32 else None
        if fp8:
            ops.gemm_mxfp8(aq.to(dev), a_s.to(dev), wq.to(dev), w_s.to(dev), bias.to(dev), epi, out, gate=gt)
        else:
            ops.gemm(ad.bfloat16().to(dev), wd.bfloat16().to(dev), bias.to(dev), epi, out, gate=gt)
        outs.append(out.float().cpu())
    return outs


# the kernel's tile is 256 x 256: (600, 528, 256) = two tiles and a tail in both dimensions, several k-tiles
@gpu
@pytest.mark.parametrize('M,N,K', [(M, N, K) for M in (1, 37, 261) for N in (16, 272) for K in (128, 384)] + [(600, 528, 256)])
def test_gemm_exact_data_bit_equal_to_bf16_gemm(dev, M, N, K):
    from wan.backend import ops
    aq, a_s, wq, w_s = _exact_operands(M, N, K, 1000 + M + N + K)
    bias, gate, r0 = W.randn((N,), 50), W.randn((N,), 51), W.randn((M, N), 52)
    for epi in (0, 1, 2, 3):
        got, ref = _run_pair(dev, ops, aq, a_s, wq, w_s, bias, gate, r0, epi)
        assert torch.isfinite(got).all()
        assert torch.equal(got, ref), (epi, int((got != ref).sum()), (got - ref).abs().max().item())
    # and the plain product itself against fp64: epilogue 3 (MG_EPI_BIAS_F32) stores float(bf16(acc + bias)), the bf16-rounded
    # Linear output widened to fp32, so the exact sum is rounded to bf16 before the comparison
    out = torch.empty(M, N, dtype=torch.float32, device=dev)
    ops.gemm_mxfp8(aq.to(dev), a_s.to(dev), wq.to(dev), w_s.to(dev), None, ops.BIAS_F32, out)
    exact = R.dequant(aq, a_s).double() @ R.dequant(wq, w_s).double().T
    assert torch.equal(out.cpu(), exact.float().bfloat16().float())


# ------------------------------------------------------------------------------------------------
# GPU: GEMM on random DiT-like data
# ------------------------------------------------------------------------------------------------
RM, RN = 261, 272


@functools.lru_cache(maxsize=None)
def _random_case(K):
    """N(0,1) activations with one x50 channel against N(0, 0.02^2) weights, quantised by the reference; the fp64 product of the
    dequantised operands plus bias, and sum_k |a_k| |w_k|.  Computed once per K, shared, never modified."""
    a = W.randn((RM, K), 60)
    a[:, 7] *= 50.0
    w = W.randn((RN, K), 61) * 0.02
    bias = W.randn((RN,), 62)
    aq, a_s = R.quant(a)
    wq, w_s = R.quant(w)
    ad, wd = R.dequant(aq, a_s).double(), R.dequant(wq, w_s).double()
    return aq, a_s, wq, w_s, bias, ad @ wd.T + bias.double(), ad.abs() @ wd.abs().T


@gpu
@pytest.mark.parametrize('K', [5120, 13824])
@pytest.mark.parametrize('epi', [0, 3])
def test_gemm_random_data_within_fp32_accumulation_bound(dev, K, epi):
    """|out - ref| <= 2^-8 |ref| + 2 K 2^-24 sum_k |a_k| |w_k|: one bf16 rounding with slack for a flipped ulp, plus the worst case
    of an fp32 accumulation of K terms in any order."""
    from wan.backend import ops
    aq, a_s, wq, w_s, bias, ref, absum = _random_case(K)
    out = torch.empty(RM, RN, dtype=torch.bfloat16 if epi == 0 else torch.float32, device=dev)
    ops.gemm_mxfp8(aq.to(dev), a_s.to(dev), wq.to(dev), w_s.to(dev), bias.to(dev), epi, out)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    acc_ratio = ((err - 2.0 ** -8 * ref.abs()).clamp_min(0) / absum).max().item()
    print(f'K={K} epi={epi}: max err {err.max().item():.3e}, max (err - 2^-8|ref|)/sum|a||w| = {acc_ratio:.3e} '
          f'(bound {2 * K * 2.0 ** -24:.3e}), rel-L2 {((got - ref).norm() / ref.norm()).item():.3e}')
    assert (err <= 2.0 ** -8 * ref.abs() + 2 * K * 2.0 ** -24 * absum).all()


@gpu
@pytest.mark.parametrize('epi', [1, 2])
def test_gemm_random_data_gelu_and_gated_residual(dev, epi):
    """epilogues 1 and 2 at K = 5120 against mg_gemm_bf16 on the dequantised operands, with test_gemm_epilogues' tolerance for them:
    max error below 1.2e-2 of the reference's maximum (one bf16 ulp of slack at a rounding boundary)."""
    from wan.backend import ops
    aq, a_s, wq, w_s, bias, _, _ = _random_case(5120)
    got, ref = _run_pair(dev, ops, aq, a_s, wq, w_s, bias, W.randn((RN,), 63), W.randn((RM, RN), 64), epi)
    assert torch.isfinite(got).all()
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f'epi={epi}: scale error {err:.3e}')
    assert err < 1.2e-2


@gpu
def test_shape_refusals(dev):
    import ctypes
    from wan.backend import lib
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    out = torch.zeros(1 << 14, dtype=torch.float32, device=dev)
    p, o, st = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for N, K in ((16, 96), (8, 128)):
        with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
            lib.call('mg_gemm_mxfp8', p, 256, p, 8, p, 256, p, 8, None, 4, N, K, 3, o, 64, None, st)
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        lib.call('mg_quant_mxfp8_rows', p, 128, 4, 96, p, 128, p, 4, st)
    lib.call('mg_gemm_mxfp8', p, 256, p, 8, p, 256, p, 8, None, 4, 16, 128, 3, o, 64, None, st)      # the same call with a legal shape
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# GPU: the model
# ------------------------------------------------------------------------------------------------
# rel-L2 of the 'mxfp8' forward against the bf16 forward of the same model (SMALL_DIT_HD128, 320 tokens), measured on an MI355X
# with all six sites of the layer loop on fp8 (MXFP8_SITES has since switched three back to bf16; the figure for that table has not been taken, the forward stays inside the bound):
MODEL_REL_L2_MEASURED = 1.869e-2
MODEL_REL_L2_BOUND = 2 * MODEL_REL_L2_MEASURED     # box-to-box and seed spread of a new quantity


@gpu
def test_model_mxfp8_forward(dev):
    import wan
    cfg = W.SMALL_DIT_HD128                       # head_dim 128, dim 256, ffn_dim 512, 2 layers
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(W.make_dit_params(cfg, 0))
    m.to(dev)
    lat = W.randn((16, 5, 16, 16), 20).to(dev)    # 5 x 8 x 8 = 320 tokens: two 256-row tiles, the second a tail
    c1, c2 = W.randn((33, 128), 30).to(dev), W.randn((9, 128), 31).to(dev)
    t = torch.tensor([700], device=dev)
    ref = m([lat], t=t, context=[c1], seq_len=320)[0].clone()
    assert m.gemm_precision == 'bf16'
    m.set_gemm_precision('mxfp8')
    a1 = m([lat], t=t, context=[c1], seq_len=320)[0].clone()
    a2 = m([lat], t=t, context=[c1], seq_len=320)[0].clone()
    assert torch.isfinite(a1).all()
    assert torch.equal(a1, a2)
    assert not torch.equal(a1, ref), 'the mxfp8 path did not run'
    rel = ((a1 - ref).double().norm() / ref.double().norm()).item()
    print(f'model rel-L2 mxfp8 vs bf16: {rel:.4e}')
    assert rel <= MODEL_REL_L2_BOUND, rel
    # forward_pair = two plain forwards, as in bf16
    b1 = m([lat], t=t, context=[c2], seq_len=320)[0].clone()
    pa, pb = m.forward_pair([lat], t, [c1], [c2], 320)
    assert torch.equal(pa[0], a1) and torch.equal(pb[0], b1)
    assert 'blocks.0.ffn.0.weight' in m.state_dict() and m.state_dict()['blocks.0.ffn.0.weight'].dtype == torch.bfloat16
    m.set_gemm_precision('bf16')
    assert torch.equal(m([lat], t=t, context=[c1], seq_len=320)[0], ref)


@gpu
def test_model_mxfp8_refuses_block_sharded_weights(dev):
    import wan
    m = wan.modules.WanModel(**W.SMALL_DIT_HD128)
    with pytest.raises(ValueError):
        m.set_gemm_precision('fp8')
    m._shards = object()                          # what wan.distributed.fsdp.BlockShards installs
    with pytest.raises(NotImplementedError, match='shard'):
        m.set_gemm_precision('mxfp8')
    m.set_gemm_precision('bf16')
