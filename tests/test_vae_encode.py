"""WanVAE.encode: the encoder half of the VAE (Encoder3d, Resample down-sampling, WanVAE_.encode) on the HIP kernels.

CPU tests pin the plain-torch restatement (tests/vae_encode_ref.py, on oracle/vae.py's modules) that the GPU tests compare
with: its fp32 evaluation against fp64, and the chunked temporal down-sampling against a whole-clip evaluation.
GPU tests: the whole encode against the restatement (<= 1e-4 of the tensor scale: the project's bound for fp32 kernels, the
one the decode is held to), the new kernels one by one against fp64 at sampled voxels (<= 1e-5, as for the existing
single-convolution tests), the full-size stages, and that the decoder's results do not move.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import weights as W
from vae_encode_ref import down, make_vae_encoder_params, vae_encode

gpu = pytest.mark.gpu


def scale_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _params(dim, seed=1):
    """decoder U encoder parameters of one seeded model."""
    P = W.make_vae_params(dim, seed)
    P.update(make_vae_encoder_params(dim, seed + 100))
    return P


# ------------------------------------------------------------------------------------------------
# CPU: the reference itself
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim,T,H,Wd', [(8, 9, 32, 48), (8, 7, 16, 24), (8, 5, 36, 44), (32, 5, 24, 40)])
def test_reference_fp32_vs_fp64(dim, T, H, Wd):
    """the restatement's fp32 evaluation against its own fp64 evaluation: the reference is not the noisy side of the GPU
    comparison (measured 2e-7 .. 6.3e-7)."""
    P = make_vae_encoder_params(dim, 3)
    video = W.randn((3, T, H, Wd), 11)
    mu32 = vae_encode(P, video)
    mu64 = vae_encode({k: v.double() for k, v in P.items()}, video.double())
    assert mu32.dtype == torch.float32 and tuple(mu32.shape) == (16, 1 + (T - 1) // 4, H // 8, Wd // 8)
    err = scale_err(mu32, mu64)
    print(f'encode reference fp32 vs fp64, dim {dim} {T}x{H}x{Wd}: scale_err {err:.2e}')
    assert err < 1e-5


def test_reference_temporal_protocol_vs_whole_clip():
    """downsample3d fed the chunks [1, 4, 4] through the one-slot cache == frame 0 passed through, then ONE stride-2 conv3d
    over the frames 0..8 (output k >= 1 reads frames 2k-2, 2k-1, 2k): the same frames gathered, fp32 summation order apart."""
    c = 8
    P = {'m.resample.1.weight': W.randn((c, c, 3, 3), 1) / math.sqrt(9 * c), 'm.resample.1.bias': 0.05 * W.randn((c,), 2),
         'm.time_conv.weight': W.randn((c, c, 3, 1, 1), 3) / math.sqrt(3 * c), 'm.time_conv.bias': 0.05 * W.randn((c,), 4)}
    x = W.randn((1, c, 9, 13, 10), 5)
    cache, outs = [None], []
    for t0, n in ((0, 1), (1, 4), (5, 4)):
        outs.append(down(P, 'm.', x[:, :, t0:t0 + n], cache, [0]))
    chunked = torch.cat(outs, dim=2)
    y = x.permute(0, 2, 1, 3, 4).reshape(9, c, 13, 10)
    y = F.conv2d(F.pad(y, (0, 1, 0, 1)), P['m.resample.1.weight'], P['m.resample.1.bias'], stride=2)
    y = y.reshape(1, 9, c, 6, 5).permute(0, 2, 1, 3, 4)
    whole = torch.cat([y[:, :, :1], F.conv3d(y, P['m.time_conv.weight'], P['m.time_conv.bias'], stride=(2, 1, 1))], dim=2)
    assert tuple(chunked.shape) == tuple(whole.shape) == (1, c, 5, 6, 5)
    assert scale_err(chunked, whole) < 1e-5


def test_decoder_only_state_dict_constructs_and_encode_names_missing_keys():
    from wan.modules.vae import WanVAE_
    m = WanVAE_(W.make_vae_params(8, 1), device='cpu')
    assert m.n_slots > 0 and m.enc_layout == []
    with pytest.raises(ValueError, match=r'encoder\.conv1\.weight'):
        m.encode(torch.zeros(3, 5, 16, 16))
    full = WanVAE_(_params(8), device='cpu')
    assert full.n_slots == m.n_slots and full.layout == m.layout and full._stages() == m._stages() and not full.enc_missing
    assert [s[2] for s in full._stages()] == [s[2] for s in m._stages()] and all(isinstance(s[2], tuple) for s in m._stages())
    assert [k for k, _ in full.enc_layout] == ['res', 'res', 'down', 'res', 'res', 'down', 'res', 'res', 'down', 'res', 'res']
    for bad in (torch.zeros(3, 0, 16, 16), torch.zeros(3, 5, 7, 16), torch.zeros(4, 5, 16, 16), torch.zeros(3, 16, 16)):
        with pytest.raises(ValueError, match='encode expects'):
            full.encode(bad)


# ------------------------------------------------------------------------------------------------
# GPU: the whole encode
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('dim,T,H,Wd', [(8, 9, 32, 48), (8, 5, 40, 24), (32, 5, 24, 40), (8, 1, 16, 16), (8, 7, 16, 24), (8, 9, 36, 44)])
def test_vae_encode_vs_reference(dev, dim, T, H, Wd):
    """WanVAE.encode against the restatement; the last two cases cover dropped trailing frames and odd intermediate sizes."""
    import wan
    P = _params(dim)
    video = W.randn((3, T, H, Wd), 70 + T)
    out = wan.modules.WanVAE(state_dict=P, device=dev).encode([video.to(dev)])[0]
    ref = vae_encode(P, video)
    assert out.dtype == torch.float32 and out.device.type == 'cuda' and tuple(out.shape) == (16, 1 + (T - 1) // 4, H // 8, Wd // 8)
    assert tuple(ref.shape) == tuple(out.shape)
    err = scale_err(out, ref)
    print(f'encode dim {dim} {T}x{H}x{Wd}: scale_err {err:.2e}')
    assert err < 1e-4


# ------------------------------------------------------------------------------------------------
# GPU: the new kernels, one by one, vs fp64 at sampled voxels
# ------------------------------------------------------------------------------------------------
def _strided_ref_f64(x, cache, w, bias, pts, stride, pad0):
    """direct fp64 evaluation at sampled OUTPUT voxels of the strided convolution: output (t, y, x) reads input coordinate
    stride * out + tap - pad0 per axis; rows / columns outside the image are zero, frames < 0 are the last frames of `cache`
    (zero where it has none).  x [T,H,W,Ci], cache [Tc,H,W,Ci] or None, w [Co,kt,kh,kw,Ci]."""
    Co, kt, kh, kw, Ci = w.shape
    T, H, Wd, _ = x.shape
    tc = 0 if cache is None else cache.shape[0]
    wd = w.double().cpu()
    out = []
    for (t, y, xx) in pts:
        acc = bias.double().cpu().clone()
        for a in range(kt):
            ts = t * stride[0] + a - pad0[0]
            assert ts < T
            if ts < -tc:
                continue
            src = x[ts] if ts >= 0 else cache[tc + ts]
            for b in range(kh):
                for c in range(kw):
                    yy, xc = y * stride[1] + b - pad0[1], xx * stride[2] + c - pad0[2]
                    if yy < 0 or yy >= H or xc < 0 or xc >= Wd:
                        continue
                    acc += wd[:, a, b, c, :] @ src[yy, xc].double().cpu()
        out.append(acc)
    return torch.stack(out)


def _sample_points(To, Ho, Wo):
    pts = [(0, 0, 0), (0, 0, Wo - 1), (0, Ho - 1, 0), (To - 1, Ho - 1, Wo - 1), (To - 1, 0, Wo - 1), (To // 2, Ho // 2, Wo // 2),
           (0, Ho - 1, Wo // 2), (To - 1, Ho // 2, Wo - 1), (0, min(1, Ho - 1), max(Wo - 2, 0))]
    return sorted(set(pts))


def _check_points(out, ref, pts, bound=1e-5):
    got = torch.stack([out[t, y, xx] for (t, y, xx) in pts]).double().cpu()
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    assert err < bound, err


@gpu
@pytest.mark.parametrize('cin,cout,T,H,Wd', [(96, 96, 2, 37, 53), (40, 192, 1, 24, 40), (192, 192, 1, 18, 31), (64, 384, 3, 9, 12),
                                             (384, 384, 1, 13, 16), (8, 8, 4, 16, 24)])
def test_strided_conv_spatial(dev, cin, cout, T, H, Wd):
    """the down-samplers' 3x3, stride 2, pad (0 before, 1 behind): ragged M, Cin % 32 != 0, odd and even H / W, Cout 96 / 192 /
    384 (and the one-block tile); the last output row / column reads the one-sided padding."""
    from wan.backend import ops
    gen = torch.Generator(device=dev).manual_seed(cin * 5 + cout)
    x = torch.randn(T, H, Wd, cin, device=dev, generator=gen)
    w = torch.randn(cout, 1, 3, 3, cin, device=dev, generator=gen) / math.sqrt(9 * cin)
    b = torch.randn(cout, device=dev, generator=gen)
    shp = ops.vae_conv_strided_out_shape(x.shape, (1, 3, 3), (1, 2, 2), 0, (0, 1), (0, 1))
    assert shp == [T, H // 2, Wd // 2]
    out = torch.full((*shp, cout), float('nan'), device=dev)
    ops.vae_conv_strided(x, w, b, out, (1, 2, 2), 0, (0, 1), (0, 1))
    assert torch.isfinite(out).all().item()
    pts = _sample_points(*shp)
    _check_points(out, _strided_ref_f64(x, None, w, b, pts, (1, 2, 2), (0, 0, 0)), pts)


@gpu
@pytest.mark.parametrize('c,T,H,Wd', [(192, 4, 9, 11), (384, 2, 5, 7), (8, 4, 6, 6), (96, 4, 16, 17)])
def test_strided_conv_temporal(dev, c, T, H, Wd):
    """time_conv of downsample3d: 3x1x1, stride 2 in time, tap origin -1 with one cached frame, no temporal padding: 4- and 2-frame chunks."""
    from wan.backend import ops
    gen = torch.Generator(device=dev).manual_seed(c + T)
    x = torch.randn(T, H, Wd, c, device=dev, generator=gen)
    cache = torch.randn(1, H, Wd, c, device=dev, generator=gen)
    w = torch.randn(c, 3, 1, 1, c, device=dev, generator=gen) / math.sqrt(3 * c)
    b = torch.randn(c, device=dev, generator=gen)
    shp = ops.vae_conv_strided_out_shape(x.shape, (3, 1, 1), (2, 1, 1), 1, (0, 0), (0, 0))
    assert shp == [T // 2, H, Wd]
    out = torch.full((*shp, c), float('nan'), device=dev)
    ops.vae_conv_strided(x, w, b, out, (2, 1, 1), 1, cache=cache)
    assert torch.isfinite(out).all().item()
    pts = _sample_points(*shp)
    _check_points(out, _strided_ref_f64(x, cache, w, b, pts, (2, 1, 1), (1, 0, 0)), pts)
    # and against torch's own strided conv3d on [cached frame | chunk], every voxel
    xin = torch.cat([cache, x]).permute(3, 0, 1, 2)[None].cpu()
    ref = F.conv3d(xin, w.permute(0, 4, 1, 2, 3).cpu(), b.cpu(), stride=(2, 1, 1))[0].permute(1, 2, 3, 0)
    assert scale_err(out, ref) < 1e-5


@gpu
def test_strided_conv_rejects_unsupported(dev):
    from wan.backend import lib, ops
    x = torch.zeros(2, 8, 8, 8, device=dev)
    w = torch.zeros(8, 1, 3, 3, 8, device=dev)
    b = torch.zeros(8, device=dev)
    out = torch.zeros(2, 4, 4, 8, device=dev)
    with pytest.raises(lib.MoviigenHipError):
        ops.vae_conv_strided(x, w, b, out, (1, 2, 2), 0, (0, 1), (0, 1), mode=ops.VAE_BF16X3)       # exact only
    with pytest.raises(lib.MoviigenHipError):
        ops.vae_conv_strided(x, w, b, torch.zeros(2, 3, 3, 8, device=dev), (1, 3, 3), 0, (0, 1), (0, 1))      # stride 3


@gpu
@pytest.mark.parametrize('cout,T,H,Wd,tc', [(8, 1, 9, 11, 0), (96, 4, 12, 20, 1), (96, 2, 17, 8, 2), (8, 4, 8, 33, 2)])
def test_input_conv_3_channels(dev, cout, T, H, Wd, tc):
    """the 3 -> cout causal 3x3x3 convolution on the staged video against the fp64 evaluation of the 3-channel convolution
    (cache of 0 / 1 / 2 frames; corners and edges read the W and H padding)."""
    from wan.backend import ops
    from test_gpu_parity import _conv_ref_f64
    gen = torch.Generator(device=dev).manual_seed(cout + T)
    video = torch.randn(3, tc + T, H, Wd, device=dev, generator=gen)
    w3 = torch.randn(cout, 3, 3, 3, 3, device=dev, generator=gen) / math.sqrt(81)                # [Co,kt,kh,kw,Ci]
    b = torch.randn(cout, device=dev, generator=gen)
    xs = ops.vae_video_in(video, tc, T, torch.empty(T, H, Wd + 2, 4, device=dev))
    cache = ops.vae_video_in(video, 0, tc, torch.empty(tc, H, Wd + 2, 4, device=dev)) if tc else None
    out = torch.full((T, H, Wd, cout), float('nan'), device=dev)
    ops.vae_conv_in3(xs, F.pad(w3, (0, 1)).contiguous(), b, out, cache=cache)
    assert torch.isfinite(out).all().item()
    cl = video.permute(1, 2, 3, 0).contiguous()                                                  # [T,H,W,3]
    pts = _sample_points(T, H, Wd)
    _check_points(out, _conv_ref_f64(cl[tc:], cl[:tc] if tc else None, w3, b, pts), pts)


@gpu
def test_layout_kernels(dev):
    from wan.backend import ops
    from wan.modules.vae import _MEAN, _STD
    gen = torch.Generator(device=dev).manual_seed(5)
    video = torch.randn(3, 7, 10, 13, device=dev, generator=gen)
    for t0, n in ((0, 1), (1, 4), (5, 2), (0, 7)):
        xs = ops.vae_video_in(video, t0, n, torch.full((n, 10, 15, 4), float('nan'), device=dev))
        assert torch.equal(xs, F.pad(video[:, t0:t0 + n].permute(1, 2, 3, 0), (0, 1, 1, 1)))
    x = torch.randn(3, 5, 6, 32, device=dev, generator=gen) * 3
    mean = torch.tensor(_MEAN, device=dev)
    inv_std = (1.0 / torch.tensor(_STD)).to(dev)
    out = ops.vae_latent_out(x, mean, inv_std, torch.full((16, 3, 5, 6), float('nan'), device=dev))
    assert scale_err(out, ((x[..., :16] - mean) * inv_std).permute(3, 0, 1, 2)) < 1e-6


# ------------------------------------------------------------------------------------------------
# GPU: full-size stages of the 1920x832 encode
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('c,H,Wd', [(96, 832, 1920), (192, 416, 960)], ids=['down96_832x1920', 'down192_416x960'])
def test_fullsize_strided_conv(dev, c, H, Wd):
    from wan.backend import ops
    gen = torch.Generator(device=dev).manual_seed(c)
    x = torch.randn(1, H, Wd, c, device=dev, generator=gen)
    w = torch.randn(c, 1, 3, 3, c, device=dev, generator=gen) / math.sqrt(9 * c)
    b = torch.randn(c, device=dev, generator=gen)
    Ho, Wo = H // 2, Wd // 2
    out = torch.full((1, Ho, Wo, c), float('nan'), device=dev)
    ops.vae_conv_strided(x, w, b, out, (1, 2, 2), 0, (0, 1), (0, 1))
    pts = [(0, 0, 0), (0, 0, Wo - 1), (0, Ho - 1, 0), (0, Ho - 1, Wo - 1), (0, 1, 1), (0, Ho // 2, Wo // 2), (0, Ho // 2 + 1, Wo - 1),
           (0, 255 % Ho, 256 % Wo), (0, Ho - 2, 63), (0, 17, Wo - 2)]
    _check_points(out, _strided_ref_f64(x, None, w, b, pts, (1, 2, 2), (0, 0, 0)), pts)
    assert torch.isfinite(out).all().item()


@gpu
def test_fullsize_input_conv(dev):
    """encoder.conv1, 3 -> 96, on one 832x1920 frame with a 2-frame cache."""
    from wan.backend import ops
    from test_gpu_parity import _conv_ref_f64
    H, Wd, cout = 832, 1920, 96
    gen = torch.Generator(device=dev).manual_seed(96)
    video = torch.randn(3, 3, H, Wd, device=dev, generator=gen)
    w3 = torch.randn(cout, 3, 3, 3, 3, device=dev, generator=gen) / 9.0
    b = torch.randn(cout, device=dev, generator=gen)
    xs = ops.vae_video_in(video, 2, 1, torch.empty(1, H, Wd + 2, 4, device=dev))
    cache = ops.vae_video_in(video, 0, 2, torch.empty(2, H, Wd + 2, 4, device=dev))
    out = torch.full((1, H, Wd, cout), float('nan'), device=dev)
    ops.vae_conv_in3(xs, F.pad(w3, (0, 1)).contiguous(), b, out, cache=cache)
    cl = video.permute(1, 2, 3, 0).contiguous()
    pts = [(0, 0, 0), (0, 0, Wd - 1), (0, H - 1, 0), (0, H - 1, Wd - 1), (0, 1, 1), (0, H // 2, Wd // 2), (0, H // 2 + 1, Wd - 1), (0, 255, 256),
           (0, H - 2, 63), (0, 17, Wd - 2)]
    _check_points(out, _conv_ref_f64(cl[2:], cl[:2], w3, b, pts), pts)
    assert torch.isfinite(out).all().item()


# ------------------------------------------------------------------------------------------------
# GPU: the decoder does not move; the two halves together
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('tile', ['auto', 256])
def test_decode_unchanged_by_encoder_weights(dev, tile):
    import wan
    z = W.randn((16, 3, 4, 6), 61).to(dev)
    a = wan.modules.WanVAE(state_dict=W.make_vae_params(8, 1), device=dev, tile=tile).decode([z])[0]
    b = wan.modules.WanVAE(state_dict=_params(8, 1), device=dev, tile=tile).decode([z])[0]
    assert torch.equal(a, b)


@gpu
def test_round_trip_real_width(dev):
    """dim-96 random weights: encode a [3,17,256,384] clip, decode the result — shapes, memory and cache protocol at the real
    channel widths (random weights reconstruct nothing: no quality claim)."""
    import wan
    vae = wan.modules.WanVAE(state_dict=_params(96, 7), device=dev)
    video = torch.rand(3, 17, 256, 384, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 2 - 1
    z = vae.encode([video])[0]
    assert tuple(z.shape) == (16, 5, 32, 48) and z.dtype == torch.float32 and torch.isfinite(z).all().item()
    out = vae.decode([z])[0]
    assert tuple(out.shape) == (3, 17, 256, 384) and torch.isfinite(out).all().item()
