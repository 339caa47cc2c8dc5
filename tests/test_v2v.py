"""Video-to-video start of WanT2V.generate (init_video, strength): the frame ingest kernel mg_video_from_u8, WanVAE.encode on a
mode='bf16x3' object, the schedulers' set_begin_index and the generate path itself.

CPU: the declarations; the fp64 restatement of the ingest (tests/resize_ref.py) against torch's own antialiased bilinear resize;
a start in the middle of the schedule with a model whose x0-prediction is exact; the strength -> steps mapping.
GPU: the ingest kernel against the restatement (<= 1e-5 absolute on the [-1, 1] output: both sides are convex combinations of values
in [-1, 1] with <= 17 fp32 terms per axis, an error of about 2 x 17 x 2^-24 = 2e-6), the bf16x3 encode against the exact one (<= 1e-4
of the tensor scale: the bound the exact encode and the fast decode are held to) and generate with init_video.
"""
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import weights as W
from abi_ref import header_declarations
from resize_ref import axis_weights, cover_geometry, resize_f64, video_from_u8_f64

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def scale_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _frames(T, H0, W0, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (T, H0, W0, 3)).astype(np.uint8))


def _vae_params(dim, seed=1):
    from vae_encode_ref import make_vae_encoder_params
    P = W.make_vae_params(dim, seed)
    P.update(make_vae_encoder_params(dim, seed + 100))
    return P


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
def test_declarations():
    """header and ctypes table agree on mg_video_from_u8; generate, the schedulers and the launcher have the new surface."""
    from wan.backend import lib
    from wan.text2video import WanT2V
    from wan.utils import FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler
    from wan.utils.utils import load_video
    decl = header_declarations()
    assert 'mg_video_from_u8' in decl, 'include/moviigen_hip.h does not declare mg_video_from_u8'
    restype, want = decl['mg_video_from_u8']
    assert restype is lib.c_int and lib.SIGNATURES['mg_video_from_u8'] == want
    par = inspect.signature(WanT2V.generate).parameters
    assert par['init_video'].default is None and par['strength'].default == 1.0
    assert list(par)[-2:] == ['init_video', 'strength']          # appended: every positional call of the reference keeps its meaning
    for cls in (FlowUniPCMultistepScheduler, FlowDPMSolverMultistepScheduler):
        assert callable(getattr(cls, 'set_begin_index'))
    assert callable(load_video)
    src = open(os.path.join(ROOT, 'scripts', 'inference', 'generate.py')).read()
    assert "'--init_video'" in src and "'--strength'" in src


@pytest.mark.parametrize('h0,w0,h,w', [(37, 53, 16, 24), (16, 24, 40, 64), (30, 30, 30, 30)])
def test_resize_ref_vs_torch(h0, w0, h, w):
    """the restatement is the filter F.interpolate(mode='bilinear', antialias=True, align_corners=False) computes."""
    x = (torch.from_numpy(np.random.RandomState(h0 + w).rand(2, 3, h0, w0)) * 2 - 1).float()
    ref = F.interpolate(x, size=(h, w), mode='bilinear', antialias=True, align_corners=False)
    got = resize_f64(x, h, w)
    err = (got - ref.double()).abs().max().item()
    print(f'resize_ref vs torch {h0}x{w0} -> {h}x{w}: max abs {err:.2e}')
    assert err < 1e-5
    for n_in, n_out in ((h0, h), (w0, w)):
        wt = axis_weights(n_in, n_out)
        assert (wt >= 0).all() and torch.allclose(wt.sum(1), torch.ones(n_out, dtype=torch.float64), atol=1e-14)
        assert ((wt > 0).sum(1) <= 2 * max(n_in / n_out, 1.0) + 1).all()
    if (h0, w0) == (h, w):
        assert torch.equal(got, x.double())


def test_cover_geometry():
    assert cover_geometry(37, 53, 16, 24) == (17, 24, 0, 0)
    assert cover_geometry(16, 24, 40, 64) == (43, 64, 1, 0)
    assert cover_geometry(9, 200, 8, 8) == (8, 178, 0, 85)
    assert cover_geometry(1080, 1920, 832, 1920) == (1080, 1920, 124, 0)
    assert cover_geometry(30, 31, 30, 31) == (30, 31, 0, 0)


def _cpu_lincomb(like, terms):
    acc = None
    for t, c in terms:
        v = torch.from_numpy(t.numpy().astype(np.float32) * np.float32(c))
        acc = v if acc is None else acc + v
    return acc


def _scheduler(solver, n, shift, lincomb=None, device='cpu'):
    """the scheduler and its timesteps as WanT2V.generate sets them up."""
    from wan.utils import FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, get_sampling_sigmas, retrieve_timesteps
    if solver == 'unipc':
        s = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False, lincomb=lincomb)
        s.set_timesteps(n, device=device, shift=shift)
        return s, s.timesteps
    s = FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False, lincomb=lincomb)
    ts, _ = retrieve_timesteps(s, device=device, sigmas=get_sampling_sigmas(n, shift))
    return s, ts


@pytest.mark.parametrize('solver', ['unipc', 'dpm++'])
@pytest.mark.parametrize('i0', [0, 3, 7])
def test_mid_schedule_start(solver, i0):
    """start from (1 - sigma) x0 + sigma eps at schedule index i0 with the model v = (x - x0) / sigma_i, whose x0-prediction x - sigma v
    is exact: every solver order then lands on x0 when sigma reaches 0."""
    n = 8
    s, ts = _scheduler(solver, n, 5.0, lincomb=_cpu_lincomb)
    x0, eps = W.randn((4, 3, 5, 6), 1), W.randn((4, 3, 5, 6), 2)
    sig = s.sigmas[i0].item()
    x = (1 - sig) * x0 + sig * eps
    s.set_begin_index(i0)
    steps = 0
    for i in range(i0, n):
        assert s.step_index == i
        v = (x - x0) / s.sigmas[i].item()
        x = s.step(v, int(ts[i]), x, return_dict=False)[0]
        steps += 1
    assert steps == n - i0 and s.step_index == n
    err = scale_err(x, x0)
    print(f'{solver} from index {i0}: scale_err {err:.2e}')
    assert err < 1e-5
    for bad in (-1, n):
        with pytest.raises(ValueError):
            s.set_begin_index(bad)


def test_set_begin_index_needs_a_schedule():
    from wan.utils import FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler
    for cls in (FlowUniPCMultistepScheduler, FlowDPMSolverMultistepScheduler):
        with pytest.raises(ValueError):
            cls(num_train_timesteps=1000, shift=1).set_begin_index(0)


def test_strength_to_steps():
    from wan.text2video import v2v_steps
    assert v2v_steps(50, 1) == (50, 0) and v2v_steps(50, 1.0) == (50, 0)
    assert v2v_steps(50, 0.5) == (25, 25)
    assert v2v_steps(50, 0.01) == (1, 49)
    assert v2v_steps(4, 0.5) == (2, 2) and v2v_steps(4, 0.1) == (1, 3)
    for bad in (0, 0.0, -0.5, 1.01, float('nan')):
        with pytest.raises(ValueError):
            v2v_steps(50, bad)


def test_load_video(tmp_path):
    from wan.utils.utils import load_video
    fr = _frames(3, 6, 7, 0).numpy()
    np.save(tmp_path / 'clip.npy', fr)
    got = load_video(str(tmp_path / 'clip.npy'))
    assert got.dtype == np.uint8 and np.array_equal(got, fr)
    np.save(tmp_path / 'bad.npy', fr.astype(np.float32))
    with pytest.raises(ValueError):
        load_video(str(tmp_path / 'bad.npy'))
    with pytest.raises(FileNotFoundError):
        load_video(str(tmp_path / 'missing.npy'))
    try:
        import imageio  # noqa: F401
    except ModuleNotFoundError:
        (tmp_path / 'clip.mp4').write_bytes(b'')
        with pytest.raises(ImportError, match=r'\.npy'):
            load_video(str(tmp_path / 'clip.mp4'))


# ------------------------------------------------------------------------------------------------
# GPU: the ingest kernel
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('T,h0,w0,h,w', [(2, 37, 53, 16, 24),      # down 2.2x, the crop removes a row
                                         (1, 16, 24, 40, 64),      # up-scaling
                                         (2, 30, 31, 30, 31),      # same size: bit-equal to the stated expression
                                         (1, 9, 200, 8, 8),        # extreme aspect, scale 1.1, wide crop
                                         (1, 64, 64, 8, 8),        # scale 8: 17 taps per axis
                                         (3, 45, 80, 24, 40),      # several frames and rows, 16:9 -> 5:3
                                         (1, 21, 610, 10, 300)])   # two column blocks, the second one ragged
def test_video_from_u8_vs_reference(dev, T, h0, w0, h, w):
    from wan.backend import ops
    fr = _frames(T, h0, w0, 7 * h0 + w)
    out = ops.video_from_u8(fr.to(dev), h, w, out=torch.full((3, T, h, w), float('nan'), device=dev))
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, T, h, w) and torch.isfinite(out).all().item()
    ref = video_from_u8_f64(fr, h, w)
    err = (out.double().cpu() - ref).abs().max().item()
    print(f'video_from_u8 {T}x{h0}x{w0} -> {h}x{w}: max abs {err:.2e}')
    assert err < 1e-5
    assert torch.equal(out, ops.video_from_u8(fr.to(dev), h, w))                 # one fixed summation order
    if (h0, w0) == (h, w):
        want = fr.numpy().astype(np.float32) / np.float32(127.5) - np.float32(1.0)      # the header's expression, IEEE fp32
        assert np.array_equal(out.cpu().numpy(), want.transpose(3, 0, 1, 2))


@gpu
def test_video_from_u8_rejects(dev):
    from wan.backend import lib, ops
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.video_from_u8(_frames(1, 65, 65, 0).to(dev), 8, 8)                    # 8.125x down
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.video_from_u8(_frames(1, 4, 4, 0).to(dev), 33, 32)                    # 8.25x up
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.video_from_u8(_frames(1, 8, 8, 0).to(dev), 0, 8)
    with pytest.raises(lib.MoviigenHipError):
        ops.video_from_u8(_frames(1, 8, 8, 0).to(dev).float(), 8, 8)
    with pytest.raises(lib.MoviigenHipError):
        ops.video_from_u8(_frames(1, 8, 8, 0).to(dev), 8, 8, out=torch.empty(3, 1, 8, 9, device=dev))
    ops.video_from_u8(_frames(1, 4, 4, 0).to(dev), 32, 32)                        # exactly 8x up is served
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# GPU: a bf16x3 VAE object encodes
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('dim', [8, 96])
def test_vae_encode_bf16x3_vs_exact(dev, dim):
    """WanVAE(mode='bf16x3').encode against the exact-mode encode of the same weights.  Measured on MI355X: see DESIGN 3.4a."""
    import wan
    P = _vae_params(dim)
    clip = W.randn((3, 9, 32, 32), 41).to(dev)
    exact = wan.modules.WanVAE(state_dict=P, device=dev)
    ref = exact.encode([clip])[0]
    out = wan.modules.WanVAE(state_dict=P, device=dev, mode='bf16x3').encode([clip])[0]
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(ref.shape) == (16, 3, 4, 4) and torch.isfinite(out).all().item()
    err = scale_err(out, ref)
    print(f'encode bf16x3 vs exact, dim {dim}: scale_err {err:.2e}')
    assert err < 1e-4
    assert not torch.equal(out, ref)                                             # the fast convolutions did run
    assert torch.equal(exact.encode([clip])[0], ref)                             # and the exact object is untouched by it


# ------------------------------------------------------------------------------------------------
# GPU: WanT2V.generate(init_video=, strength=)
# ------------------------------------------------------------------------------------------------
SIZE, FRAMES, STEPS = (64, 64), 5, 4


@pytest.fixture(scope='module')
def pipe(dev):
    import wan
    from wan.configs import Config
    cfg = W.TINY_DIT
    model = wan.modules.WanModel(**cfg)
    model.load_state_dict(W.make_dit_params(cfg, 0))
    vae = wan.modules.WanVAE(state_dict=_vae_params(8), device=dev)
    conf = Config(num_train_timesteps=1000, param_dtype=torch.bfloat16, vae_stride=(4, 8, 8), patch_size=(1, 2, 2), sample_neg_prompt='',
                  vae_checkpoint='', text_len=cfg['text_len'])
    return wan.WanT2V(conf, '', device_id=0, model=model, vae=vae)


def _call(pipe, solver, **kw):
    ctx, ctx_null = W.randn((9, W.TINY_DIT['text_dim']), 31), W.randn((5, W.TINY_DIT['text_dim']), 32)
    return pipe.generate(ctx, size=SIZE, frame_num=FRAMES, shift=5.0, sample_solver=solver, sampling_steps=STEPS, guide_scale=5.0, n_prompt=ctx_null,
                         seed=0, offload_model=False, noise=W.randn((16, 2, 8, 8), 33), **kw)


@gpu
@pytest.mark.parametrize('solver', ['unipc', 'dpm++'])
def test_generate_init_video_half_strength(dev, pipe, solver, monkeypatch):
    from wan.backend import ops
    frames = _frames(7, 50, 70, 5)                                                # another size, more frames than frame_num
    noise = W.randn((16, 2, 8, 8), 33).to(dev)
    seen, starts = [], []
    inner = pipe.start_latent

    def spy(init_video, size, frame_num, noise_, sigma):
        lat = inner(init_video, size, frame_num, noise_, sigma)
        starts.append((sigma, lat.clone()))
        return lat
    monkeypatch.setattr(pipe, 'start_latent', spy)
    video = _call(pipe, solver, init_video=frames, strength=0.5, callback=lambda i, l: seen.append(i))
    assert seen == [2, 3]                                                         # 2 of the 4 steps ran: schedule indices 2 and 3
    assert tuple(video.shape) == (3, FRAMES, SIZE[1], SIZE[0]) and video.dtype == torch.float32 and torch.isfinite(video).all().item()
    # the start latent, rebuilt in torch from the public pieces
    sched, _ = _scheduler(solver, STEPS, 5.0)
    sig2 = sched.sigmas[2].item()
    assert len(starts) == 1 and starts[0][0] == sig2
    clip = ops.video_from_u8(frames[:FRAMES].to(dev), SIZE[1], SIZE[0])
    z0 = pipe.vae.encode([clip])[0]
    want = (1 - sig2) * z0 + sig2 * noise
    err = scale_err(starts[0][1], want)
    print(f'{solver}: start latent vs torch rebuild {err:.2e}')
    assert err < 1e-6
    # a float clip already at `size` is taken as it is; numpy frames are accepted
    assert torch.equal(pipe.start_latent(clip, SIZE, FRAMES, noise, sig2), starts[0][1])
    assert torch.equal(pipe.start_latent(frames.numpy(), SIZE, FRAMES, noise, sig2), starts[0][1])
    assert torch.equal(video, _call(pipe, solver, init_video=clip.cpu(), strength=0.5))


@gpu
@pytest.mark.parametrize('solver', ['unipc', 'dpm++'])
def test_generate_full_strength_and_plain_call(dev, pipe, solver):
    plain = _call(pipe, solver)
    assert torch.equal(_call(pipe, solver, init_video=None, strength=1.0), plain)
    seen = []
    full = _call(pipe, solver, init_video=_frames(FRAMES, 50, 70, 5), strength=1.0, callback=lambda i, l: seen.append(i))
    assert seen == [0, 1, 2, 3]
    assert torch.equal(full, plain)                                               # 0 x z0 + 1 x noise: the plain start, bit for bit


@gpu
def test_generate_init_video_rejects(dev, pipe):
    with pytest.raises(ValueError, match='strength'):
        _call(pipe, 'unipc', init_video=_frames(FRAMES, 50, 70, 5), strength=0.0)
    with pytest.raises(ValueError, match='strength'):
        _call(pipe, 'unipc', strength=0.5)                                        # nothing to start from
    with pytest.raises(ValueError, match='init_video'):
        _call(pipe, 'unipc', init_video=_frames(FRAMES - 1, 50, 70, 5), strength=0.5)          # too few frames
    with pytest.raises(ValueError, match='init_video'):
        _call(pipe, 'unipc', init_video=torch.zeros(3, FRAMES, 32, 64), strength=0.5)          # a float clip at another size
