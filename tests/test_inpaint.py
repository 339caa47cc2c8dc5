"""Masked video-to-video, WanT2V.inpaint (mask, keep_frames): the four device passes mg_mask_from_u8, mg_mask_to_latent_u8,
mg_masked_renoise_f32, mg_mask_composite_f32 and the method itself.

CPU: the declarations, load_mask, the restatements of tests/mask_ref.py against brute-force loops.
GPU: mask_from_u8 against the fp64 restatement — the kernel's sum r carries the ingest's error, <= 1e-5 on [-1, 1] = 1.3e-3 on the byte scale,
so pixels whose fp64 r lies within 2e-3 of the threshold 127.5 are left out (at most 0.5 % of a case; on these inputs none is); the other
three passes bit for bit against torch.where / the plain-loop restatement; inpaint on the tiny pipeline of tests/test_v2v.py.
"""
import inspect
import os

import numpy as np
import pytest
import torch

import weights as W
from abi_ref import header_declarations
from mask_ref import latent_footprint, mask_from_u8_ref, mask_to_latent_ref

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mg_mask_from_u8', 'mg_mask_to_latent_u8', 'mg_masked_renoise_f32', 'mg_mask_composite_f32')
STRIDE = (4, 8, 8)


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _frames(T, H0, W0, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (T, H0, W0, 3)).astype(np.uint8))


def _vae_params(dim, seed=1):
    from vae_encode_ref import make_vae_encoder_params
    P = W.make_vae_params(dim, seed)
    P.update(make_vae_encoder_params(dim, seed + 100))
    return P


def _random_mask(T, h0, w0, w):
    return torch.from_numpy(np.random.RandomState(h0 + w).randint(0, 256, (T, h0, w0)).astype(np.uint8))


def _rect_mask(T, h0, w0):
    m = torch.zeros(T, h0, w0, dtype=torch.uint8)
    m[:, h0 // 3:, w0 // 4:3 * w0 // 4] = 255
    return m


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
def test_declarations():
    """header and ctypes table agree on the four functions; generate keeps its signature, inpaint and the launcher have the new surface."""
    from wan.backend import lib
    from wan.text2video import WanT2V
    decl = header_declarations()
    for name in NAMES:
        assert name in decl, f'include/moviigen_hip.h does not declare {name}'
        restype, want = decl[name]
        assert restype is lib.c_int and lib.SIGNATURES[name] == want, name
    par = inspect.signature(WanT2V.generate).parameters
    assert list(par)[-2:] == ['init_video', 'strength'] and par['init_video'].default is None and par['strength'].default == 1.0
    par = inspect.signature(WanT2V.inpaint).parameters
    assert list(par)[:3] == ['self', 'input_prompt', 'init_video']
    assert par['mask'].default is None and par['keep_frames'].default == 0 and par['strength'].default == 1.0
    src = open(os.path.join(ROOT, 'scripts', 'inference', 'generate.py')).read()
    assert "'--mask'" in src and "'--keep_frames'" in src


def test_launcher_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location('mg_generate_inpaint', os.path.join(ROOT, 'scripts', 'inference', 'generate.py'))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    a = g._parse_args(['--ckpt_dir', '/x', '--init_video', 'c.npy', '--mask', 'm.npy', '--keep_frames', '5'])
    assert a.mask == 'm.npy' and a.keep_frames == 5
    a = g._parse_args(['--ckpt_dir', '/x'])
    assert a.mask is None and a.keep_frames == 0
    for bad in (['--mask', 'm.npy'], ['--keep_frames', '3'], ['--init_video', 'c.npy', '--keep_frames', '82'],
                ['--init_video', 'c.npy', '--keep_frames', '-1']):
        with pytest.raises(AssertionError):
            g._parse_args(['--ckpt_dir', '/x'] + bad)


def test_launcher_routes_to_inpaint(tmp_path, monkeypatch):
    """generate.py calls WanT2V.inpaint with the loaded mask when --mask / --keep_frames are given, WanT2V.generate otherwise (a recording pipeline)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('mg_generate_inpaint_run', os.path.join(ROOT, 'scripts', 'inference', 'generate.py'))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    calls = []

    class Pipe:
        last_step_plan = None

        def __init__(self, **kw):
            pass

        def generate(self, prompt, **kw):
            calls.append(('generate', kw))
            return torch.zeros(3, 5, 8, 8)

        def inpaint(self, prompt, **kw):
            calls.append(('inpaint', kw))
            return torch.zeros(3, 5, 8, 8)
    monkeypatch.setattr(g.wan, 'WanT2V', Pipe)
    monkeypatch.setattr(g, 'cache_video', lambda **kw: kw['save_file'])
    frames, mask = _frames(5, 6, 7, 0).numpy(), np.random.RandomState(1).randint(0, 256, (6, 7)).astype(np.uint8)
    np.save(tmp_path / 'clip.npy', frames)
    np.save(tmp_path / 'mask.npy', mask)
    base = ['--ckpt_dir', '/x', '--frame_num', '5', '--save_file', str(tmp_path / 'out.mp4'), '--init_video', str(tmp_path / 'clip.npy')]
    g.generate(g._parse_args(base + ['--strength', '0.5']))
    g.generate(g._parse_args(base + ['--mask', str(tmp_path / 'mask.npy')]))
    g.generate(g._parse_args(base + ['--keep_frames', '1', '--strength', '0.5']))
    assert [c[0] for c in calls] == ['generate', 'inpaint', 'inpaint']
    assert 'mask' not in calls[0][1] and 'keep_frames' not in calls[0][1] and calls[0][1]['strength'] == 0.5
    assert np.array_equal(calls[1][1]['mask'], mask) and calls[1][1]['keep_frames'] == 0 and np.array_equal(calls[1][1]['init_video'], frames)
    assert calls[2][1]['mask'] is None and calls[2][1]['keep_frames'] == 1 and calls[2][1]['strength'] == 0.5
    WanT2V = __import__('wan.text2video', fromlist=['WanT2V']).WanT2V
    for _, kw in calls[1:]:                                    # every keyword the launcher passes is one inpaint takes
        inspect.signature(WanT2V.inpaint).bind(None, 'prompt', **{k: v for k, v in kw.items() if k in ('init_video', 'mask', 'keep_frames', 'strength')})
        inspect.signature(WanT2V.generate).bind(None, 'prompt', **{k: v for k, v in kw.items() if k not in ('mask', 'keep_frames')})


def test_load_mask(tmp_path):
    from wan.utils.utils import load_mask
    m3 = np.random.RandomState(0).randint(0, 256, (3, 6, 7)).astype(np.uint8)
    np.save(tmp_path / 'm3.npy', m3)
    np.save(tmp_path / 'm2.npy', m3[0])
    for name, want in (('m3.npy', m3), ('m2.npy', m3[0])):
        got = load_mask(str(tmp_path / name))
        assert got.dtype == np.uint8 and np.array_equal(got, want)
    np.save(tmp_path / 'float.npy', m3.astype(np.float32))
    np.save(tmp_path / 'rgb.npy', np.zeros((2, 6, 7, 3), np.uint8))
    for bad in ('float.npy', 'rgb.npy'):
        with pytest.raises(ValueError):
            load_mask(str(tmp_path / bad))
    with pytest.raises(FileNotFoundError):
        load_mask(str(tmp_path / 'missing.npy'))
    try:
        import imageio  # noqa: F401
    except ModuleNotFoundError:
        (tmp_path / 'mask.mp4').write_bytes(b'')
        with pytest.raises(ImportError, match=r'\.npy'):
            load_mask(str(tmp_path / 'mask.mp4'))


def test_load_mask_from_frames(tmp_path, monkeypatch):
    """a file load_video reads: the per-pixel maximum over the three channels"""
    from wan.utils import utils
    fr = _frames(2, 5, 6, 3).numpy()
    monkeypatch.setattr(utils, 'load_video', lambda path: fr)
    (tmp_path / 'mask.mp4').write_bytes(b'')
    got = utils.load_mask(str(tmp_path / 'mask.mp4'))
    assert got.dtype == np.uint8 and got.shape == (2, 5, 6) and np.array_equal(got, fr.max(axis=3)) and got.flags['C_CONTIGUOUS']


def test_footprint_vs_brute_force():
    """mask_to_latent_ref against the plain loop over latent_footprint; latent frame 0 reads pixel frame 0 only."""
    st, sh, sw = 4, 2, 3
    assert [list(r) for r in latent_footprint(0, 1, 2, st, sh, sw)] == [[0], [2, 3], [6, 7, 8]]
    assert [list(r) for r in latent_footprint(2, 0, 0, st, sh, sw)] == [[5, 6, 7, 8], [0, 1], [0, 1, 2]]
    T, H, Wd = 9, 6, 9
    pm = torch.from_numpy((np.random.RandomState(1).rand(T, H, Wd) < 0.04).astype(np.uint8))
    got = mask_to_latent_ref(pm, st, sh, sw)
    assert tuple(got.shape) == (3, 3, 3) and 0 < int(got.sum()) < got.numel()
    for j in range(3):
        for y in range(3):
            for x in range(3):
                fr, rows, cols = latent_footprint(j, y, x, st, sh, sw)
                want = int(any(pm[t, r, c] for t in fr for r in rows for c in cols))
                assert int(got[j, y, x]) == want, (j, y, x)
    # every pixel frame belongs to exactly one latent frame
    owner = [j for t in range(T) for j in range(3) if t in latent_footprint(j, 0, 0, st, sh, sw)[0]]
    assert owner == [0, 1, 1, 1, 1, 2, 2, 2, 2]
    one = torch.zeros(T, H, Wd, dtype=torch.uint8)
    one[1, 0, 0] = 7                                        # pixel frame 1: latent frame 1, not 0
    lm = mask_to_latent_ref(one, st, sh, sw)
    assert int(lm.sum()) == 1 and int(lm[1, 0, 0]) == 1


def test_mask_ref_equal_size():
    m = _random_mask(2, 30, 31, 31)
    pm, r = mask_from_u8_ref(m, 2, 30, 31)
    assert torch.equal(r, m.double()) and torch.equal(pm, (m >= 128).to(torch.uint8))
    pm1, _ = mask_from_u8_ref(m, 2, 30, 31, keep_frames=1)
    assert not pm1[0].any() and torch.equal(pm1[1], pm[1])
    pm_b, _ = mask_from_u8_ref(m[:1], 3, 30, 31)           # one mask for every frame
    assert tuple(pm_b.shape) == (3, 30, 31) and all(torch.equal(pm_b[t], pm[0]) for t in range(3))


# ------------------------------------------------------------------------------------------------
# GPU: mg_mask_from_u8
# ------------------------------------------------------------------------------------------------
MASK_SHAPES = [(2, 37, 53, 16, 24), (1, 16, 24, 40, 64), (2, 30, 31, 30, 31), (1, 9, 200, 8, 8), (1, 64, 64, 8, 8), (2, 50, 70, 64, 64),
               (1, 33, 300, 24, 272)]


@gpu
@pytest.mark.parametrize('kind', ['random', 'rect'])
@pytest.mark.parametrize('T,h0,w0,h,w', MASK_SHAPES)
def test_mask_from_u8_vs_reference(dev, T, h0, w0, h, w, kind):
    from wan.backend import ops
    mask = _random_mask(T, h0, w0, w) if kind == 'random' else _rect_mask(T, h0, w0)
    out = ops.mask_from_u8(mask.to(dev), T, h, w, out=torch.full((T, h, w), 0xFF, dtype=torch.uint8, device=dev))
    assert out.dtype == torch.uint8 and tuple(out.shape) == (T, h, w)
    got = out.cpu()
    assert int(got.max()) <= 1                                                    # every byte written, 0 or 1
    want, r = mask_from_u8_ref(mask, T, h, w)
    near = (r - 127.5).abs() < 2e-3
    print(f'mask_from_u8 {kind} {T}x{h0}x{w0} -> {h}x{w}: {int(near.sum())} of {near.numel()} pixels within 2e-3 of the threshold, '
          f'{int((got != want)[~near].sum())} others differ, {int(want.sum())} set')
    assert near.double().mean().item() <= 0.005
    assert torch.equal(got[~near], want[~near])
    assert torch.equal(out, ops.mask_from_u8(mask.to(dev), T, h, w))
    if (h0, w0) == (h, w):
        assert torch.equal(got, (mask >= 128).to(torch.uint8))                    # bit-exact at equal size


@gpu
def test_mask_from_u8_frames(dev):
    """Tm = 1 is the mask expanded to T frames; keep_frames zeroes exactly the first frames."""
    from wan.backend import ops
    T, h0, w0, h, w = 3, 37, 53, 16, 24
    one = _random_mask(1, h0, w0, w).to(dev)
    full = ops.mask_from_u8(one.expand(T, h0, w0).contiguous(), T, h, w)
    assert torch.equal(ops.mask_from_u8(one, T, h, w), full) and 0 < int(full.sum()) < full.numel()
    longer = torch.cat([one.expand(T, h0, w0), 255 - one.expand(2, h0, w0)]).contiguous()        # Tm > T: the first T frames are read
    assert torch.equal(ops.mask_from_u8(longer, T, h, w), full)
    ones = torch.full((T, h0, w0), 255, dtype=torch.uint8, device=dev)
    for k in (0, 1, T):
        pm = ops.mask_from_u8(ones, T, h, w, keep_frames=k)
        assert not pm[:k].any().item() and (pm[k:] == 1).all().item(), k


@gpu
def test_mask_from_u8_rejects(dev):
    from wan.backend import lib, ops
    m = torch.zeros(2, 8, 8, dtype=torch.uint8, device=dev)
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.mask_from_u8(m, 3, 8, 8)                                              # Tm = 2 with T = 3
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.mask_from_u8(m, 2, 8, 8, keep_frames=3)                               # keep_frames = T + 1
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.mask_from_u8(m, 2, 8, 8, keep_frames=-1)
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.mask_from_u8(torch.zeros(1, 65, 65, dtype=torch.uint8, device=dev), 1, 8, 8)          # 8.125x down
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.mask_from_u8(torch.zeros(1, 4, 4, dtype=torch.uint8, device=dev), 1, 33, 32)          # 8.25x up
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.mask_from_u8(m, 2, 0, 8)
    with pytest.raises(lib.MoviigenHipError):
        ops.mask_from_u8(m.float(), 2, 8, 8)                                      # a float mask
    ops.mask_from_u8(m, 2, 8, 8, keep_frames=2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# GPU: mg_mask_to_latent_u8
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('T,H,Wd', [(5, 16, 24), (1, 8, 8), (9, 64, 320)])
def test_mask_to_latent_vs_reference(dev, T, H, Wd):
    from wan.backend import ops
    st, sh, sw = STRIDE
    rs = np.random.RandomState(T + Wd)
    for density in (0.002, 0.5):
        pm = torch.from_numpy((rs.rand(T, H, Wd) < density).astype(np.uint8) * rs.randint(1, 256, (T, H, Wd)).astype(np.uint8))
        lm = ops.mask_to_latent(pm.to(dev), STRIDE)
        assert lm.dtype == torch.uint8 and torch.equal(lm.cpu(), mask_to_latent_ref(pm, st, sh, sw))
    # one set pixel in each corner of a footprint, in the first and the last frame of a group: exactly that latent cell is set
    Tl, Hl, Wl = (T - 1) // st + 1, H // sh, Wd // sw
    for (j, y, x) in {(0, 0, 0), (Tl - 1, Hl - 1, Wl - 1), (Tl - 1, 0, Wl - 1), (min(1, Tl - 1), Hl - 1, 0)}:
        fr, rows, cols = latent_footprint(j, y, x, st, sh, sw)
        for t in {fr[0], fr[-1]}:
            for r in (rows[0], rows[-1]):
                for c in (cols[0], cols[-1]):
                    pm = torch.zeros(T, H, Wd, dtype=torch.uint8)
                    pm[t, r, c] = 1
                    lm = ops.mask_to_latent(pm.to(dev), STRIDE).cpu()
                    assert int(lm.sum()) == 1 and int(lm[j, y, x]) == 1, (j, y, x, t, r, c)


@gpu
def test_mask_to_latent_keep_frames_and_rejects(dev):
    from wan.backend import lib, ops
    pm = ops.mask_from_u8(torch.full((1, 16, 24), 255, dtype=torch.uint8, device=dev), 5, 16, 24, keep_frames=3)
    lm = ops.mask_to_latent(pm, STRIDE)
    assert tuple(lm.shape) == (2, 2, 3) and not lm[0].any().item() and (lm[1] == 1).all().item()      # frames 3, 4 are under latent frame 1
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.mask_to_latent(torch.zeros(4, 16, 24, dtype=torch.uint8, device=dev), STRIDE)             # T = 4
    with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
        ops.mask_to_latent(torch.zeros(5, 12, 24, dtype=torch.uint8, device=dev), STRIDE)             # H = 12
    with pytest.raises(lib.MoviigenHipError):
        ops.mask_to_latent(torch.zeros(5, 16, 24, device=dev), STRIDE)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# GPU: mg_masked_renoise_f32, mg_mask_composite_f32
# ------------------------------------------------------------------------------------------------
def _lm_cases(n, dev, seed):
    rnd = torch.from_numpy((np.random.RandomState(seed).rand(n) < 0.5).astype(np.uint8) * np.uint8(200)).to(dev)      # non-zero, not 1
    return {'keep': torch.zeros(n, dtype=torch.uint8, device=dev), 'regen': torch.ones(n, dtype=torch.uint8, device=dev), 'random': rnd}


@gpu
@pytest.mark.parametrize('thw', [128,          # 16-byte groups only
                                 105,          # not a multiple of 4: groups straddle the channel boundary, the mask is read byte by byte
                                 140000,       # 2.24 M elements > 8192 x 256: more elements than threads
                                 525000])      # 2.1 M groups of four > 8192 x 256 threads: the grid-stride loop of the 16-byte path runs twice
def test_masked_renoise(dev, thw):
    from wan.backend import ops
    C = 16
    lat0, z0, noise = (W.randn((C, thw), s).to(dev) for s in (1, 2, 3))
    for sigma in (0.0, 0.6247, 1.0):
        fresh = ops.lincomb(torch.empty_like(z0), [(z0, 1.0 - sigma), (noise, sigma)])
        for name, lm in _lm_cases(thw, dev, thw).items():
            got = ops.masked_renoise(lat0.clone(), z0, noise, lm, 1.0 - sigma, sigma)
            assert torch.equal(got, torch.where(lm.bool(), lat0, fresh)), (sigma, name)
    # a select, not a multiply: NaN on the side not chosen does not leak
    lm = _lm_cases(thw, dev, thw)['random']
    regen = lm.bool().expand(C, thw)
    nan = torch.tensor(float('nan'), device=dev)
    lat_n, z0_n = torch.where(regen, lat0, nan), torch.where(regen, nan, z0)      # NaN in latent at kept cells, in z0 at regenerated cells
    got = ops.masked_renoise(lat_n.clone(), z0_n, noise, lm, 0.3753, 0.6247)
    assert torch.isfinite(got).all().item()
    assert torch.equal(got, torch.where(regen, lat0, ops.lincomb(torch.empty_like(z0), [(z0, 0.3753), (noise, 0.6247)])))


@gpu
@pytest.mark.parametrize('thw', [105, 140000])      # 140000: 2.24 M elements > 8192 x 256 threads, the element loop runs twice
def test_masked_renoise_unaligned_and_rejects(dev, thw):
    """tensors that do not start on a 16-byte boundary take the element-by-element path: the same bits"""
    from wan.backend import lib, ops
    C = 16
    base = [W.randn((C * thw + 1,), s).to(dev) for s in (1, 2, 3)]
    lat0, z0, noise = (b[1:].view(C, thw) for b in base)
    assert lat0.data_ptr() % 16 == 4 and lat0.is_contiguous()
    lm = _lm_cases(thw, dev, 5)['random']
    got_buf = base[0].clone()
    ops.masked_renoise(got_buf[1:].view(C, thw), z0, noise, lm, 0.25, 0.75)
    fresh = ops.lincomb(torch.empty(C, thw, device=dev), [(z0.clone(), 0.25), (noise.clone(), 0.75)])
    assert torch.equal(got_buf[1:].view(C, thw), torch.where(lm.bool(), lat0, fresh)) and got_buf[0].item() == base[0][0].item()
    with pytest.raises(lib.MoviigenHipError):
        ops.masked_renoise(lat0.clone(), z0, noise, lm[:-1], 0.25, 0.75)
    with pytest.raises(lib.MoviigenHipError):
        ops.masked_renoise(lat0.clone(), z0, noise, lm.float(), 0.25, 0.75)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize('H,Wd', [(64, 64), (33, 31)])
def test_mask_composite(dev, H, Wd):
    from wan.backend import lib, ops
    T = 5
    video, src = W.randn((3, T, H, Wd), 4).to(dev), W.randn((3, T, H, Wd), 5).to(dev)
    for name, pm in _lm_cases(T * H * Wd, dev, H).items():
        pm = pm.view(T, H, Wd)
        got = ops.mask_composite(video.clone(), src, pm)
        assert torch.equal(got, torch.where(pm.bool(), video, src)), name
    regen = pm.bool().expand(3, T, H, Wd)
    nan = torch.tensor(float('nan'), device=dev)
    got = ops.mask_composite(torch.where(regen, video, nan), torch.where(regen, nan, src), pm)
    assert torch.isfinite(got).all().item() and torch.equal(got, torch.where(regen, video, src))
    with pytest.raises(lib.MoviigenHipError):
        ops.mask_composite(video.clone(), src, pm[:-1])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# GPU: WanT2V.inpaint on the tiny pipeline of tests/test_v2v.py
# ------------------------------------------------------------------------------------------------
SIZE, FRAMES, STEPS = (64, 64), 5, 4
SOLVERS = ['unipc', 'dpm++']


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


@pytest.fixture(scope='module')
def source(dev, pipe):
    """(frames, clip, z0, noise): computed once, never written"""
    from wan.backend import ops
    frames = _frames(7, 50, 70, 5)
    clip = ops.video_from_u8(frames[:FRAMES].to(dev), SIZE[1], SIZE[0])
    return frames, clip, pipe.vae.encode([clip])[0], W.randn((16, 2, 8, 8), 33).to(dev)


def _kw(solver, **kw):
    ctx_null = W.randn((5, W.TINY_DIT['text_dim']), 32)
    return dict(size=SIZE, frame_num=FRAMES, shift=5.0, sample_solver=solver, sampling_steps=STEPS, guide_scale=5.0, n_prompt=ctx_null,
                seed=0, offload_model=False, noise=W.randn((16, 2, 8, 8), 33), **kw)


def _ctx():
    return W.randn((9, W.TINY_DIT['text_dim']), 31)


def _sigmas(pipe, solver):
    return pipe._scheduler(solver, STEPS, 5.0)[0].sigmas.tolist()


def _left_half():
    mask = torch.zeros(50, 70, dtype=torch.uint8)
    mask[:, :35] = 255
    return mask


def _masks(dev, mask, keep_frames=0):
    from wan.backend import ops
    m = torch.full((1, SIZE[1], SIZE[0]), 255, dtype=torch.uint8) if mask is None else mask.view(-1, *mask.shape[-2:])
    pm = ops.mask_from_u8(m.to(dev), FRAMES, SIZE[1], SIZE[0], keep_frames)
    return pm, ops.mask_to_latent(pm, STRIDE)


def _check_kept_cells(seen, sigmas, z0, noise, lm):
    """at every callback(i, latent) the kept cells hold (1 - sigma_{i+1}) z0 + sigma_{i+1} noise, the bits of ops.lincomb"""
    from wan.backend import ops
    kept = (lm == 0).expand_as(z0)
    assert kept.any().item() and not kept.all().item()
    for i, latent in seen:
        s = sigmas[i + 1]
        want = ops.lincomb(torch.empty_like(z0), [(z0, 1.0 - s), (noise, s)])
        assert torch.equal(latent[kept], want[kept]), i
    assert sigmas[seen[-1][0] + 1] == 0.0 and torch.equal(seen[-1][1][kept], z0[kept])


@gpu
@pytest.mark.parametrize('solver', SOLVERS)
def test_inpaint_all_regenerate_is_generate(dev, pipe, source, solver):
    frames = source[0]
    mask = torch.full((50, 70), 255, dtype=torch.uint8)
    half = pipe.inpaint(_ctx(), frames, mask=mask, **_kw(solver, strength=0.5))
    assert torch.equal(half, pipe.generate(_ctx(), **_kw(solver, init_video=frames, strength=0.5)))
    full = pipe.inpaint(_ctx(), frames, mask=mask.bool().numpy(), **_kw(solver))            # a bool array, strength 1
    assert torch.equal(full, pipe.generate(_ctx(), **_kw(solver)))
    assert not torch.equal(full, half)


@gpu
@pytest.mark.parametrize('solver', SOLVERS)
def test_inpaint_all_keep_is_the_source(dev, pipe, source, solver):
    frames, clip, z0, _ = source
    seen = []
    video = pipe.inpaint(_ctx(), frames, mask=torch.zeros(1, 50, 70, dtype=torch.uint8), **_kw(solver, callback=lambda i, l: seen.append((i, l.clone()))))
    assert [i for i, _ in seen] == [0, 1, 2, 3]
    assert torch.equal(video, clip)
    assert torch.equal(seen[-1][1], z0)


@gpu
@pytest.mark.parametrize('solver', SOLVERS)
def test_inpaint_left_half(dev, pipe, source, solver):
    frames, clip, z0, noise = source
    pm, lm = _masks(dev, _left_half())
    seen = []
    video = pipe.inpaint(_ctx(), frames, mask=_left_half(), **_kw(solver, callback=lambda i, l: seen.append((i, l.clone()))))
    assert [i for i, _ in seen] == [0, 1, 2, 3]
    _check_kept_cells(seen, _sigmas(pipe, solver), z0, noise, lm)
    last = seen[-1][1]
    regen = (lm != 0).expand_as(z0)
    assert not torch.equal(last[regen], z0[regen])
    kept_px = (pm == 0).expand_as(video)
    assert kept_px.any().item() and not kept_px.all().item()
    assert torch.equal(video[kept_px], clip[kept_px])
    assert torch.equal(video[~kept_px], pipe.vae.decode([last])[0][~kept_px])
    assert torch.isfinite(video).all().item() and tuple(video.shape) == (3, FRAMES, SIZE[1], SIZE[0])


@gpu
@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('solver', SOLVERS)
def test_inpaint_keep_frames(dev, pipe, source, solver, k):
    frames, clip, z0, noise = source
    seen = []
    video = pipe.inpaint(_ctx(), frames, keep_frames=k, **_kw(solver, callback=lambda i, l: seen.append((i, l.clone()))))
    last = seen[-1][1]
    assert torch.equal(video[:, :k], clip[:, :k])                                 # pixel frames < k are the clip's
    assert not torch.equal(video[:, k:], clip[:, k:])
    assert torch.equal(last[:, 0], z0[:, 0])                                      # latent frame 0 = pixel frame 0 alone: kept for every k >= 1
    assert not torch.equal(last[:, 1], z0[:, 1])                                  # latent frame 1 holds a regenerated frame (3 or 4): regenerated,
    #                                                                               while for k = 3 pixel frames 1 and 2 still equal the clip (above)
    _check_kept_cells(seen, _sigmas(pipe, solver), z0, noise, _masks(dev, None, k)[1])


@gpu
def test_inpaint_with_step_cache(dev, pipe, source):
    frames, _, z0, noise = source
    seen = []
    video = pipe.inpaint(_ctx(), frames, mask=_left_half(), **_kw('unipc', step_cache=[True, False, True, False],
                                                                   callback=lambda i, l: seen.append((i, l.clone()))))
    assert pipe.last_step_plan == [True, False, True, False] and [i for i, _ in seen] == [0, 1, 2, 3]
    assert torch.isfinite(video).all().item()
    _check_kept_cells(seen, _sigmas(pipe, 'unipc'), z0, noise, _masks(dev, _left_half())[1])


@gpu
def test_inpaint_rejects(dev, pipe, source):
    frames = source[0]
    ok = torch.zeros(50, 70, dtype=torch.uint8)
    with pytest.raises(ValueError, match='mask'):
        pipe.inpaint(_ctx(), frames, **_kw('unipc'))                              # no mask and keep_frames = 0
    with pytest.raises(ValueError, match='mask'):
        pipe.inpaint(_ctx(), frames, mask=torch.zeros(64, 64, dtype=torch.uint8), **_kw('unipc'))     # another spatial size
    with pytest.raises(ValueError, match='mask'):
        pipe.inpaint(_ctx(), frames, mask=torch.zeros(3, 50, 70, dtype=torch.uint8), **_kw('unipc'))  # Tm = 3
    with pytest.raises(ValueError, match='init_video'):
        pipe.inpaint(_ctx(), None, mask=ok, **_kw('unipc'))
    with pytest.raises(ValueError, match='keep_frames'):
        pipe.inpaint(_ctx(), frames, mask=ok, keep_frames=6, **_kw('unipc'))
    with pytest.raises(ValueError, match='mask'):
        pipe.inpaint(_ctx(), frames, mask=torch.zeros(50, 70), **_kw('unipc'))    # a float mask
    with pytest.raises(ValueError, match='mask'):
        pipe.inpaint(_ctx(), source[1].cpu(), mask=ok, **_kw('unipc'))            # a float clip: the mask must be at `size`
