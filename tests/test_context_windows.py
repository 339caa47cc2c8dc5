"""Context windows of WanT2V.generate (windows=ContextWindows(...)): the host plan wan/utils/context_windows.py, the two device
passes mg_window_gather_f32 / mg_window_blend_f32 and the sampling loop.

CPU: the plan's properties, its argument checks, the declarations, the launcher flags.
GPU: the gather bit for bit against the slice; the blend, whole tensor, against tests/context_windows_ref.py in fp64 with the same fp32
weights, within K 2^-24 sum_k w_k |v_k| per element (K = the windows that cover the frame: one rounding per product or fma);
WanT2V.generate / inpaint on the tiny pipeline of tests/test_guidance.py.
"""
import importlib.util
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

import weights as W
from abi_ref import header_declarations
from context_windows_ref import blend_once_ref, blend_ref, gather_ref

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mg_window_gather_f32', 'mg_window_blend_f32')
ST = 4                                                  # the VAE's temporal stride: pixel frames = ST (latent frames - 1) + 1
PLAN_CASES = [(7, 3, 1), (7, 4, 2), (9, 4, 3), (6, 3, 0), (41, 21, 4)]      # (F, Fw, O) in latent frames
FUSES = ['pyramid', 'flat']
NAN_BITS = 0x7fc00123                                   # what an accumulator without an initial value may hold


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _windows(Fw, O, fuse='pyramid'):
    from wan.utils.context_windows import ContextWindows
    return ContextWindows(frames=ST * (Fw - 1) + 1, overlap=ST * O, fuse=fuse)


# ------------------------------------------------------------------------------------------------
# CPU: the plan
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fuse', FUSES)
@pytest.mark.parametrize('F,Fw,O', PLAN_CASES)
def test_plan_properties(F, Fw, O, fuse):
    cw = _windows(Fw, O, fuse)
    assert (cw.Fw, cw.O) == (Fw, O)
    plan = cw.plan(F)
    starts = plan.starts
    assert all(0 <= f0 and f0 + Fw <= F for f0 in starts)                               # every window has Fw frames inside [0, F)
    assert all(a < b for a, b in zip(starts, starts[1:])) and starts[-1] == F - Fw and starts[0] == 0
    assert starts[:-1] == [k * (Fw - O) for k in range(len(starts) - 1)] and (len(starts) - 1) * (Fw - O) + Fw >= F
    assert tuple(plan.weights.shape) == (len(starts), Fw) == tuple(plan.first.shape)
    assert plan.weights.dtype == torch.float32 and plan.first.dtype == torch.uint8
    raw = [min(j + 1, Fw - j) if fuse == 'pyramid' else 1 for j in range(Fw)]
    for f in range(F):
        cover = [k for k, f0 in enumerate(starts) if f0 <= f < f0 + Fw]
        assert cover and cover == plan.cover(f), f                                      # every frame is covered
        assert [int(plan.first[k, f - starts[k]]) for k in cover] == [1] + [0] * (len(cover) - 1), f      # the earliest window, and it alone, has `first`
        w64 = [plan.weights64[k][f - starts[k]] for k in cover]
        den = sum(raw[f - starts[k]] for k in cover)
        assert w64 == [raw[f - starts[k]] / den for k in cover], f
        assert abs(sum(w64) - 1.0) <= 1e-15, f
        assert [float(plan.weights[k, f - starts[k]]) for k in cover] == [float(np.float32(v)) for v in w64], f     # rounded once
        if len(cover) == 1:
            assert plan.weights[cover[0], f - starts[cover[0]]].item() == 1.0, f
    again = _windows(Fw, O, fuse).plan(F)                                               # a function of (F, Fw, O, fuse) alone
    assert again.starts == starts and torch.equal(again.weights, plan.weights) and torch.equal(again.first, plan.first)


def test_plan_end_aligned_window_makes_three_cover_one_frame():
    """(9, 4, 3): the windows step by one frame and the end-aligned last window at 5 is the next regular one: frames 3, 4 and 5 lie in four
    windows, so more than two cover a frame.  (7, 4, 2) is the case where the end-aligned window is an EXTRA one: the regular starts are
    0 and 2, the last window starts at 3 and frame 3 lies in all three."""
    plan = _windows(4, 3).plan(9)
    assert plan.starts == [0, 1, 2, 3, 4, 5]
    assert max(len(plan.cover(f)) for f in range(9)) >= 3 and len(plan.cover(3)) == 4
    plan = _windows(4, 2).plan(7)
    assert plan.starts == [0, 2, 3] and plan.cover(3) == [0, 1, 2] and len(plan.cover(2)) == 2
    # pyramid, frame 3: raw weights 1 (window 0, j = 3), 2 (window 1, j = 1), 1 (window 2, j = 0)
    assert [plan.weights64[k][3 - plan.starts[k]] for k in range(3)] == [0.25, 0.5, 0.25]


def test_plan_none_when_the_clip_fits_one_window():
    for F in (1, 2, 3):
        assert _windows(3, 1).plan(F) is None
    assert _windows(3, 1).plan(4) is not None
    from wan.utils.context_windows import ContextWindows
    assert ContextWindows().plan(21) is None and ContextWindows().plan(41).starts == [0, 17, 20]       # the defaults: 81 frames, overlap 16
    assert (ContextWindows().frames, ContextWindows().overlap, ContextWindows().fuse) == (81, 16, 'pyramid')


def test_plan_rejects():
    from wan.utils.context_windows import ContextWindows
    for bad in (dict(frames=80), dict(frames=10, overlap=4), dict(frames=0), dict(overlap=15), dict(overlap=2), dict(overlap=-4),
                dict(frames=9, overlap=12), dict(frames=9, overlap=16), dict(frames=1, overlap=4), dict(fuse='linear'), dict(fuse=None),
                dict(frames=9.0), dict(frames='9'), dict(overlap=4.0), dict(frames=True)):
        with pytest.raises(ValueError):
            ContextWindows(**bad)
    ContextWindows(frames=9, overlap=8)                 # O = 2 < Fw = 3
    ContextWindows(frames=1, overlap=0)                 # Fw = 1, O = 0
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            ContextWindows().plan(bad)


def test_declarations():
    """header and ctypes table agree on the two functions; generate, inpaint, WanT2V and ops have the new surface"""
    from wan.backend import lib, ops
    from wan.text2video import WanT2V
    decl = header_declarations()
    for name in NAMES:
        assert name in decl, f'include/moviigen_hip.h does not declare {name}'
        restype, want = decl[name]
        assert lib.SIGNATURES[name] == want, name
        assert restype is lib.c_int and name not in lib._RESTYPE
    par = list(inspect.signature(WanT2V.generate).parameters)
    assert par[par.index('guidance') + 1] == 'windows' and par[-2:] == ['init_video', 'strength']
    assert inspect.signature(WanT2V.generate).parameters['windows'].default is None
    par = list(inspect.signature(WanT2V.__init__).parameters)
    assert par[par.index('guidance') + 1] == 'windows' and par[-2:] == ['lora', 'lora_strength']
    assert inspect.signature(WanT2V.__init__).parameters['windows'].default is None
    inspect.signature(WanT2V.inpaint).bind(None, 'prompt', 'clip', windows=None)
    assert callable(ops.window_gather) and callable(ops.window_blend)


def _launcher(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', 'inference', 'generate.py'))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


def test_launcher_flags_reach_generate(tmp_path, monkeypatch):
    from wan.text2video import WanT2V
    from wan.utils.context_windows import ContextWindows
    g = _launcher('mg_generate_windows')
    assert {'--context_frames', '--context_overlap', '--context_fuse'} <= {f for f, _ in g.FLAGS}
    a = g._parse_args(['--ckpt_dir', '/x'])
    assert a.context_frames is None and a.context_overlap == 16 and a.context_fuse == 'pyramid' and a.windows is None
    a = g._parse_args(['--ckpt_dir', '/x', '--frame_num', '161', '--context_frames', '81', '--context_overlap', '16'])
    assert isinstance(a.windows, ContextWindows) and (a.windows.frames, a.windows.overlap, a.windows.fuse, a.frame_num) == (81, 16, 'pyramid', 161)
    assert g._parse_args(['--ckpt_dir', '/x', '--context_frames', '41', '--context_overlap', '8', '--context_fuse', 'flat']).windows.fuse == 'flat'
    for bad in (['--context_frames', '80'], ['--context_frames', '81', '--context_overlap', '15'], ['--context_frames', '9', '--context_overlap', '12'],
                ['--context_frames', '81', '--step_cache', '0.1']):
        with pytest.raises(AssertionError):
            g._parse_args(['--ckpt_dir', '/x'] + bad)
    calls = []

    class Pipe:
        last_step_plan = last_guidance_plan = None
        last_window_plan = [0, 2, 4]

        def __init__(self, **kw):
            pass

        def generate(self, prompt, **kw):
            calls.append(('generate', kw))
            return torch.zeros(3, 25, 8, 8)

        def inpaint(self, prompt, **kw):
            calls.append(('inpaint', kw))
            return torch.zeros(3, 25, 8, 8)
    monkeypatch.setattr(g.wan, 'WanT2V', Pipe)
    monkeypatch.setattr(g, 'cache_video', lambda **kw: kw['save_file'])
    np.save(tmp_path / 'clip.npy', np.zeros((25, 6, 7, 3), dtype=np.uint8))
    base = ['--ckpt_dir', '/x', '--frame_num', '25', '--save_file', str(tmp_path / 'out.mp4')]
    g.generate(g._parse_args(base))
    g.generate(g._parse_args(base + ['--context_frames', '9', '--context_overlap', '4']))
    g.generate(g._parse_args(base + ['--context_frames', '9', '--context_overlap', '4', '--init_video', str(tmp_path / 'clip.npy'), '--keep_frames', '5']))
    assert [c[0] for c in calls] == ['generate', 'generate', 'inpaint']
    assert 'windows' not in calls[0][1]                                         # without the flag the call is the one it was
    assert (calls[1][1]['windows'].Fw, calls[1][1]['windows'].O, calls[1][1]['frame_num']) == (3, 1, 25)
    assert calls[2][1]['windows'].Fw == 3 and calls[2][1]['keep_frames'] == 5
    inspect.signature(WanT2V.generate).bind(None, 'prompt', **calls[1][1])      # every keyword the launcher passes is one generate takes


# ------------------------------------------------------------------------------------------------
# GPU: the two passes.  F = 7; hw = 35: rows that are not 16-byte aligned and a scalar tail, 36: aligned for every f0, 1: degenerate
# ------------------------------------------------------------------------------------------------
F7 = 7
SHAPES = [(C, hw, Fw, 0) for C in (1, 3, 16) for hw in (35, 36, 1) for Fw in (3, 4)] + [(3, hw, Fw, 1) for hw in (35, 36) for Fw in (3, 4)]
SHAPE_IDS = [f'C{C}-hw{hw}-Fw{Fw}' + ('-base+4B' if off else '') for C, hw, Fw, off in SHAPES]
GUARD = 8                                               # elements in front of and behind a tensor inside its enclosing buffer


def _host(shape, seed):
    a = np.random.RandomState(seed).standard_normal(shape).astype(np.float32)
    a.setflags(write=False)
    return a


def _embed(a, off, dev, fill=-7.0):
    """a device copy of `a` inside a larger buffer, `off` elements (4 `off` bytes) behind a 16-byte boundary -> (view, buffer)"""
    buf = torch.full((GUARD + off + a.size + GUARD,), fill, device=dev)
    assert buf.data_ptr() % 16 == 0 and (GUARD * 4) % 16 == 0
    view = buf[GUARD + off:GUARD + off + a.size].view(a.shape)
    view.copy_(torch.tensor(a))
    assert view.data_ptr() % 16 == 4 * off
    return view, buf


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@gpu
@pytest.mark.parametrize('C,hw,Fw,off', SHAPES, ids=SHAPE_IDS)
def test_window_gather(dev, C, hw, Fw, off):
    from wan.backend import ops
    xn = _host((C, F7, hw), 100 + C + hw)
    x, xbuf = _embed(xn, off, dev)
    for f0 in range(F7 - Fw + 1):
        out, obuf = _embed(np.zeros((C, Fw, hw), dtype=np.float32), off, dev)
        out.fill_(float('nan'))
        before = _bits(obuf)
        assert ops.window_gather(x, f0, out) is out
        want = gather_ref(xn, f0, Fw)
        assert np.array_equal(_bits(out), want.view(np.uint32)), f0                     # the bits of the slice
        after = _bits(obuf)
        lo = GUARD + off
        assert np.array_equal(after[:lo], before[:lo]) and np.array_equal(after[lo + out.numel():], before[lo + out.numel():]), f0
        again, _ = _embed(np.zeros((C, Fw, hw), dtype=np.float32), off, dev)
        ops.window_gather(x, f0, again)
        assert np.array_equal(_bits(again), _bits(out)), f0                             # run twice: identical bytes
    assert np.array_equal(_bits(xbuf)[GUARD + off:GUARD + off + xn.size], xn.reshape(-1).view(np.uint32))    # x is only read


@gpu
@pytest.mark.parametrize('C,hw,Fw,off', SHAPES, ids=SHAPE_IDS)
def test_window_blend_one_call_every_f0(dev, C, hw, Fw, off):
    """one call at every valid f0 on an accumulator of finite values, `first` alternating over the window's frames: frames with `first`
    hold the fp32 product w v exactly, the others fma(w, v, a) within one rounding 2^-24 (w |v| + |a|) of fp64, every frame outside the window
    keeps its bits, and so does everything around acc"""
    from wan.backend import ops
    an, pn = _host((C, F7, hw), 200 + C + hw), _host((C, Fw, hw), 300 + C + hw)
    wn = np.linspace(0.25, 1.0, Fw).astype(np.float32)
    fn = (np.arange(Fw) % 2 == 0).astype(np.uint8)
    w, first = torch.from_numpy(wn).to(dev), torch.from_numpy(fn).to(dev)
    pred, _ = _embed(pn, off, dev)
    for f0 in range(F7 - Fw + 1):
        acc, abuf = _embed(an, off, dev)
        assert ops.window_blend(acc, pred, f0, w, first) is acc
        got = acc.cpu().numpy()
        value, mag = blend_once_ref(an, pn, f0, wn, fn)
        outside = np.ones(F7, dtype=bool)
        outside[f0:f0 + Fw] = False
        assert np.array_equal(got[:, outside].view(np.uint32), an[:, outside].view(np.uint32)), f0
        sel = fn.astype(bool)
        assert np.array_equal(got[:, f0:f0 + Fw][:, sel].view(np.uint32), (wn[None, :, None] * pn)[:, sel].view(np.uint32)), f0
        err = np.abs(got.astype(np.float64) - value)
        assert (err <= 2.0 ** -24 * mag).all(), (f0, float((err / mag).max()))
        bits = _bits(abuf)
        assert (bits[:GUARD + off] == bits[0]).all() and (bits[GUARD + off + an.size:] == bits[0]).all(), f0
    assert np.array_equal(_bits(pred), pn.view(np.uint32)) and np.array_equal(w.cpu().numpy(), wn) and np.array_equal(first.cpu().numpy(), fn)


@gpu
@pytest.mark.parametrize('fuse', FUSES)
@pytest.mark.parametrize('C,hw,Fw,off', SHAPES, ids=SHAPE_IDS)
def test_window_blend_plan_order(dev, C, hw, Fw, off, fuse):
    """the plan's windows in ascending order on an accumulator full of NaNs.  Fw = 3: starts 0, 2, 4; Fw = 4: starts 0, 2, 3, frame 3 in three windows"""
    from wan.backend import ops
    plan = _windows(Fw, Fw // 2, fuse).plan(F7)
    assert plan.starts == ([0, 2, 4] if Fw == 3 else [0, 2, 3])
    preds = [_host((C, Fw, hw), 400 + 10 * k + C + hw) for k in range(len(plan.starts))]
    w, first = plan.weights.to(dev), plan.first.to(dev)
    runs = []
    for rep in range(2):
        acc, abuf = _embed(np.zeros((C, F7, hw), dtype=np.float32), off, dev)
        acc.view(torch.int32).fill_(NAN_BITS)
        assert torch.isnan(acc).all().item()
        for k, f0 in enumerate(plan.starts):
            before = _bits(acc)
            pred, _ = _embed(preds[k], off, dev)
            ops.window_blend(acc, pred, f0, w[k], first[k])
            after = _bits(acc)
            outside = np.ones(F7, dtype=bool)
            outside[f0:f0 + Fw] = False
            assert np.array_equal(after[:, outside], before[:, outside]), (k, f0)       # untouched at the moment of this call
            seen = np.zeros(F7, dtype=bool)
            seen[:f0 + Fw] = True                                                       # (ascending starts: what has been covered so far)
            assert np.isfinite(after.view(np.float32)[:, seen]).all(), (k, f0)          # `first` is a select: the NaNs under it are gone
            assert (after[:, ~seen] == NAN_BITS).all(), (k, f0)
        runs.append((_bits(acc), _bits(abuf)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])      # run twice: identical bytes
    got = runs[0][0].view(np.float32)
    assert np.isfinite(got).all()
    value, mag, count = blend_ref(preds, plan.starts, plan.weights.numpy(), F7)
    assert (count >= 1).all() and (count.max() == 3) == (Fw == 4)
    for f in range(F7):
        if count[f] == 1:                                                               # covered once: weight 1.0f, the bits of pred
            k = plan.cover(f)[0]
            assert np.array_equal(got[:, f].view(np.uint32), preds[k][:, f - plan.starts[k]].view(np.uint32)), f
    err = np.abs(got.astype(np.float64) - value)                                        # every element, none left out
    bound = count[None, :, None] * 2.0 ** -24 * mag
    assert err.shape == (C, F7, hw) and (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())


@gpu
def test_window_ops_reject(dev):
    from wan.backend import lib, ops
    C, hw, Fw = 3, 36, 3
    x, out = torch.zeros(C, F7, hw, device=dev), torch.full((C, Fw, hw), -7.0, device=dev)
    acc, pred = torch.full((C, F7, hw), -7.0, device=dev), torch.zeros(C, Fw, hw, device=dev)
    w, first = torch.ones(Fw, device=dev), torch.ones(Fw, dtype=torch.uint8, device=dev)
    bad_gather = [(None, 0, out), (x, 0, None), (x.cpu(), 0, out), (x.double(), 0, out), (x, 0, out.half()), (x, -1, out), (x, F7 - Fw + 1, out),
                  (x, 0, torch.zeros(C, F7 + 1, hw, device=dev)), (x, 0, torch.zeros(C + 1, Fw, hw, device=dev)), (x, 0, torch.zeros(C, Fw, hw + 1, device=dev)),
                  (x[:, :, ::2], 0, out[:, :, ::2]), (x.transpose(0, 1), 0, out), (x, 0, torch.zeros(C, 0, hw, device=dev)), (x.view(-1), 0, out.view(-1))]
    for args in bad_gather:
        with pytest.raises(lib.MoviigenHipError):
            ops.window_gather(*args)
    bad_blend = [(None, pred, 0, w, first), (acc, None, 0, w, first), (acc, pred, 0, None, first), (acc, pred, 0, w, None), (acc, pred, 0, w.cpu(), first),
                 (acc, pred, 0, w.double(), first), (acc, pred, 0, w, first.float()), (acc, pred, 0, w[:2], first), (acc, pred, 0, w, first[:2]),
                 (acc, pred, 0, torch.ones(2 * Fw, device=dev)[::2], first), (acc, pred, -1, w, first), (acc, pred, F7 - Fw + 1, w, first),
                 (acc, pred.half(), 0, w, first), (acc, torch.zeros(C, Fw, hw + 1, device=dev), 0, w, first)]
    for args in bad_blend:
        with pytest.raises(lib.MoviigenHipError):
            ops.window_blend(*args)
    # the C ABI's own checks, behind the wrapper's: MG_ERR_SHAPE = -2 for a non-positive C, F, hw or Fw, f0 < 0 or f0 + Fw > F — checked
    # BEFORE the pointers (null pointers with a bad shape give -2) — and MG_ERR_ARG = -1 for a null pointer
    h, p = lib.load(), lambda t: lib.c_vp(t.data_ptr())
    good = dict(C=C, F=F7, hw=hw, f0=2, Fw=Fw)
    shapes = [dict(C=0), dict(C=-1), dict(F=0), dict(F=-7), dict(hw=0), dict(hw=-36), dict(Fw=0), dict(Fw=-3), dict(f0=-1), dict(f0=F7 - Fw + 1), dict(Fw=F7 + 1, f0=0),
              dict(F=2 ** 62, hw=2 ** 40)]
    for kw in shapes:
        a = dict(good, **kw)
        for px, po in ((p(x), p(out)), (None, None)):
            assert h.mg_window_gather_f32(px, a['C'], a['F'], a['hw'], a['f0'], a['Fw'], po, None) == -2, kw
        for pa, pp, pw, pf in ((p(acc), p(pred), p(w), p(first)), (None, None, None, None)):
            assert h.mg_window_blend_f32(pa, pp, a['C'], a['F'], a['hw'], a['f0'], a['Fw'], pw, pf, None) == -2, kw
    g = (good['C'], good['F'], good['hw'], good['f0'], good['Fw'])
    assert h.mg_window_gather_f32(None, *g, p(out), None) == -1 and h.mg_window_gather_f32(p(x), *g, None, None) == -1
    for nulled in range(4):
        ptrs = [p(acc), p(pred), p(w), p(first)]
        ptrs[nulled] = None
        assert h.mg_window_blend_f32(ptrs[0], ptrs[1], *g, ptrs[2], ptrs[3], None) == -1, nulled
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, -7.0)) and torch.equal(acc, torch.full_like(acc, -7.0))       # nothing was written


# ------------------------------------------------------------------------------------------------
# GPU: WanT2V.generate / inpaint(windows=) on the tiny pipeline of tests/test_guidance.py: latent [16, 7, 8, 8], three windows of 3 frames
# ------------------------------------------------------------------------------------------------
SIZE, FRAMES, LAT, STARTS = (64, 64), 25, (16, 7, 8, 8), [0, 2, 4]


def _vae_params(dim, seed=1):
    from vae_encode_ref import make_vae_encoder_params
    P = W.make_vae_params(dim, seed)
    P.update(make_vae_encoder_params(dim, seed + 100))
    return P


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
def prompts(dev):
    return W.randn((9, W.TINY_DIT['text_dim']), 31).to(dev), W.randn((5, W.TINY_DIT['text_dim']), 32).to(dev)


@pytest.fixture(scope='module')
def cw():
    from wan.utils.context_windows import ContextWindows
    return ContextWindows(frames=9, overlap=4)          # Fw = 3, O = 1


def _call(pipe, prompts, run=None, steps=2, **kw):
    lats = []
    kw.setdefault('callback', lambda i, l: lats.append((i, l.clone())))
    video = (run or pipe.generate)(prompts[0], size=SIZE, frame_num=FRAMES, shift=5.0, sample_solver='unipc', sampling_steps=steps, guide_scale=5.0,
                                   n_prompt=prompts[1], seed=0, offload_model=False, noise=W.randn(LAT, 33), **kw)
    return video, lats


def _record_calls(monkeypatch):
    """every library entry point called through wan.backend.lib.call, with its arguments, in order"""
    from wan.backend import lib
    log, real = [], lib.call
    monkeypatch.setattr(lib, 'call', lambda name, *args: (log.append((name, args)), real(name, *args))[1])
    return log


def _count_forwards(pipe, monkeypatch):
    """wrap the two methods `_sample` calls for a prediction -> the list of [method, DiT forwards it ran, latent frames it saw], one entry per call"""
    log, m = [], pipe.model
    inner = m._forward_one

    def one(*a, **kw):
        log[-1][1] += 1
        return inner(*a, **kw)
    monkeypatch.setattr(m, '_forward_one', one)
    for name in ('_guidance_pair', '_cond_prediction'):
        def wrapped(latent, *a, _f=getattr(pipe, name), _n=name, **kw):
            log.append([_n, 0, latent.shape[1]])
            return _f(latent, *a, **kw)
        monkeypatch.setattr(pipe, name, wrapped)
    return log


@gpu
def test_one_step_prediction_is_the_blend_of_the_window_predictions(dev, pipe, prompts, cw):
    """the whole-clip cond / uncond the product forms against this test's own composition: _guidance_pair on torch slices of the same latent
    (the same bits in, hence the same bits out of the DiT) blended in fp64; the kernel test's bound per element"""
    from wan.text2video import WindowRun
    plan = cw.plan(LAT[1])
    assert plan.starts == STARTS
    latent, t = W.randn(LAT, 33).to(dev), torch.tensor([999], device=dev)
    ctx, ctx_null = [prompts[0]], [prompts[1]]
    run = WindowRun(plan, latent, True, pipe.patch_size, pipe.sp_size)
    assert run.seq_len == 3 * 4 * 4 and tuple(run.lat.shape) == (16, 3, 8, 8)
    run.cond.view(torch.int32).fill_(NAN_BITS)
    run.uncond.view(torch.int32).fill_(NAN_BITS)
    with torch.no_grad():
        cond, uncond = pipe._window_predictions(run, latent, t, ctx, ctx_null)
        assert cond is run.cond and uncond is run.uncond and torch.equal(latent, W.randn(LAT, 33).to(dev))
        cond = cond.clone()                                                             # (the buffers are reused by the next call)
        pairs = [pipe._guidance_pair(latent[:, f0:f0 + 3].contiguous(), t, ctx, ctx_null, 48) for f0 in STARTS]
        only, none = pipe._window_predictions(run, latent, t, ctx, None)                # a 'cond' step: the conditional branch alone
    assert none is None and only is run.cond
    for got, preds in ((cond, [p[0] for p in pairs]), (uncond, [p[1] for p in pairs])):
        preds = [p.cpu().numpy().reshape(16, 3, 64) for p in preds]
        value, mag, count = blend_ref(preds, STARTS, plan.weights.numpy(), 7)
        g = got.cpu().numpy().reshape(16, 7, 64)
        assert np.isfinite(g).all() and count.tolist() == [1, 1, 2, 1, 2, 1, 1]
        err = np.abs(g.astype(np.float64) - value)
        assert (err <= count[None, :, None] * 2.0 ** -24 * mag).all()
        assert np.array_equal(g[:, 0], preds[0][:, 0]) and np.array_equal(g[:, 6], preds[2][:, 2])
    # model(...) alone gives the cond half of forward_pair bit for bit: the 'cond' step's buffer is the guided step's cond buffer
    assert torch.equal(only, cond)


@gpu
def test_one_window_is_the_loop_without_windows(dev, pipe, prompts, monkeypatch):
    from wan.utils.context_windows import ContextWindows
    _call(pipe, prompts)                                # what a pipeline launches once per shape or prompt (folded VAE weights, prompt caches) is behind us
    log = _record_calls(monkeypatch)
    video, lats = _call(pipe, prompts)
    plain = [name for name, _ in log]
    assert pipe.last_window_plan is None
    del log[:]
    v, l = _call(pipe, prompts, windows=ContextWindows(frames=25))
    assert pipe.last_window_plan is None
    assert [name for name, _ in log] == plain and not any(name in NAMES for name in plain)          # the same library calls
    assert torch.equal(v, video) and len(l) == len(lats) == 2 and all(torch.equal(a[1], b[1]) for a, b in zip(l, lats))
    del log[:]
    pipe.windows = ContextWindows(frames=81)            # the object's default is what generate(windows=None) uses
    try:
        assert torch.equal(_call(pipe, prompts)[0], video) and [name for name, _ in log] == plain
    finally:
        pipe.windows = None


@gpu
def test_two_steps_with_windows(dev, pipe, prompts, cw, monkeypatch):
    log = _record_calls(monkeypatch)
    video, lats = _call(pipe, prompts, windows=cw)
    assert tuple(video.shape) == (3, FRAMES, SIZE[1], SIZE[0]) and torch.isfinite(video).all().item()
    assert pipe.last_window_plan == STARTS
    assert [i for i, _ in lats] == [0, 1] and all(tuple(l.shape) == LAT and torch.isfinite(l).all().item() for _, l in lats)
    names = [name for name, _ in log]
    # per step: three gathers, three blends per branch, ONE mix on the whole clip
    assert names.count('mg_window_gather_f32') == 6 and names.count('mg_window_blend_f32') == 12 and names.count('mg_cfg_combine_f32') == 2
    assert [a[4] for n, a in log if n == 'mg_window_gather_f32'] == STARTS * 2                       # ascending, every step
    assert all(a[4] == 16 * 7 * 8 * 8 for n, a in log if n == 'mg_cfg_combine_f32')                  # n: the whole clip
    assert all(a[2] == 3 for n, a in log if n == 'mg_patchify_bf16')                                 # every DiT pass sees Fw = 3 frames
    v2, l2 = _call(pipe, prompts, windows=cw)
    assert torch.equal(v2, video) and all(torch.equal(a[1], b[1]) for a, b in zip(l2, lats))         # the same seed: the same bits
    plain, _ = _call(pipe, prompts)
    assert pipe.last_window_plan is None and not torch.equal(plain, video)                           # windows are another computation
    pipe.windows = cw
    try:
        assert torch.equal(_call(pipe, prompts)[0], video) and pipe.last_window_plan == STARTS
    finally:
        pipe.windows = None


@gpu
def test_step_kinds_with_windows(dev, pipe, prompts, cw, monkeypatch):
    """3 steps at shift 5: sigma = 1 (0.9998), 0.909, 0.714 -> 'zero' (zero-init), 'guided' (inside the band), 'cond' (below it)"""
    from wan.utils.guidance import Guidance
    fwd = _count_forwards(pipe, monkeypatch)
    calls = _record_calls(monkeypatch)
    seen = []
    _call(pipe, prompts, steps=3, windows=cw, guidance=Guidance(interval=(0.8, 0.95), zero_init_steps=1), callback=lambda i, l: seen.append((i, len(fwd), len(calls))))
    assert pipe.last_guidance_plan == ['zero', 'guided', 'cond'] and pipe.last_window_plan == STARTS
    assert [n for _, n, _ in seen] == [0, 3, 6]                                                     # no forward in the 'zero' step
    assert fwd == [['_guidance_pair', 2, 3]] * 3 + [['_cond_prediction', 1, 3]] * 3                # one forward per window and branch
    names = [n for n, _ in calls]
    assert not any(n in NAMES for n in names[:seen[0][2]])                                          # ... and no window pass either
    step = lambda k: names[seen[k - 1][2]:seen[k][2]]      # noqa: E731
    assert step(1).count('mg_window_gather_f32') == 3 and step(1).count('mg_window_blend_f32') == 6 and step(1).count('mg_cfg_combine_f32') == 1
    assert step(2).count('mg_window_gather_f32') == 3 and step(2).count('mg_window_blend_f32') == 3 and step(2).count('mg_cfg_combine_f32') == 0


@gpu
def test_cfg_zero_star_statistics_are_over_the_whole_clip(dev, pipe, prompts, cw, monkeypatch):
    from wan.utils.guidance import Guidance
    calls = _record_calls(monkeypatch)
    video, _ = _call(pipe, prompts, windows=cw, guidance=Guidance(zero_star=True, rescale=0.5))
    n = 16 * 7 * 8 * 8
    assert [a[2] for name, a in calls if name == 'mg_cfg_stats_f32'] == [n, n]                      # once per step
    assert [a[1] for name, a in calls if name == 'mg_cfg_coef_f32'] == [n, n]
    assert [a[3] for name, a in calls if name == 'mg_cfg_combine_coef_f32'] == [n, n] and torch.isfinite(video).all().item()


@gpu
def test_windows_with_a_step_cache_raise_before_any_forward(dev, pipe, prompts, cw, monkeypatch):
    import wan

    def no_forward(*a, **kw):
        raise AssertionError('a DiT forward ran: the argument check came too late')
    monkeypatch.setattr(pipe.model, '_forward_one', no_forward)
    with pytest.raises(ValueError, match='step_cache'):
        _call(pipe, prompts, windows=cw, step_cache=0.1)
    pipe.step_cache = 0.1                               # the object's default counts too
    try:
        with pytest.raises(ValueError, match='step_cache'):
            _call(pipe, prompts, windows=cw)
    finally:
        pipe.step_cache = None
    for bad in (9, (9, 4), 'pyramid', dict(frames=9)):
        with pytest.raises(ValueError, match='windows'):
            _call(pipe, prompts, windows=bad)
    with pytest.raises(ValueError, match='windows'):
        wan.WanT2V(pipe.config, '', device_id=0, model=pipe.model, vae=pipe.vae, windows=9)
    from wan.utils.context_windows import ContextWindows
    with pytest.raises(ValueError, match='stride'):
        _call(pipe, prompts, windows=ContextWindows(frames=9, overlap=4, stride=2))


@gpu
def test_inpaint_with_windows_keeps_the_source_pixels(dev, pipe, prompts, cw):
    from wan.backend import ops
    frames = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (FRAMES + 2, 50, 70, 3)).astype(np.uint8))
    clip = ops.video_from_u8(frames[:FRAMES].to(dev), SIZE[1], SIZE[0])
    video, lats = _call(pipe, prompts, run=lambda p, **kw: pipe.inpaint(p, frames, keep_frames=5, windows=cw, **kw))
    assert pipe.last_window_plan == STARTS and tuple(video.shape) == (3, FRAMES, SIZE[1], SIZE[0]) and torch.isfinite(video).all().item()
    assert torch.equal(video[:, :5], clip[:, :5]) and not torch.equal(video[:, 5:], clip[:, 5:])    # kept pixels: the source's, bit for bit
    z0 = pipe.vae.encode([clip])[0]
    assert torch.equal(lats[-1][1][:, :2], z0[:, :2])   # latent frames 0 and 1 lie under the kept pixel frames 0 .. 4: sigma ends in 0, they end as z0
