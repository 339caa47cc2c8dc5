"""Guidance options of WanT2V.generate (guidance=Guidance(...)): the host rule wan/utils/guidance.py, the three device passes
mg_cfg_stats_f32, mg_cfg_coef_f32, mg_cfg_combine_coef_f32 and the sampling loop.

CPU: Guidance's validation and plan against hand-written expectations, the launcher flags, the declarations, the cfg-parallel branch rule.
GPU: cfg_stats against sums wider than fp64 (tests/guidance_ref.py) within k 2^-53 sum |terms|, k the longest chain of additions an element
passes through in the kernel's order; cfg_coefficients against the fp64 restatement within 2^-22 relative (two fp64 evaluations that differ
in their last bits round to the same fp32 value or, at a tie, to neighbours: 1 ulp = 2^-23, doubled); cfg_combine_coef bit for bit against
ops.lincomb; the three together against fp64 end to end; WanT2V.generate / inpaint on the tiny pipeline of tests/test_inpaint.py bit for bit
against loops written here from the model, the ops and the scheduler.
"""
import functools
import importlib.util
import inspect
import math
import os

import numpy as np
import pytest
import torch

import weights as W
from abi_ref import header_declarations
from guidance_ref import coef_ref, combine_ref, stats_ref, variances

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('mg_cfg_stats_partials_bytes', 'mg_cfg_stats_f32', 'mg_cfg_coef_f32', 'mg_cfg_combine_coef_f32')
# csrc/dit_elementwise.hip: cfg_stats_kernel runs CS_GRID workgroups (read back from mg_cfg_stats_partials_bytes) of NT lanes, a lane takes
# CS_UNROLL 16-byte groups one grid stride apart per sweep; cfg_combine_coef_kernel runs at most CC_GRID workgroups of NT lanes, one group per lane
NT, CS_UNROLL, CC_GRID, CS_SUMS = 256, 4, 2048, 5


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _launcher(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', 'inference', 'generate.py'))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


def _scheduler(solver, n, shift, device='cpu'):
    """the scheduler and its timesteps as WanT2V.generate sets them up"""
    from wan.utils import FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, get_sampling_sigmas, retrieve_timesteps
    if solver == 'unipc':
        s = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
        s.set_timesteps(n, device=device, shift=shift)
        return s, s.timesteps
    s = FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    ts, _ = retrieve_timesteps(s, device=device, sigmas=get_sampling_sigmas(n, shift))
    return s, ts


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
def test_declarations():
    """header and ctypes table agree on the four functions; generate, inpaint, WanT2V and the launcher have the new surface"""
    from wan.backend import lib
    from wan.text2video import WanT2V
    decl = header_declarations()
    for name in NAMES:
        assert name in decl, f'include/moviigen_hip.h does not declare {name}'
        restype, want = decl[name]
        assert restype in (lib.c_int, lib.c_i64) and lib.SIGNATURES[name] == want, name
        assert (restype is lib.c_i64) == (lib._RESTYPE.get(name) is lib.ctypes.c_int64), name
    assert inspect.signature(WanT2V.generate).parameters['guidance'].default is None
    assert inspect.signature(WanT2V.__init__).parameters['guidance'].default is None
    inspect.signature(WanT2V.inpaint).bind(None, 'prompt', 'clip', guidance=None)
    from wan.backend import ops
    for fn in ('cfg_stats_partials', 'cfg_stats', 'cfg_coefficients', 'cfg_combine_coef'):
        assert callable(getattr(ops, fn))


def test_guidance_validation():
    from wan.utils.guidance import Guidance
    g = Guidance()
    assert (g.scale, g.interval, g.zero_star, g.zero_init_steps, g.rescale) == (None, (0.0, 1.0), False, 0, 0.0) and g.plain_mix
    g = Guidance(scale=3, interval=[0.25, 0.75], zero_star=True, zero_init_steps=np.int64(2), rescale=1)
    assert (g.scale, g.interval, g.zero_star, g.zero_init_steps, g.rescale) == (3.0, (0.25, 0.75), True, 2, 1.0) and not g.plain_mix
    assert not Guidance(rescale=0.5).plain_mix and not Guidance(zero_star=True).plain_mix and Guidance(interval=(0.5, 0.5)).plain_mix
    for bad in (dict(interval=(-0.1, 1.0)), dict(interval=(0.0, 1.1)), dict(interval=(0.7, 0.3)), dict(interval=(0.5,)), dict(interval=0.5),
                dict(interval=(float('nan'), 1.0)), dict(interval=('a', 'b')), dict(rescale=-0.01), dict(rescale=1.01), dict(rescale=float('nan')),
                dict(zero_init_steps=-1), dict(zero_init_steps=1.5), dict(zero_init_steps=2.0), dict(zero_init_steps='2'), dict(zero_init_steps=True),
                dict(scale=float('inf'))):
        with pytest.raises(ValueError):
            Guidance(**bad)


@pytest.mark.parametrize('solver', ['unipc', 'dpm++'])
def test_guidance_plan(solver):
    """both solvers at (steps 6, shift 5.0): sigma = 1 (0.9998 for unipc), 0.961, 0.909, 0.833, 0.714, 0.5 (0.4997)"""
    from wan.utils.guidance import Guidance
    sched, ts = _scheduler(solver, 6, 5.0)
    sig = sched.sigmas.tolist()[:len(ts)]
    want = [1.0 if solver == 'dpm++' else 0.9998, 0.9615, 0.9091, 0.8333, 0.7143, 0.5 if solver == 'dpm++' else 0.4997]
    assert len(sig) == 6 and all(abs(a - b) < 4e-4 for a, b in zip(sig, want))
    z, c, G = 'zero', 'cond', 'guided'
    assert Guidance().plan(sig) == [G] * 6
    assert Guidance(scale=3.0, zero_star=True, rescale=0.5).plan(sig) == [G] * 6
    assert Guidance(interval=(0.6, 0.95)).plan(sig) == [c, c, G, G, G, c]                     # 'cond' steps on both sides
    assert Guidance(interval=(0.0, 0.95)).plan(sig) == [c, c, G, G, G, G]
    assert Guidance(interval=(0.6, 1.0)).plan(sig) == [G, G, G, G, G, c]
    assert Guidance(interval=(0.0, 0.0)).plan(sig) == [c] * 6
    assert Guidance(interval=(sig[3], sig[3])).plan(sig) == [c, c, c, G, c, c]                # both ends belong to the band
    assert Guidance(zero_init_steps=2).plan(sig) == [z, z, G, G, G, G]
    assert Guidance(interval=(0.6, 0.95), zero_init_steps=1).plan(sig) == [z, c, G, G, G, c]
    assert Guidance(interval=(0.6, 0.95), zero_init_steps=3).plan(sig) == [z, z, z, G, G, c]
    assert Guidance(zero_init_steps=9).plan(sig) == [z] * 6
    # i0 > 0 (video-to-video): the plan is per SCHEDULE index, the loop reads it from i0 on
    assert Guidance(interval=(0.6, 0.95), zero_init_steps=2).plan(sig, 3) == [z, z, G, G, G, c]
    assert Guidance(interval=(0.6, 0.95), zero_init_steps=2).plan(sig, 3)[3:] == [G, G, c]
    with pytest.raises(ValueError):
        Guidance().plan(sig, 6)


def test_step_plan_adjusted_to_guidance():
    from wan.utils.guidance import adjust_step_plan
    z, c, G, C, S = 'zero', 'cond', 'guided', True, False
    kinds = [c, c, G, G, G, c]
    assert adjust_step_plan([C, S, S, C, S, S], kinds) == [C, S, C, C, S, S]                # the first 'guided' step behind 'cond' steps is computed
    assert adjust_step_plan([S, S, S, S, S, S], kinds) == [C, S, C, S, S, S]                # ... and the first step that runs a forward
    assert adjust_step_plan([S, S, S, S, S, S], kinds, own_branch_only=True) == [C, S, C, S, S, C]
    assert adjust_step_plan([S, S, S, S, S, S], [z, z, G, G, c, G]) == [S, S, C, S, S, C]    # 'zero' steps run no forward
    assert adjust_step_plan([S, S, S, S, S, S], kinds, 3) == [S, S, S, C, S, S]
    assert adjust_step_plan([C, S, C, S, C, C], [G] * 6) == [C, S, C, S, C, C]


def test_launcher_flags_reach_generate(tmp_path, monkeypatch):
    """the four flags parse, are declared in the launcher's table, and reach WanT2V.generate / inpaint as one Guidance; without them the call
    carries no `guidance` (a recording pipeline)"""
    from wan.utils.guidance import Guidance
    g = _launcher('mg_generate_guidance')
    assert {'--guide_interval', '--cfg_zero_star', '--cfg_zero_init', '--guide_rescale'} <= {f for f, _ in g.FLAGS}
    a = g._parse_args(['--ckpt_dir', '/x'])
    assert a.guide_interval is None and a.cfg_zero_star is False and a.cfg_zero_init == 0 and a.guide_rescale == 0.0 and a.guidance is None
    a = g._parse_args(['--ckpt_dir', '/x', '--guide_interval', '0.25,0.9', '--cfg_zero_star', '--cfg_zero_init', '2', '--guide_rescale', '0.7'])
    assert isinstance(a.guidance, Guidance)
    assert (a.guidance.scale, a.guidance.interval, a.guidance.zero_star, a.guidance.zero_init_steps, a.guidance.rescale) == (None, (0.25, 0.9), True, 2, 0.7)
    assert g._parse_args(['--ckpt_dir', '/x', '--guide_rescale', '0.5']).guidance.interval == (0.0, 1.0)
    for bad in (['--guide_interval', '0.9,0.25'], ['--guide_interval', '0.5'], ['--guide_interval', 'a,b'], ['--guide_interval', '0,1.5'],
                ['--guide_rescale', '1.5'], ['--guide_rescale', '-0.5'], ['--cfg_zero_init', '-1']):
        with pytest.raises(AssertionError):
            g._parse_args(['--ckpt_dir', '/x'] + bad)
    calls = []

    class Pipe:
        last_step_plan = None
        last_guidance_plan = ['cond', 'guided']

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
    np.save(tmp_path / 'clip.npy', np.zeros((5, 6, 7, 3), dtype=np.uint8))
    base = ['--ckpt_dir', '/x', '--frame_num', '5', '--save_file', str(tmp_path / 'out.mp4')]
    g.generate(g._parse_args(base))
    g.generate(g._parse_args(base + ['--guide_interval', '0.3,0.95', '--sample_guide_scale', '4']))
    g.generate(g._parse_args(base + ['--cfg_zero_star', '--init_video', str(tmp_path / 'clip.npy'), '--keep_frames', '1']))
    assert [c[0] for c in calls] == ['generate', 'generate', 'inpaint']
    assert 'guidance' not in calls[0][1]
    assert calls[1][1]['guidance'].interval == (0.3, 0.95) and calls[1][1]['guidance'].scale is None and calls[1][1]['guide_scale'] == 4.0
    assert calls[2][1]['guidance'].zero_star and calls[2][1]['keep_frames'] == 1
    WanT2V = __import__('wan.text2video', fromlist=['WanT2V']).WanT2V
    inspect.signature(WanT2V.generate).bind(None, 'prompt', **calls[1][1])          # every keyword the launcher passes is one generate takes


def test_cfg_parallel_branch_rule():
    """on a 'cond' step both halves of a cfg-parallel layout run the CONDITIONAL branch and exchange nothing (a stub model and a stub cfgp);
    a 'guided' step, for contrast, runs each half's own branch and swaps"""
    from wan.text2video import WanT2V
    ctx, ctx_null, latent, t = [torch.ones(2, 4)], [torch.zeros(2, 4)], torch.zeros(16, 1, 2, 2), torch.tensor([999])

    class Cfgp:
        def __init__(self, branch):
            self.branch, self.exchanged = branch, 0

        def exchange(self, mine):
            self.exchanged += 1
            return mine, mine
    for branch in (0, 1):
        seen = []

        def model(x, t, context, seq_len):
            seen.append(context)
            return [x[0] + 1.0]
        pipe = WanT2V.__new__(WanT2V)
        pipe.model, pipe.cfgp = model, Cfgp(branch)
        out = pipe._cond_prediction(latent, t, ctx, 4)
        assert len(seen) == 1 and seen[0] is ctx and pipe.cfgp.exchanged == 0 and torch.equal(out, latent + 1.0)
        pipe._guidance_pair(latent, t, ctx, ctx_null, 4)
        assert len(seen) == 2 and seen[1] is (ctx_null if branch else ctx) and pipe.cfgp.exchanged == 1


# ------------------------------------------------------------------------------------------------
# GPU: the three passes
# ------------------------------------------------------------------------------------------------
def _grid():
    from wan.backend import lib
    nbytes = int(lib.load().mg_cfg_stats_partials_bytes())
    assert nbytes % (CS_SUMS * 8) == 0
    return nbytes // (CS_SUMS * 8)


def _sizes():
    """the sizes at which cfg_stats_kernel takes another path, from its constants"""
    lanes = _grid() * NT
    sweep = lanes * CS_UNROLL * 4
    return {'tail only': 3, 'one element': 1, 'fewer groups than lanes': 2048, 'n % 4 != 0': 4 * 1000 + 3,
            'one grid stride, unroll partly used': lanes * 4 + 5, 'exactly one sweep': sweep, 'one sweep and a partial second': sweep + lanes * 2 + 4 * 77 + 1}


SIZE_NAMES = ['tail only', 'one element', 'fewer groups than lanes', 'n % 4 != 0', 'one grid stride, unroll partly used', 'exactly one sweep',
              'one sweep and a partial second']


def _chain(n):
    """k: the longest chain of additions an element passes through in cfg_stats' order — its lane's (4 per 16-byte group, the groups of a
    lane one after the other, + the scalar tail's one), the wave's tree (6), the workgroup's waves (NT / 64) and the partials in index order"""
    grid = _grid()
    nvec = n // 4
    return 4 * math.ceil(nvec / (grid * NT)) + (1 if n % 4 else 0) + 6 + NT // 64 + grid


@functools.lru_cache(maxsize=None)
def _pair(n):
    """(u, c) fp32 arrays, u ~ N(0.5, 1), c = u + 0.3 N(0, 1): correlated and with a mean, so the variance terms cancel.  Computed once, never written"""
    rs = np.random.RandomState(n % 9973)
    u = (0.5 + rs.standard_normal(n)).astype(np.float32)
    c = (u + 0.3 * rs.standard_normal(n)).astype(np.float32)
    u.setflags(write=False)
    c.setflags(write=False)
    return u, c


@functools.lru_cache(maxsize=None)
def _pair_sums(n):
    return stats_ref(*_pair(n))


def _scratch(dev):
    from wan.backend import ops
    return torch.full((5,), -7.0, dtype=torch.float64, device=dev), ops.cfg_stats_partials(dev), torch.full((2,), -7.0, device=dev)


@gpu
def test_cfg_stats_constants(dev):
    assert sorted(_sizes()) == sorted(SIZE_NAMES)
    sizes = _sizes()
    assert _grid() >= 1 and max(sizes.values()) < 8 << 20 and sizes['exactly one sweep'] > CC_GRID * NT * 4      # (the combine's element loop wraps there)


@gpu
@pytest.mark.parametrize('name', SIZE_NAMES)
def test_cfg_stats(dev, name):
    from wan.backend import ops
    n = _sizes()[name]
    un, cn = _pair(n)
    u, c = torch.from_numpy(un).to(dev), torch.from_numpy(cn).to(dev)
    stats, partials, _ = _scratch(dev)
    assert ops.cfg_stats(u, c, stats, partials) is stats
    got = stats.cpu().numpy()
    again = torch.empty(5, dtype=torch.float64, device=dev)
    ops.cfg_stats(u.clone(), c.clone(), again, torch.full_like(partials, float('nan')))     # other buffers, scratch with no usable initial value
    assert got.tobytes() == again.cpu().numpy().tobytes()                                    # the same 40 bytes
    assert np.array_equal(u.cpu().numpy(), un) and np.array_equal(c.cpu().numpy(), cn)       # the inputs are only read
    exact, scale = _pair_sums(n)
    k = _chain(n)
    for q, label in enumerate(('sum u', 'sum c', 'sum u^2', 'sum c^2', 'sum u c')):
        err = abs(float(np.longdouble(got[q]) - exact[q]))
        print(f'n {n} ({name}) {label}: {got[q]!r} err {err:.3e} bound {k} * 2^-53 * {scale[q]:.6e} = {k * 2.0 ** -53 * scale[q]:.3e}')
        assert err <= k * 2.0 ** -53 * scale[q], label


@gpu
def test_cfg_stats_rejects(dev):
    from wan.backend import lib, ops
    n = 4096
    u, c = torch.from_numpy(_pair(n)[0]).to(dev), torch.from_numpy(_pair(n)[1]).to(dev)
    stats, partials, _ = _scratch(dev)
    wide = torch.zeros(2, n + 4, device=dev)
    bad = [(None, c, stats, partials), (u, None, stats, partials), (u, c, None, partials), (u, c, stats, None),
           (u.cpu(), c, stats, partials), (u, c, stats.cpu(), partials),
           (u.double(), c, stats, partials), (u, c.half(), stats, partials), (u, c, stats.float(), partials), (u, c, stats, partials.float()),
           (u[::2], c[::2], stats, partials), (wide[:, :n], wide[:, :n], stats, partials),          # sliced views
           (wide[0, 1:n + 1], c, stats, partials), (u, wide[0, 3:n + 3], stats, partials),            # dense, but 4 and 12 bytes off a 16-byte boundary
           (u, c[:-4], stats, partials), (u[:0], c[:0], stats, partials),                            # size mismatch, no element
           (u, c, stats[:4], partials), (u, c, torch.empty(6, dtype=torch.float64, device=dev), partials), (u, c, stats, partials[:-1])]
    for args in bad:
        with pytest.raises(lib.MoviigenHipError):
            ops.cfg_stats(*args)
    torch.cuda.synchronize()
    assert torch.equal(stats, torch.full_like(stats, -7.0))                                         # nothing was written
    # the C ABI's own checks, behind the wrapper's: MG_ERR_ARG = -1 on a null pointer, MG_ERR_SHAPE = -2 on n < 1 and on misaligned pointers
    h, p = lib.load(), lambda t, off=0: lib.c_vp(t.data_ptr() + off)
    assert h.mg_cfg_stats_f32(None, p(c), n, p(stats), p(partials), None) == -1 and h.mg_cfg_stats_f32(p(u), p(c), n, None, p(partials), None) == -1
    assert h.mg_cfg_stats_f32(p(u), p(c), n, p(stats), None, None) == -1
    assert h.mg_cfg_stats_f32(p(u), p(c), 0, p(stats), p(partials), None) == -2
    assert h.mg_cfg_stats_f32(p(u, 4), p(c), n - 4, p(stats), p(partials), None) == -2 and h.mg_cfg_stats_f32(p(u), p(c, 8), n - 4, p(stats), p(partials), None) == -2
    assert h.mg_cfg_stats_f32(p(u), p(c), n, p(stats, 4), p(partials), None) == -2 and h.mg_cfg_stats_f32(p(u), p(c), n, p(stats), p(partials, 4), None) == -2
    torch.cuda.synchronize()
    assert torch.equal(stats, torch.full_like(stats, -7.0))


# stats (S_u, S_c, S_uu, S_cc, S_uc) over N = 1000 elements that need not come from data: var_u = 1, var_c = 1.1296, S_uc^2 < S_uu S_cc
N_COEF, STATS_COEF = 1000, (500.0, 520.0, 1250.0, 1400.0, 1300.0)
COEF_CASES = [      # (name, stats, g, zero_star, rescale, exact)
    ('plain', STATS_COEF, 5.0, False, 0.0, (-4.0, 5.0)),
    ('plain, g not an integer', STATS_COEF, 7.3, False, 0.0, (float(np.float32(1.0 - float(np.float32(7.3)))), float(np.float32(7.3)))),
    ('zero_star', STATS_COEF, 5.0, True, 0.0, None),
    ('rescale 0.7', STATS_COEF, 5.0, False, 0.7, None),
    ('zero_star and rescale 0.7', STATS_COEF, 5.0, True, 0.7, None),
    ('rescale 1', STATS_COEF, 3.5, True, 1.0, None),
    ('S_uu = 0', (0.0, 520.0, 0.0, 1400.0, 0.0), 5.0, True, 0.0, (0.0, 5.0)),
    ('constant tensors u = 1, c = 2: var_p = 0, f = 1', (1000.0, 2000.0, 1000.0, 4000.0, 2000.0), 5.0, False, 0.7, (-4.0, 5.0)),
    ('constant tensors u = c = 1, g = 1: var_p = var_c = 0, f = 1', (1000.0, 1000.0, 1000.0, 1000.0, 1000.0), 1.0, False, 0.7, (0.0, 1.0)),
]


def test_coefficient_cases_are_well_conditioned():
    """CPU, the reference alone: the cases that take the rescale branch have var_p and var_c well away from 0; the fallback cases have var_p <= 0"""
    for name, stats, g, zs, phi, exact in COEF_CASES:
        if phi > 0.0:
            s = stats[4] / (stats[2] + 1e-8) if zs else 1.0
            varp, varc = variances(stats, N_COEF, s * (1.0 - g), g)
            if exact is None:
                assert varp > 0.1 and varc > 0.1, (name, varp, varc)
            else:
                assert varp <= 0.0, (name, varp)
        if exact is not None:
            assert tuple(float(np.float32(v)) for v in coef_ref(stats, N_COEF, g, zs, phi)) == exact, name


@gpu
@pytest.mark.parametrize('case', COEF_CASES, ids=[c[0] for c in COEF_CASES])
def test_cfg_coefficients(dev, case):
    from wan.backend import ops
    name, stats, g, zs, phi, exact = case
    coef = torch.full((2,), -7.0, device=dev)
    assert ops.cfg_coefficients(torch.tensor(stats, dtype=torch.float64, device=dev), N_COEF, g, zs, phi, coef) is coef
    got = [float(v) for v in coef.tolist()]
    want = coef_ref(stats, N_COEF, g, zs, phi)
    print(f'{name}: got {got} fp64 reference {want}')
    if exact is not None:
        assert tuple(got) == exact                      # (-0.0 == 0.0: the S_uu = 0 case gives 0 (1 - g))
    for a, b in zip(got, want):
        assert abs(a - b) <= 2.0 ** -22 * abs(b)


@gpu
def test_cfg_coefficients_rejects(dev):
    from wan.backend import lib, ops
    stats = torch.tensor(STATS_COEF, dtype=torch.float64, device=dev)
    coef = torch.full((2,), -7.0, device=dev)
    for kw in (dict(rescale=-0.1), dict(rescale=1.5), dict(rescale=float('nan')), dict(g=float('inf')), dict(g=float('-inf')), dict(g=float('nan')),
               dict(n=0), dict(stats=stats[:4]), dict(stats=stats.float()), dict(stats=stats.cpu()), dict(stats=None), dict(coef=None),
               dict(coef=torch.zeros(3, device=dev)), dict(coef=coef.double()), dict(coef=torch.zeros(4, device=dev)[::2])):
        args = dict(dict(stats=stats, n=N_COEF, g=5.0, zero_star=True, rescale=0.5, coef=coef), **kw)
        with pytest.raises(lib.MoviigenHipError):
            ops.cfg_coefficients(**args)
    h, p = lib.load(), lambda t: lib.c_vp(t.data_ptr())
    assert h.mg_cfg_coef_f32(p(stats), N_COEF, float('inf'), 0, 0.0, p(coef), None) == -1 and h.mg_cfg_coef_f32(p(stats), N_COEF, 5.0, 0, 1.5, p(coef), None) == -1
    assert h.mg_cfg_coef_f32(p(stats), N_COEF, 5.0, 0, float('nan'), p(coef), None) == -1 and h.mg_cfg_coef_f32(None, N_COEF, 5.0, 0, 0.0, p(coef), None) == -1
    torch.cuda.synchronize()
    assert torch.equal(coef, torch.full_like(coef, -7.0))


@gpu
@pytest.mark.parametrize('name', SIZE_NAMES)
def test_cfg_combine_coef_is_lincomb(dev, name):
    from wan.backend import ops
    n = _sizes()[name]
    u, c = torch.from_numpy(_pair(n)[0]).to(dev), torch.from_numpy(_pair(n)[1]).to(dev)
    coef = torch.tensor([-4.1632, 5.0371], device=dev)
    au, ac = coef.tolist()
    want = ops.lincomb(torch.empty_like(u), [(u, au), (c, ac)])
    out = torch.full_like(u, float('nan'))
    assert ops.cfg_combine_coef(out, u, c, coef) is out
    assert torch.equal(out, want)
    ua, ca = u.clone(), c.clone()
    ops.cfg_combine_coef(ua, ua, c, coef)               # out aliases u
    ops.cfg_combine_coef(ca, u, ca, coef)               # out aliases c
    assert torch.equal(ua, want) and torch.equal(ca, want)
    assert torch.equal(coef, torch.tensor([-4.1632, 5.0371], device=dev))


@gpu
def test_cfg_combine_coef_rejects(dev):
    from wan.backend import lib, ops
    n = 4096
    u, c = torch.from_numpy(_pair(n)[0]).to(dev), torch.from_numpy(_pair(n)[1]).to(dev)
    out, coef = torch.full_like(u, -7.0), torch.tensor([-4.0, 5.0], device=dev)
    wide = torch.zeros(2, n + 4, device=dev)
    bad = [(None, u, c, coef), (out, None, c, coef), (out, u, None, coef), (out, u, c, None), (out.cpu(), u, c, coef), (out, u.cpu(), c, coef),
           (out, u, c, coef.cpu()), (out.double(), u, c, coef), (out, u.half(), c, coef), (out, u, c, coef.double()), (out, u[:-4], c, coef),
           (out, u, c[:-4], coef), (out[::2], u[::2], c[::2], coef), (out, torch.zeros(n, 2, device=dev)[:, 0], c, coef),
           (out, wide[0, 1:n + 1], c, coef), (wide[1, 1:n + 1], u, c, coef), (out, u, c, torch.zeros(3, device=dev))]
    for args in bad:
        with pytest.raises(lib.MoviigenHipError):
            ops.cfg_combine_coef(*args)
    h, p = lib.load(), lambda t, off=0: lib.c_vp(t.data_ptr() + off)
    assert h.mg_cfg_combine_coef_f32(None, p(u), p(c), n, p(coef), None) == -1 and h.mg_cfg_combine_coef_f32(p(out), p(u), p(c), n, None, None) == -1
    assert h.mg_cfg_combine_coef_f32(p(out), p(u), p(c), -1, p(coef), None) == -2 and h.mg_cfg_combine_coef_f32(p(out), p(u, 4), p(c), n - 4, p(coef), None) == -2
    assert h.mg_cfg_combine_coef_f32(p(out, 8), p(u), p(c), n - 4, p(coef), None) == -2
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, -7.0))


@gpu
@pytest.mark.parametrize('name', ['fewer groups than lanes', 'one sweep and a partial second'])
@pytest.mark.parametrize('zs,phi', [(True, 0.7), (True, 0.0), (False, 0.7)])
def test_three_launches_against_fp64(dev, name, zs, phi):
    """stats -> coefficients -> combine against tests/guidance_ref.py in fp64 end to end.  The two coefficients carry at most 2^-22 relative
    (above), the one fma rounds once: |out - ref| <= 2^-22 (|a_u| max |u| + |a_c| max |c|) + 2^-24 max |out|"""
    from wan.backend import ops
    n = _sizes()[name]
    assert n == 2048 or n > _grid() * NT * CS_UNROLL * 4
    un, cn = _pair(n)
    u, c = torch.from_numpy(un).to(dev), torch.from_numpy(cn).to(dev)
    stats, partials, coef = _scratch(dev)
    out = torch.empty_like(u)
    ops.cfg_stats(u, c, stats, partials)
    ops.cfg_coefficients(stats, n, 5.0, zs, phi, coef)
    ops.cfg_combine_coef(out, u, c, coef)
    au, ac = coef_ref([float(v) for v in _pair_sums(n)[0]], n, 5.0, zs, phi)
    ref = combine_ref(un, cn, au, ac)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    bound = 2.0 ** -22 * (abs(au) * float(np.abs(un).max()) + abs(ac) * float(np.abs(cn).max())) + 2.0 ** -24 * float(np.abs(ref).max())
    print(f'n {n} zero_star {zs} rescale {phi}: a_u {au!r} a_c {ac!r} (device {coef.tolist()}) max err {err:.3e} bound {bound:.3e}')
    assert err <= bound


# ------------------------------------------------------------------------------------------------
# GPU: WanT2V.generate / inpaint(guidance=) on the tiny pipeline of tests/test_inpaint.py
# ------------------------------------------------------------------------------------------------
SIZE, FRAMES, STEPS, SEQ = (64, 64), 5, 6, 32
SOLVERS = ['unipc', 'dpm++']
BAND = (0.6, 0.95)                                      # steps 0, 1 and 5 of the 6-step schedule lie outside: 'cond' on both ends
KINDS = ['cond', 'cond', 'guided', 'guided', 'guided', 'cond']
C, S = True, False


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


def _call(pipe, prompts, solver, run=None, **kw):
    lats = []
    kw.setdefault('callback', lambda i, l: lats.append((i, l.clone())))
    video = (run or pipe.generate)(prompts[0], size=SIZE, frame_num=FRAMES, shift=5.0, sample_solver=solver, sampling_steps=STEPS, guide_scale=5.0,
                                   n_prompt=prompts[1], seed=0, offload_model=False, noise=W.randn((16, 2, 8, 8), 33), **kw)
    return video, lats


@pytest.fixture(scope='module')
def plain(pipe, prompts):
    """the run without a Guidance, once per solver, shared"""
    return {s: _call(pipe, prompts, s) for s in SOLVERS}


def _hand_loop(pipe, prompts, solver, dev, kinds, g=5.0, zero_star=False, rescale=0.0, plan=None):
    """the loop of WanT2V.generate(guidance=) written from the model, forward_pair, the ops and the scheduler -> the latent behind every step"""
    from wan.backend import ops
    m = pipe.model
    sched, ts = _scheduler(solver, STEPS, 5.0, device=dev)
    latent = W.randn((16, 2, 8, 8), 33).to(dev)
    pred = torch.empty_like(latent)
    stats, partials, coef = _scratch(dev)
    ctx, ctx_null = [prompts[0]], [prompts[1]]
    out = []
    for i, t_host in enumerate(ts.tolist()):
        mode = m.step_cache('compute' if plan[i] else 'skip') if plan is not None else torch.no_grad()
        if kinds[i] == 'zero':
            p = torch.zeros_like(latent)
        elif kinds[i] == 'cond':
            with mode:
                p = m([latent], t=ts[i:i + 1], context=ctx, seq_len=SEQ)[0]
        else:
            with mode:
                cond, uncond = m.forward_pair([latent], ts[i:i + 1], ctx, ctx_null, SEQ)
            p = pred
            if not zero_star and rescale == 0.0:
                ops.cfg_combine(pred, uncond[0], cond[0], g)
            else:
                ops.cfg_stats(uncond[0], cond[0], stats, partials)
                ops.cfg_coefficients(stats, latent.numel(), g, zero_star, rescale, coef)
                ops.cfg_combine_coef(pred, uncond[0], cond[0], coef)
        latent = sched.step(p.unsqueeze(0), t_host, latent.unsqueeze(0), return_dict=False)[0].squeeze(0)
        out.append(latent)
    m.drop_step_cache()
    return out


def _count_forwards(pipe, monkeypatch):
    """wrap the two methods `_sample` calls for a prediction -> the list of (method, DiT forwards it ran), one entry per call"""
    log, m = [], pipe.model
    inner = m._forward_one

    def one(*a, **kw):
        log[-1][1] += 1
        return inner(*a, **kw)
    monkeypatch.setattr(m, '_forward_one', one)
    for name in ('_guidance_pair', '_cond_prediction'):
        def wrapped(*a, _f=getattr(pipe, name), _n=name, **kw):
            log.append([_n, 0])
            return _f(*a, **kw)
        monkeypatch.setattr(pipe, name, wrapped)
    return log


@gpu
@pytest.mark.parametrize('solver', SOLVERS)
def test_scale_alone_is_guide_scale(dev, pipe, prompts, plain, solver):
    from wan.utils.guidance import Guidance
    video, lats = plain[solver]
    v, l = _call(pipe, prompts, solver, guidance=Guidance(scale=5.0))
    assert pipe.last_guidance_plan == ['guided'] * STEPS and pipe.last_step_plan is None
    assert torch.equal(v, video) and all(torch.equal(a[1], b[1]) for a, b in zip(l, lats))
    kw = dict(size=SIZE, frame_num=FRAMES, shift=5.0, sample_solver=solver, sampling_steps=STEPS, n_prompt=prompts[1], seed=0, offload_model=False,
              noise=W.randn((16, 2, 8, 8), 33))
    v3 = pipe.generate(prompts[0], guide_scale=3.0, **kw)
    assert pipe.last_guidance_plan is None
    assert torch.equal(pipe.generate(prompts[0], guide_scale=7.0, guidance=Guidance(scale=3.0), **kw), v3) and not torch.equal(v3, video)
    pipe.guidance = Guidance(scale=3.0)                                          # the object's default is what generate(guidance=None) uses
    try:
        assert torch.equal(pipe.generate(prompts[0], guide_scale=7.0, **kw), v3) and pipe.last_guidance_plan == ['guided'] * STEPS
    finally:
        pipe.guidance = None


@gpu
@pytest.mark.parametrize('solver', SOLVERS)
def test_interval_equals_hand_written_loop(dev, pipe, prompts, plain, solver, monkeypatch):
    from wan.utils.guidance import Guidance
    want = _hand_loop(pipe, prompts, solver, dev, KINDS)
    log = _count_forwards(pipe, monkeypatch)
    gd = Guidance(interval=BAND)
    video, lats = _call(pipe, prompts, solver, guidance=gd)
    assert pipe.last_guidance_plan == KINDS == gd.plan(_scheduler(solver, STEPS, 5.0)[0].sigmas.tolist()[:STEPS])
    assert [i for i, _ in lats] == list(range(STEPS))
    for i in range(STEPS):
        assert torch.equal(lats[i][1], want[i]), i
    assert torch.equal(video, pipe.vae.decode([want[-1]])[0])
    # a 'cond' step runs exactly ONE DiT forward, a 'guided' one two
    assert log == [['_cond_prediction', 1] if k == 'cond' else ['_guidance_pair', 2] for k in KINDS]
    assert not torch.equal(lats[0][1], plain[solver][1][0][1])                  # step 0 without guidance is another step


@gpu
@pytest.mark.parametrize('solver', SOLVERS)
def test_zero_star_and_rescale_equal_hand_written_loop(dev, pipe, prompts, plain, solver):
    """the three ops' numerics are pinned above: this pins the plumbing"""
    from wan.utils.guidance import Guidance
    for kinds, kw in ((['guided'] * STEPS, {}), (KINDS, dict(interval=BAND))):
        want = _hand_loop(pipe, prompts, solver, dev, kinds, zero_star=True, rescale=0.7)
        video, lats = _call(pipe, prompts, solver, guidance=Guidance(zero_star=True, rescale=0.7, **kw))
        assert pipe.last_guidance_plan == kinds
        for i in range(STEPS):
            assert torch.equal(lats[i][1], want[i]), i
        assert torch.equal(video, pipe.vae.decode([want[-1]])[0]) and torch.isfinite(video).all().item()
    assert not torch.equal(lats[-1][1], _hand_loop(pipe, prompts, solver, dev, KINDS)[-1])         # the mix is another one


@gpu
@pytest.mark.parametrize('solver', SOLVERS)
def test_zero_init_steps(dev, pipe, prompts, plain, solver, monkeypatch):
    from wan.utils.guidance import Guidance
    kinds = ['zero', 'zero'] + ['guided'] * (STEPS - 2)
    want = _hand_loop(pipe, prompts, solver, dev, kinds)      # steps 0 and 1: what the scheduler gives for a zero prediction
    log = _count_forwards(pipe, monkeypatch)
    seen = []

    def callback(i, latent):
        seen.append((i, latent.clone(), len(log)))
    _call(pipe, prompts, solver, guidance=Guidance(zero_init_steps=2), callback=callback)
    assert pipe.last_guidance_plan == kinds and [i for i, _, _ in seen] == list(range(STEPS))
    assert [n for _, _, n in seen] == [0, 0, 1, 2, 3, 4]                         # no forward on the zero steps
    for i in range(STEPS):
        assert torch.equal(seen[i][1], want[i]), i
    # video-to-video from schedule index 3 >= 2: nothing is zeroed
    frames = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (FRAMES, 50, 70, 3)).astype(np.uint8))
    ref, ref_lats = _call(pipe, prompts, solver, init_video=frames, strength=0.5)
    del log[:]
    v, lats = _call(pipe, prompts, solver, init_video=frames, strength=0.5, guidance=Guidance(zero_init_steps=2))
    assert [i for i, _ in lats] == [3, 4, 5] and pipe.last_guidance_plan[3:] == ['guided'] * 3 and len(log) == 3
    assert torch.equal(v, ref) and all(torch.equal(a[1], b[1]) for a, b in zip(lats, ref_lats))


@gpu
def test_step_cache_computes_the_first_guided_step(dev, pipe, prompts):
    """an explicit plan that would skip step 2, the first 'guided' step behind the 'cond' steps 0 and 1: it is computed (the unconditional
    residual would be missing or arbitrarily old), and the run is the one with that entry set to True by hand"""
    from wan.utils.guidance import Guidance
    gd = Guidance(interval=BAND, zero_star=True, rescale=0.7)
    asked, adjusted = [C, S, S, C, S, C], [C, S, C, C, S, C]
    video, lats = _call(pipe, prompts, 'unipc', guidance=gd, step_cache=asked)
    assert pipe.last_step_plan == adjusted and pipe.last_guidance_plan == KINDS
    ref, ref_lats = _call(pipe, prompts, 'unipc', guidance=gd, step_cache=adjusted)
    assert pipe.last_step_plan == adjusted
    assert torch.equal(video, ref) and all(torch.equal(a[1], b[1]) for a, b in zip(lats, ref_lats))
    want = _hand_loop(pipe, prompts, 'unipc', dev, KINDS, zero_star=True, rescale=0.7, plan=adjusted)
    for i in range(STEPS):
        assert torch.equal(lats[i][1], want[i]), i
    assert all('resid' not in ws and 'xin' not in ws for ws in pipe.model._ws.values())      # dropped when the loop ends
    assert torch.isfinite(video).all().item()


@gpu
@pytest.mark.parametrize('solver', SOLVERS)
def test_inpaint_with_guidance(dev, pipe, prompts, solver):
    from wan.backend import ops
    from wan.utils.guidance import Guidance
    frames = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (7, 50, 70, 3)).astype(np.uint8))
    mask = torch.zeros(50, 70, dtype=torch.uint8)
    mask[:, :35] = 255
    clip = ops.video_from_u8(frames[:FRAMES].to(dev), SIZE[1], SIZE[0])
    z0, noise = pipe.vae.encode([clip])[0], W.randn((16, 2, 8, 8), 33).to(dev)
    pm = ops.mask_from_u8(mask.view(1, 50, 70).to(dev), FRAMES, SIZE[1], SIZE[0], 0)
    lm = ops.mask_to_latent(pm, (4, 8, 8))
    video, seen = _call(pipe, prompts, solver, run=lambda p, **kw: pipe.inpaint(p, frames, mask=mask, **kw),
                        guidance=Guidance(interval=BAND, zero_star=True, zero_init_steps=1, rescale=0.7))
    assert pipe.last_guidance_plan == ['zero'] + KINDS[1:] and [i for i, _ in seen] == list(range(STEPS))
    # the kept-cell invariant: at every callback(i, latent) the kept cells hold (1 - sigma_{i+1}) z0 + sigma_{i+1} noise, the bits of ops.lincomb
    sigmas = _scheduler(solver, STEPS, 5.0)[0].sigmas.tolist()
    kept = (lm == 0).expand_as(z0)
    assert kept.any().item() and not kept.all().item()
    for i, latent in seen:
        s = sigmas[i + 1]
        want = ops.lincomb(torch.empty_like(z0), [(z0, 1.0 - s), (noise, s)])
        assert torch.equal(latent[kept], want[kept]), i
    assert sigmas[-1] == 0.0 and torch.equal(seen[-1][1][kept], z0[kept])
    kept_px = (pm == 0).expand_as(video)
    assert torch.equal(video[kept_px], clip[kept_px]) and torch.isfinite(video).all().item()


@gpu
def test_invalid_guidance_raises_before_any_gpu_work(dev, pipe, prompts, monkeypatch):
    import wan
    from wan.utils.guidance import Guidance

    def no_gpu_work(*a, **kw):
        raise AssertionError('the prompt was encoded: the argument check came too late')
    monkeypatch.setattr(pipe, '_encode', no_gpu_work)
    for bad in (5.0, (0.2, 0.8), 'cfg_zero_star', dict(rescale=0.5)):
        with pytest.raises(ValueError, match='guidance'):
            _call(pipe, prompts, 'unipc', guidance=bad)
    with pytest.raises(ValueError):
        _call(pipe, prompts, 'unipc', guidance=Guidance(rescale=0.5), strength=0.5)          # (strength < 1 without init_video, as without a Guidance)
    with pytest.raises(ValueError, match='rescale'):
        Guidance(rescale=1.5)
    with pytest.raises(ValueError, match='guidance'):
        wan.WanT2V(pipe.config, '', device_id=0, model=pipe.model, vae=pipe.vae, guidance=0.5)
