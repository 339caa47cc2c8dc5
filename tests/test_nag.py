"""Normalized attention guidance (nag=NAG(...)): the host rule wan/utils/nag.py, the row-wise mix mg_nag_combine_bf16,
WanModel.forward / forward_pair(nag=) and the sampling loop.

CPU: declarations, the new keywords, NAG's validation, the launcher flags, and the properties of the restatement tests/nag_ref.py (without
NAG it IS the oracle, bit for bit; scale 1 and an equal negative prompt change nothing).
GPU: the kernel against the fp64 row reference within half a bf16 ulp plus k 2^-24 M, k derived below from the kernel's order of
operations; its bit-exact properties; WanModel.forward(nag=) against the bf16-emulating restatement at the tolerance of the same comparison
without NAG; forward_pair, the prompt K/V cache, the step cache; WanT2V.generate / inpaint / windows on the tiny pipeline of
tests/test_guidance.py bit for bit against loops written here from the model, the ops and the scheduler.
"""
import functools
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import weights as W
from abi_ref import header_declarations
from nag_ref import dit_forward_nag, nag_rows

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'mg_nag_combine_bf16'

# csrc/nag.hip, nag_combine_wave_kernel — the fp32 operations behind one output element, u = 2^-24 each, relative to a magnitude <= M:
#   g = fma(s, p, -((s - 1) n))                  2   (s - 1 is exact)
#   Np: a lane adds <= 16 chunks x 8 elements in order (128 additions, zeros past the row add exactly), then 6 butterfly steps       134
#   Ng: the same chain                                                                                                         134
#       ... and the roundings of the g_j it adds: sum_j 2 u (s|p_j| + (s-1)|n_j|) = 2 kappa u Ng, kappa = sum (s|p|+(s-1)|n|) / sum |g|   2 kappa
#   c = (tau Np) / (Ng + 1e-7): one product, one sum (1e-7f is not 1e-7: far below u of the sum), one division counted twice       4
#   alpha c: 1;  1 - alpha: 1;  (1 - alpha) p: 1;  the final fma: 1                                                              4
#   the rounding to bf16 acts on the fp32 value, not on the reference: (1 + 2^-8) on all of the above                             2
# The side the comparison Ng > tau Np falls on can differ from the reference's only when the two sums are closer than their own error,
# where c is within that error of 1 on both sides: c is continuous at the threshold and the same count covers it.
K_CHAIN = 2 + 134 + 134 + 4 + 4 + 2
U = 2.0 ** -24
HALF_ULP_BF16 = 2.0 ** -8
GRID_ROWS = 2048 * 4            # rows one sweep of the capped grid covers (NAG_MAX_GRID workgroups of 4 waves)

PARAMS = [(1.0, 2.5, 0.25), (4.0, 2.5, 0.5), (11.0, 2.5, 0.25), (11.0, 1.2, 1.0), (3.0, 100.0, 1.0)]
# (rows, dim, extra row stride); the planted rows need 5: the 1-row shapes are one random row
SHAPES = [(1, 8, 0), (5, 128, 0), (1, 136, 0), (5, 520, 0), (5, 5120, 0), (1, 8192, 0), (8197, 128, 0), (3, 5120, 64)]
SHAPE_IDS = [f'r{r}-d{d}' + ('-views' if e else '') for r, d, e in SHAPES]
assert SHAPES[6][0] > GRID_ROWS


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _launcher(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', 'inference', 'generate.py'))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
def test_declarations():
    """header, ctypes table and ops agree on mg_nag_combine_bf16; the new keyword is on every surface"""
    from wan.backend import lib, ops
    from wan.modules import WanModel
    from wan.text2video import WanT2V
    hdr = open(os.path.join(ROOT, 'include', 'moviigen_hip.h')).read()
    decl = header_declarations()
    assert NAME in decl, f'include/moviigen_hip.h does not declare {NAME}'
    restype, want = decl[NAME]
    assert restype is lib.c_int and lib.SIGNATURES[NAME] == want and len(want) == 12 and NAME not in lib._RESTYPE
    assert hdr.index(NAME) < hdr.index('#ifdef MG_AB_BUILD')                 # the product section
    assert list(inspect.signature(ops.nag_combine).parameters) == ['zp', 'zn', 'out', 'scale', 'tau', 'alpha']
    for fn in (WanT2V.generate, WanT2V.__init__):
        assert inspect.signature(fn).parameters['nag'].default is None
    inspect.signature(WanT2V.inpaint).bind(None, 'prompt', 'clip', nag=None)
    for fn in (WanModel.forward, WanModel.forward_pair):
        p = inspect.signature(fn).parameters['nag']
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert 'test_nag_combine' in open(os.path.join(ROOT, 'moviigen1.1_amd', 'csrc', 'tools', 'selftest.cpp')).read()


def test_nag_validation():
    from wan.utils.nag import NAG
    n = NAG(4)
    assert (n.scale, n.tau, n.alpha, n.n_prompt) == (4.0, 2.5, 0.25, None) and n.params == (4.0, 2.5, 0.25)
    n = NAG(np.float32(1), tau=1, alpha=np.int64(1), n_prompt='blurry')
    assert n.params == (1.0, 1.0, 1.0) and n.n_prompt == 'blurry' and 'blurry' in repr(n)
    assert NAG(64, tau=1e6, alpha=0).params == (64.0, 1e6, 0.0)
    emb = torch.zeros(3, 8)
    assert NAG(2, n_prompt=emb).n_prompt is emb and 'embedding' in repr(NAG(2, n_prompt=emb))
    nan, inf = float('nan'), float('inf')
    for bad in (dict(scale=0.99), dict(scale=64.01), dict(scale=nan), dict(scale=inf), dict(scale=-4), dict(scale='a'), dict(scale=None),
                dict(scale=True), dict(scale=4, tau=0.99), dict(scale=4, tau=nan), dict(scale=4, tau=inf), dict(scale=4, tau=None),
                dict(scale=4, alpha=-0.01), dict(scale=4, alpha=1.01), dict(scale=4, alpha=nan), dict(scale=4, alpha='x'), dict(scale=4, alpha=False)):
        with pytest.raises(ValueError):
            NAG(**bad)
    with pytest.raises(TypeError):
        NAG()                                                                   # no default scale: nothing is recommended


def test_launcher_flags_reach_generate(tmp_path, monkeypatch):
    """the four flags parse, are declared in the launcher's table, and reach WanT2V.generate / inpaint as one NAG; without them the call
    carries no `nag` (a recording pipeline); the dependants without --nag_scale are refused"""
    from wan.utils.nag import NAG
    g = _launcher('mg_generate_nag')
    assert {'--nag_scale', '--nag_tau', '--nag_alpha', '--nag_negative'} <= {f for f, _ in g.FLAGS}
    a = g._parse_args(['--ckpt_dir', '/x'])
    assert a.nag_scale is None and a.nag_tau is None and a.nag_alpha is None and a.nag_negative is None and a.nag is None
    a = g._parse_args(['--ckpt_dir', '/x', '--nag_scale', '4'])
    assert isinstance(a.nag, NAG) and a.nag.params == (4.0, 2.5, 0.25) and a.nag.n_prompt is None
    a = g._parse_args(['--ckpt_dir', '/x', '--nag_scale', '11', '--nag_tau', '3', '--nag_alpha', '0.5', '--nag_negative', 'blurry, static'])
    assert a.nag.params == (11.0, 3.0, 0.5) and a.nag.n_prompt == 'blurry, static'
    for bad in (['--nag_tau', '3'], ['--nag_alpha', '0.5'], ['--nag_negative', 'x'], ['--nag_scale', '0.5'], ['--nag_scale', '65'],
                ['--nag_scale', 'nan'], ['--nag_scale', '4', '--nag_tau', '0.5'], ['--nag_scale', '4', '--nag_alpha', '1.5']):
        with pytest.raises(AssertionError):
            g._parse_args(['--ckpt_dir', '/x'] + bad)
    calls = []

    class Pipe:
        last_step_plan = None
        last_guidance_plan = ['cond', 'cond']

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
    g.generate(g._parse_args(base + ['--nag_scale', '4', '--nag_alpha', '0.5', '--guide_interval', '0,0']))
    g.generate(g._parse_args(base + ['--nag_scale', '2', '--nag_negative', 'blurry', '--init_video', str(tmp_path / 'clip.npy'), '--keep_frames', '1']))
    assert [c[0] for c in calls] == ['generate', 'generate', 'inpaint']
    assert 'nag' not in calls[0][1]
    assert calls[1][1]['nag'].params == (4.0, 2.5, 0.5) and calls[1][1]['guidance'].interval == (0.0, 0.0)
    assert calls[2][1]['nag'].params == (2.0, 2.5, 0.25) and calls[2][1]['nag'].n_prompt == 'blurry' and calls[2][1]['keep_frames'] == 1
    WanT2V = __import__('wan.text2video', fromlist=['WanT2V']).WanT2V
    inspect.signature(WanT2V.generate).bind(None, 'prompt', **calls[1][1])          # every keyword the launcher passes is one generate takes


def test_pipeline_refuses_a_model_without_the_keyword():
    from wan.text2video import _checked_nag
    from wan.utils.nag import NAG

    class Own(torch.nn.Module):
        def forward(self, x, t, context, seq_len):
            return x
    assert _checked_nag(None, Own()) is None
    with pytest.raises(ValueError, match='nag'):
        _checked_nag(NAG(4), Own())
    with pytest.raises(ValueError, match='nag'):
        _checked_nag(NAG(4), lambda x, t, context, seq_len: x)
    for bad in (4.0, (4, 2.5, 0.25), 'nag', dict(scale=4)):
        with pytest.raises(ValueError, match='nag'):
            _checked_nag(bad)
    import wan
    n = NAG(4)
    assert _checked_nag(n, wan.modules.WanModel(**W.TINY_DIT)) is n


# the restatement's inputs, shared by the CPU properties and the GPU forwards
DIT_CASES = [('tiny', W.TINY_DIT), ('hd128', W.SMALL_DIT_HD128)]
SEQ = 32
FWD_PARAMS = [(4.0, 2.5, 0.5), (11.0, 2.5, 0.25)]
TOL = 1.2e-2                    # test_gpu_parity.py::test_dit_forward_vs_reference (c): the engine against the bf16-emulating oracle


def _dit_inputs(cfg):
    return W.randn((16, 2, 8, 8), 21), torch.tensor([417]), W.randn((7, cfg['text_dim']), 22), W.randn((5, cfg['text_dim']), 23)


@functools.lru_cache(maxsize=None)
def _ref(tag, nag=None, equal=False):
    """the bf16-emulating restatement, computed once per case -> (output, clipped rows per block)"""
    cfg = dict(DIT_CASES)[tag]
    lat, t, ctx, neg = _dit_inputs(cfg)
    log = []
    out = dit_forward_nag(W.make_dit_params(cfg, 0), cfg, lat, t, ctx, SEQ, None if nag is None else (ctx.clone() if equal else neg), nag,
                          emulate_bf16=True, clip_log=log)
    return out, log


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize('tag', [c[0] for c in DIT_CASES])
def test_restatement_properties(tag):
    from oracle import dit
    cfg = dict(DIT_CASES)[tag]
    lat, t, ctx, _ = _dit_inputs(cfg)
    P = W.make_dit_params(cfg, 0)
    plain = _ref(tag)[0]
    assert torch.equal(plain, dit.dit_forward(P, cfg, lat, t, ctx, SEQ, emulate_bf16=True))            # without NAG it IS the oracle
    assert torch.equal(dit_forward_nag(P, cfg, lat, t, ctx, SEQ), dit.dit_forward(P, cfg, lat, t, ctx, SEQ))
    assert torch.equal(_ref(tag, (1.0, 2.5, 0.25))[0], plain)                                          # scale 1
    for nag in FWD_PARAMS:
        assert torch.equal(_ref(tag, nag, equal=True)[0], plain)                                       # negative == prompt
        out, log = _ref(tag, nag)
        assert rel_l2(out, plain) >= 5 * TOL and len(log) == cfg['num_layers']                         # NAG is no small change
    if tag == 'hd128':          # both branches of the clip act inside the model
        for clipped in _ref(tag, FWD_PARAMS[0])[1]:
            assert 0.1 <= clipped.double().mean().item() <= 0.9


# ------------------------------------------------------------------------------------------------
# GPU: the kernel
# ------------------------------------------------------------------------------------------------
def _threshold_row(p, z, s, tau, above):
    """n = p + beta z (bf16) with beta bisected so that Ng of g = s p - (s - 1) n lies within 1e-3 relative of tau Np, on the asked side"""
    p64 = p.double()
    Np = p64.abs().sum().item()

    def ratio(beta):
        n = (p64 + beta * z.double()).to(torch.bfloat16)
        return n, ((s * p64 - (s - 1.0) * n.double()).abs().sum().item()) / (tau * Np)
    lo, hi = 0.0, 1.0
    while ratio(hi)[1] < 1.0:
        hi *= 2.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if ratio(mid)[1] < 1.0 else (lo, mid)
    # walk off the threshold to the asked side in steps far below 1e-3
    beta, step = (hi, 1.0 + 2e-5) if above else (lo, 1.0 - 2e-5)
    for _ in range(200):
        n, r = ratio(beta)
        if (r > 1.0) == above and abs(r - 1.0) < 1e-3 and r != 1.0:
            return n
        beta *= step
    raise AssertionError('no threshold row found')


@functools.lru_cache(maxsize=None)
def _case(si, pi):
    """inputs of shape SHAPES[si] at PARAMS[pi] (bf16, CPU) with their fp64 reference -> (p, n, ref dict, planted: name -> row)"""
    rows, dim, _ = SHAPES[si]
    s, tau, alpha = PARAMS[pi]
    p = W.randn((rows, dim), 100 + si).to(torch.bfloat16)
    z = W.randn((rows, dim), 200 + si)
    # the negative rows range from independent of p to nearly p: the clip acts on some rows and not on others
    rho = torch.tensor([0.0, 0.5, 0.9, 0.97, 0.995])[torch.arange(rows) % 5][:, None]
    n = (rho * p.float() + (1 - rho * rho).sqrt() * z).to(torch.bfloat16)
    planted = {}
    if rows >= 5:
        base = 0 if rows == 5 else 4096             # (in the long launch: rows of the second sweep's neighbourhood, 4100 among them)
        planted = dict(p_zero=base, both_zero=base + 1, equal=base + 2, large=base + 3, above=base + 4)
        p[planted['p_zero']] = 0
        p[planted['both_zero']] = 0
        n[planted['both_zero']] = 0
        n[planted['equal']] = p[planted['equal']]
        p[planted['large']] = (p[planted['large']].float() * 1e4).to(torch.bfloat16)
        n[planted['large']] = (n[planted['large']].float() * 1e4).to(torch.bfloat16)
        if rows > 5:
            planted['below'] = base + 5
        if s > 1.0:             # (scale 1: g is p, no row is near a threshold)
            n[planted['above']] = _threshold_row(p[planted['above']], z[planted['above']], s, tau, True)
            if 'below' in planted:
                n[planted['below']] = _threshold_row(p[planted['below']], z[planted['below']], s, tau, False)
    return p, n, nag_rows(p, n, s, tau, alpha), planted


def _strided(t, extra, dev):
    """t on the device as a column-slice view with row stride dim + extra"""
    if not extra:
        return t.to(dev)
    buf = torch.zeros(t.shape[0], t.shape[1] + extra, dtype=t.dtype, device=dev)
    view = buf[:, :t.shape[1]]
    view.copy_(t)
    return view


def test_kernel_cases_cover_both_branches():
    """counted on the reference, over all cases: at least 10 % of the rows clipped and at least 10 % not; the planted rows are what they claim"""
    clipped = total = 0
    for si in range(len(SHAPES)):
        for pi, (s, tau, alpha) in enumerate(PARAMS):
            p, n, ref, planted = _case(si, pi)
            clipped += int(ref['clipped'].sum())
            total += ref['clipped'].numel()
            if planted:
                assert ref['c'][planted['p_zero']].item() == (0.0 if s > 1.0 else 1.0) and ref['out'][planted['p_zero']].abs().max().item() == 0.0
                assert ref['out'][planted['both_zero']].abs().max().item() == 0.0 and not ref['clipped'][planted['both_zero']]
                assert torch.equal(p[planted['equal']], n[planted['equal']])
                assert p[planted['large']].float().abs().max().item() > 1e4
                if s > 1.0:
                    assert ref['clipped'][planted['above']] and ref['margin'][planted['above']] < 1e-3
                    if 'below' in planted:
                        assert not ref['clipped'][planted['below']] and ref['margin'][planted['below']] < 1e-3
    assert 0.1 <= clipped / total <= 0.9, clipped / total


@gpu
@pytest.mark.parametrize('pi', range(len(PARAMS)), ids=[f's{s:g}-tau{t:g}-a{a:g}' for s, t, a in PARAMS])
@pytest.mark.parametrize('si', range(len(SHAPES)), ids=SHAPE_IDS)
def test_nag_combine_against_fp64(dev, si, pi):
    from wan.backend import ops
    rows, dim, extra = SHAPES[si]
    s, tau, alpha = PARAMS[pi]
    p, n, ref, planted = _case(si, pi)
    zp, zn = _strided(p, extra, dev), _strided(n, extra, dev)
    out = _strided(torch.full_like(p, float('nan')), extra, dev)
    assert ops.nag_combine(zp, zn, out, s, tau, alpha) is out
    got = out.cpu()
    assert torch.isfinite(got.float()).all().item()
    assert torch.equal(zp.cpu(), p) and torch.equal(zn.cpu(), n)                  # the inputs are only read
    k = K_CHAIN + 2.0 * ref['kappa'][:, None]
    err = (got.double() - ref['out']).abs()
    bound = HALF_ULP_BF16 * ref['out'].abs() + k * U * ref['M']
    worst = (err - bound).max().item()
    print(f'nag_combine {SHAPE_IDS[si]} s={s:g} tau={tau:g} alpha={alpha:g}: max err / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}, '
          f'kappa <= {ref["kappa"].max().item():.1f}, clipped {int(ref["clipped"].sum())} of {rows}')
    assert worst <= 0.0, worst
    # the exact properties
    if s == 1.0:
        assert torch.equal(got.view(torch.int16), p.view(torch.int16))
    if planted:
        assert torch.equal(got[planted['equal']].view(torch.int16), p[planted['equal']].view(torch.int16))
        assert got[planted['both_zero']].float().abs().max().item() == 0.0
        if s > 1.0:
            assert got[planted['p_zero']].float().abs().max().item() == 0.0
    # two launches give the same bytes; in place (out is zp) equals out of place
    again = _strided(torch.zeros_like(p), extra, dev)
    ops.nag_combine(zp, zn, again, s, tau, alpha)
    assert torch.equal(again.view(torch.int16), out.view(torch.int16))
    assert ops.nag_combine(zp, zn, zp, s, tau, alpha) is zp
    assert torch.equal(zp.view(torch.int16), out.view(torch.int16)) and torch.equal(zn.cpu(), n)
    if extra:                   # nothing behind a row's dim elements was written
        assert out._base[:, dim:].float().abs().max().item() == 0.0 and zp._base[:, dim:].float().abs().max().item() == 0.0
    if rows > GRID_ROWS:        # a row's bits do not depend on the launch it is part of: row 4100 alone
        r = 4100
        alone = torch.empty(1, dim, dtype=torch.bfloat16, device=dev)
        ops.nag_combine(p[r:r + 1].to(dev), n[r:r + 1].to(dev), alone, s, tau, alpha)
        assert torch.equal(alone[0].view(torch.int16), out[r].view(torch.int16))


@gpu
def test_nag_combine_rejects(dev):
    """argument checks only: every refusal returns before anything is launched"""
    from wan.backend import lib, ops
    h = lib.load()
    fn = getattr(h, NAME)
    P = lambda t, off=0: lib.ctypes.c_void_p(t.data_ptr() + off)    # noqa: E731
    rows, dim = 4, 64
    zp, zn, out = (torch.zeros(rows, dim, dtype=torch.bfloat16, device=dev) for _ in range(3))
    ok = lambda **kw: fn(*[kw.get(k, v) for k, v in dict(zp=P(zp), ldp=dim, zn=P(zn), ldn=dim, out=P(out), ldo=dim, rows=rows, dim=dim,      # noqa: E731
                                                          scale=4.0, tau=2.5, alpha=0.5, stream=None).items()])
    assert ok() == 0 and ok(rows=0) == 0 and ok(out=P(zp)) == 0                                    # in place on zp is allowed
    for kw in (dict(zp=None), dict(zn=None), dict(out=None)):
        assert ok(**kw) == -1, kw
    nan, inf = float('nan'), float('inf')
    for kw in (dict(scale=0.5), dict(scale=65.0), dict(scale=nan), dict(scale=inf), dict(tau=0.5), dict(tau=nan), dict(tau=inf), dict(alpha=-0.1),
               dict(alpha=1.1), dict(alpha=nan), dict(out=P(zn)), dict(out=P(zp, 32)), dict(out=P(zp), ldo=dim + 8, rows=2)):
        assert ok(**kw) == -1, kw
    for kw in (dict(dim=0), dict(dim=-8), dict(dim=60, ldp=64), dict(dim=8200, ldp=8200, ldn=8200, ldo=8200), dict(ldp=dim + 4), dict(ldn=dim + 4),
               dict(ldo=dim + 4), dict(ldp=dim - 8), dict(ldn=dim - 8), dict(ldo=dim - 8), dict(rows=-1), dict(zp=P(zp, 2)), dict(zn=P(zn, 8)),
               dict(out=P(out, 4))):
        assert ok(**kw) == -2, kw
    torch.cuda.synchronize()
    assert out.float().abs().max().item() == 0.0
    # the wrapper's own checks
    E = lib.MoviigenHipError
    f32 = torch.zeros(rows, dim, device=dev)
    wide = torch.zeros(rows, 2 * dim, dtype=torch.bfloat16, device=dev)
    for args in ((f32, zn, out), (zp, f32, out), (zp, zn, f32), (zp.cpu(), zn, out), (zp[:2], zn, out), (zp, zn[:, :32], out), (zp, zn, out.view(-1)),
                 (zp, zn, wide.t()[:rows, :dim]), (wide[:, 4:4 + dim], zn, out), (zp, wide[:, ::2], out), (None, zn, out)):
        with pytest.raises(E):
            ops.nag_combine(*args, 4.0, 2.5, 0.5)
    for params in ((0.5, 2.5, 0.5), (65.0, 2.5, 0.5), (4.0, 0.5, 0.5), (4.0, inf, 0.5), (4.0, 2.5, 1.5), (nan, 2.5, 0.5)):
        with pytest.raises(E):
            ops.nag_combine(zp, zn, out, *params)
    with pytest.raises(E):
        ops.nag_combine(zp, zn, zn, 4.0, 2.5, 0.5)                               # out may not be zn: the library's refusal
    empty = torch.zeros(0, dim, dtype=torch.bfloat16, device=dev)
    assert ops.nag_combine(empty, empty, empty, 4.0, 2.5, 0.5) is empty


# ------------------------------------------------------------------------------------------------
# GPU: WanModel
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(tag):
    import wan
    cfg = dict(DIT_CASES)[tag]
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(W.make_dit_params(cfg, 0))
    return m.to('cuda:0')


def _gpu_inputs(tag, dev):
    lat, t, ctx, neg = _dit_inputs(dict(DIT_CASES)[tag])
    return lat.to(dev), t.to(dev), ctx.to(dev), neg.to(dev)


def _count(monkeypatch, obj, name, log, key=lambda a, kw: 1):
    real = getattr(obj, name)

    def counting(*a, **kw):
        log.append(key(a, kw))
        return real(*a, **kw)
    monkeypatch.setattr(obj, name, counting)


@gpu
@pytest.mark.parametrize('tag', [c[0] for c in DIT_CASES])
def test_forward_against_the_restatement(dev, tag):
    from wan.utils.nag import NAG
    m = _model(tag)
    lat, t, ctx, neg = _gpu_inputs(tag, dev)
    plain_ref = _ref(tag)[0]
    plain = m([lat], t=t, context=[ctx], seq_len=SEQ)[0]
    assert rel_l2(plain, plain_ref) < TOL
    for params in FWD_PARAMS:
        ref = _ref(tag, params)[0]
        sep = rel_l2(ref, plain_ref)
        assert sep >= 5 * TOL                    # a forward that ignores nag, or mixes wrongly, cannot pass below
        out = m([lat], t=t, context=[ctx], seq_len=SEQ, nag=(NAG(*params), [neg]))[0]
        err = rel_l2(out, ref)
        print(f'forward(nag={params}) {tag}: rel-L2 {err:.2e} against the restatement, NAG moves the output by {sep:.2e}')
        assert out.dtype == torch.float32 and tuple(out.shape) == tuple(lat.shape) and err < TOL
    assert torch.equal(m([lat], t=t, context=[ctx], seq_len=SEQ)[0], plain)     # the plain forward is what it was


@gpu
@pytest.mark.parametrize('tag', [c[0] for c in DIT_CASES])
def test_scale_one_and_equal_prompts_are_the_plain_forward(dev, tag, monkeypatch):
    import wan.modules.model as mm
    from wan.backend import ops
    from wan.utils.nag import NAG
    m = _model(tag)
    lat, t, ctx, neg = _gpu_inputs(tag, dev)
    plain = m([lat], t=t, context=[ctx], seq_len=SEQ)[0].clone()
    cross, mixes = [], []
    _count(monkeypatch, mm, 'attend', cross, key=lambda a, kw: bool(kw.get('packed')))
    _count(monkeypatch, ops, 'nag_combine', mixes)
    layers = len(m.blocks)
    m([lat], t=t, context=[ctx], seq_len=SEQ)
    assert sum(cross) == layers and not mixes                                   # one cross-attention launch per block, no mix
    for nag in ((NAG(1, 2.5, 0.25), [neg]), (NAG(4, 2.5, 0.5), [ctx.clone()]), (NAG(11, 2.5, 0.25), [ctx.clone()])):
        del cross[:], mixes[:]
        out = m([lat], t=t, context=[ctx], seq_len=SEQ, nag=nag)[0]
        assert sum(cross) == 2 * layers and len(mixes) == layers                # both kernels really ran
        assert torch.equal(out, plain)
    for bad in (NAG(4), (NAG(4), neg), (NAG(4), [neg, neg]), ((4, 2.5, 0.25), [neg]), (NAG(4), [neg[0]])):
        with pytest.raises(ValueError, match='nag'):
            m([lat], t=t, context=[ctx], seq_len=SEQ, nag=bad)


@gpu
@pytest.mark.parametrize('tag', [c[0] for c in DIT_CASES])
def test_forward_pair(dev, tag, monkeypatch):
    from wan.utils.nag import NAG
    m = _model(tag)
    lat, t, ctx, neg = _gpu_inputs(tag, dev)
    other = W.randn((6, dict(DIT_CASES)[tag]['text_dim']), 24).to(dev)
    for negs in ([neg], [other]):               # NAG's negative prompt is the pair's, or a third prompt
        nag = (NAG(4, 2.5, 0.5), negs)
        cond = m([lat], t=t, context=[ctx], seq_len=SEQ, nag=nag)[0].clone()
        uncond = m([lat], t=t, context=[neg], seq_len=SEQ)[0].clone()
        a, b = m.forward_pair([lat], t, [ctx], [neg], SEQ, nag=nag)
        assert torch.equal(a[0], cond) and torch.equal(b[0], uncond) and not torch.equal(cond, m([lat], t=t, context=[ctx], seq_len=SEQ)[0])
        monkeypatch.setenv('MOVIIGEN_CFG_SHARED_PREFIX', '0')
        a, b = m.forward_pair([lat], t, [ctx], [neg], SEQ, nag=nag)
        assert torch.equal(a[0], cond) and torch.equal(b[0], uncond)
        monkeypatch.delenv('MOVIIGEN_CFG_SHARED_PREFIX')


@gpu
def test_negative_prompt_kv_are_made_once(dev, monkeypatch):
    import wan
    from wan.utils.nag import NAG
    cfg = W.TINY_DIT
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(W.make_dit_params(cfg, 0))
    m.to(dev)
    lat, t, ctx, neg = _gpu_inputs('tiny', dev)
    made = []
    _count(monkeypatch, m, '_cross_kv', made, key=lambda a, kw: a[0])
    nag = (NAG(4, 2.5, 0.5), [neg])
    a = m([lat], t=t, context=[ctx], seq_len=SEQ, nag=nag)[0].clone()
    assert sorted(made) == sorted(list(range(cfg['num_layers'])) * 2)           # per block: the prompt's and the negative prompt's
    b = m([lat], t=t, context=[ctx], seq_len=SEQ, nag=nag)[0]
    m([lat], t=t, context=[neg], seq_len=SEQ)                                   # ... which a plain forward of that prompt shares
    assert len(made) == 2 * cfg['num_layers'] and torch.equal(a, b)


@gpu
def test_step_cache_keeps_nag_residuals_apart(dev):
    from wan.backend import ops
    from wan.utils.nag import NAG
    cfg = W.TINY_DIT
    m = _model('tiny')
    lat, t, ctx, neg = _gpu_inputs('tiny', dev)
    lat2, t2 = W.randn((16, 2, 8, 8), 25).to(dev), torch.tensor([380], device=dev)
    nag = (NAG(4, 2.5, 0.5), [neg])
    m.drop_step_cache()
    try:
        plain = m([lat], t=t, context=[ctx], seq_len=SEQ)[0].clone()
        guided = m([lat], t=t, context=[ctx], seq_len=SEQ, nag=nag)[0].clone()
        with m.step_cache('compute'):
            assert torch.equal(m([lat], t=t, context=[ctx], seq_len=SEQ)[0], plain)
        with m.step_cache('skip'):
            with pytest.raises(RuntimeError, match='no residual'):              # a plain forward's residual is not a NAG forward's
                m([lat], t=t, context=[ctx], seq_len=SEQ, nag=nag)
        with m.step_cache('compute'):
            assert torch.equal(m([lat], t=t, context=[ctx], seq_len=SEQ, nag=nag)[0], guided)
            ws = next(iter(m._ws.values()))
            r = (ws['x'] - ws['xin']).clone()
        table = ws['resid']
        assert torch.equal(table[m._resid_key(ctx, (nag[0], neg))][1], r) and not torch.equal(table[m._ctx_key(ctx)][1], r)
        with m.step_cache('skip'):
            got = m([lat2], t=t2, context=[ctx], seq_len=SEQ, nag=nag)[0].clone()
            with pytest.raises(RuntimeError, match='no residual'):              # other parameters: another residual
                m([lat2], t=t2, context=[ctx], seq_len=SEQ, nag=(NAG(4, 2.5, 0.25), [neg]))
        # the skipped forward from public ops: patchify -> gemm -> lincomb(x, r) -> ln_modulate -> head_gemm -> unpatchify
        d, L = m.dim, SEQ
        tok = torch.empty(L, cfg['in_dim'] * 4, dtype=torch.bfloat16, device=dev)
        ops.patchify(lat2, 2, 2, tok)
        x = torch.empty(L, d, device=dev)
        ops.gemm(tok, m.patch_embedding.weight.data.reshape(d, -1), m.patch_embedding.bias, ops.BIAS_F32, x)
        e, _ = m.time_embeddings(t2)
        hmod = ops.add_rows(m.head.modulation.data.reshape(2, d), e.reshape(1, d), torch.empty(2, d, device=dev), 1)
        hf = ops.ln_modulate(ops.lincomb(torch.empty_like(x), [(x, 1.0), (r, 1.0)]), hmod[1], hmod[0], True, m.eps, torch.empty_like(x))
        y = ops.head_gemm(hf, m.head.head.weight, m.head.head.bias, torch.empty(L, 4 * cfg['out_dim'], device=dev))
        want = ops.unpatchify(y, cfg['out_dim'], 2, 4, 4, 2, 2, torch.empty(cfg['out_dim'], 2, 8, 8, device=dev))
        assert torch.equal(got, want)
    finally:
        m.drop_step_cache()


# ------------------------------------------------------------------------------------------------
# GPU: WanT2V.generate / inpaint on the tiny pipeline of tests/test_guidance.py
# ------------------------------------------------------------------------------------------------
SOLVERS = ['unipc', 'dpm++']
SIZE, FRAMES, STEPS = (64, 64), 5, 4


def _scheduler(solver, n, shift, device):
    from wan.utils import FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, get_sampling_sigmas, retrieve_timesteps
    if solver == 'unipc':
        s = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
        s.set_timesteps(n, device=device, shift=shift)
        return s, s.timesteps
    s = FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    ts, _ = retrieve_timesteps(s, device=device, sigmas=get_sampling_sigmas(n, shift))
    return s, ts


@pytest.fixture(scope='module')
def pipe(dev):
    import wan
    from vae_encode_ref import make_vae_encoder_params
    from wan.configs import Config
    cfg = W.TINY_DIT
    model = wan.modules.WanModel(**cfg)
    model.load_state_dict(W.make_dit_params(cfg, 0))
    Pv = W.make_vae_params(8, 1)
    Pv.update(make_vae_encoder_params(8, 101))
    vae = wan.modules.WanVAE(state_dict=Pv, device=dev)
    conf = Config(num_train_timesteps=1000, param_dtype=torch.bfloat16, vae_stride=(4, 8, 8), patch_size=(1, 2, 2), sample_neg_prompt='',
                  vae_checkpoint='', text_len=cfg['text_len'])
    return wan.WanT2V(conf, '', device_id=0, model=model, vae=vae)


@pytest.fixture(scope='module')
def prompts(dev):
    d = W.TINY_DIT['text_dim']
    return W.randn((9, d), 31).to(dev), W.randn((5, d), 32).to(dev), W.randn((6, d), 34).to(dev)


def _call(pipe, prompts, solver, run=None, frames=FRAMES, lat=(16, 2, 8, 8), steps=STEPS, **kw):
    lats = []
    kw.setdefault('callback', lambda i, l: lats.append((i, l.clone())))
    video = (run or pipe.generate)(prompts[0], size=SIZE, frame_num=frames, shift=5.0, sample_solver=solver, sampling_steps=steps, guide_scale=5.0,
                                   n_prompt=prompts[1], seed=0, offload_model=False, noise=W.randn(lat, 33), **kw)
    return video, lats


def _loop(pipe, solver, dev, predict, lat=(16, 2, 8, 8), steps=STEPS, after=None):
    """the sampling loop from the scheduler and `predict(latent, t)` alone -> the latent behind every step"""
    sched, ts = _scheduler(solver, steps, 5.0, dev)
    latent = W.randn(lat, 33).to(dev)
    out = []
    for i, t_host in enumerate(ts.tolist()):
        with torch.no_grad():
            pred = predict(latent, ts[i:i + 1])
        latent = sched.step(pred.unsqueeze(0), t_host, latent.unsqueeze(0), return_dict=False)[0].squeeze(0)
        if after is not None:
            after(i, latent, sched)
        out.append(latent.clone())
    return out


def _same(lats, want, steps=STEPS):
    assert [i for i, _ in lats] == list(range(steps))
    for i in range(steps):
        assert torch.equal(lats[i][1], want[i]), i


@gpu
@pytest.mark.parametrize('solver', SOLVERS)
def test_negative_prompt_at_one_forward_per_step(dev, pipe, prompts, solver, monkeypatch):
    """the recipe: Guidance(interval=(0, 0)) makes every step 'cond', NAG carries the negative prompt"""
    from wan.utils.guidance import Guidance
    from wan.utils.nag import NAG
    m, nag, every_cond = pipe.model, NAG(4, 2.5, 0.5), Guidance(interval=(0.0, 0.0))
    want = _loop(pipe, solver, dev, lambda x, t: m([x], t=t, context=[prompts[0]], seq_len=SEQ, nag=(nag, [prompts[1]]))[0])
    without, lats0 = _call(pipe, prompts, solver, guidance=every_cond)
    assert pipe.last_nag is None
    forwards = []
    _count(monkeypatch, m, '_forward_one', forwards)
    video, lats = _call(pipe, prompts, solver, guidance=every_cond, nag=nag)
    assert pipe.last_guidance_plan == ['cond'] * STEPS and pipe.last_nag is nag and len(forwards) == STEPS       # ONE forward per step
    _same(lats, want)
    assert torch.equal(video, pipe.vae.decode([want[-1]])[0]) and torch.isfinite(video).all().item()
    assert not torch.equal(lats[0][1], lats0[0][1]) and not torch.equal(video, without)                         # the negative prompt acts
    # NAG's own negative prompt instead of the call's; the object's default is what generate(nag=None) uses
    own = NAG(4, 2.5, 0.5, n_prompt=prompts[2])
    want = _loop(pipe, solver, dev, lambda x, t: m([x], t=t, context=[prompts[0]], seq_len=SEQ, nag=(own, [prompts[2]]))[0])
    pipe.nag = own
    try:
        _same(_call(pipe, prompts, solver, guidance=every_cond)[1], want)
        assert pipe.last_nag is own
    finally:
        pipe.nag = None
    assert not torch.equal(want[-1], lats[-1][1])


@gpu
@pytest.mark.parametrize('solver', SOLVERS)
def test_guided_call_with_nag(dev, pipe, prompts, solver):
    from wan.backend import ops
    from wan.utils.nag import NAG
    m, nag = pipe.model, NAG(4, 2.5, 0.5, n_prompt=prompts[2])
    mixed = torch.empty(16, 2, 8, 8, device=dev)

    def predict(x, t):
        cond, uncond = m.forward_pair([x], t, [prompts[0]], [prompts[1]], SEQ, nag=(nag, [prompts[2]]))
        return ops.cfg_combine(mixed, uncond[0], cond[0], 5.0)
    want = _loop(pipe, solver, dev, predict)
    video, lats = _call(pipe, prompts, solver, nag=nag)
    assert pipe.last_guidance_plan is None and pipe.last_nag is nag
    _same(lats, want)
    assert not torch.equal(lats[0][1], _call(pipe, prompts, solver)[1][0][1])


@gpu
def test_inpaint_with_nag(dev, pipe, prompts):
    from wan.backend import ops
    from wan.utils.guidance import Guidance
    from wan.utils.nag import NAG
    m, nag = pipe.model, NAG(4, 2.5, 0.5)
    frames = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (7, 50, 70, 3)).astype(np.uint8))
    mask = torch.zeros(50, 70, dtype=torch.uint8)
    mask[:, :35] = 255
    clip = ops.video_from_u8(frames[:FRAMES].to(dev), SIZE[1], SIZE[0])
    z0, noise = pipe.vae.encode([clip])[0], W.randn((16, 2, 8, 8), 33).to(dev)
    lm = ops.mask_to_latent(ops.mask_from_u8(mask.view(1, 50, 70).to(dev), FRAMES, SIZE[1], SIZE[0], 0), (4, 8, 8))

    def renoise(i, latent, sched):
        s = sched.sigmas.tolist()[i + 1]
        ops.masked_renoise(latent, z0, noise, lm, 1.0 - s, s)
    want = _loop(pipe, 'unipc', dev, lambda x, t: m([x], t=t, context=[prompts[0]], seq_len=SEQ, nag=(nag, [prompts[1]]))[0], after=renoise)
    video, lats = _call(pipe, prompts, 'unipc', run=lambda p, **kw: pipe.inpaint(p, frames, mask=mask, **kw), guidance=Guidance(interval=(0.0, 0.0)),
                        nag=nag)
    _same(lats, want)
    assert torch.isfinite(video).all().item() and pipe.last_nag is nag


@gpu
def test_windows_with_nag(dev, pipe, prompts):
    from wan.backend import ops
    from wan.text2video import WindowRun
    from wan.utils.context_windows import ContextWindows
    from wan.utils.guidance import Guidance
    from wan.utils.nag import NAG
    m, nag, cw, lat = pipe.model, NAG(4, 2.5, 0.5), ContextWindows(frames=9, overlap=4), (16, 7, 8, 8)
    plan = cw.plan(lat[1])
    assert plan.starts == [0, 2, 4]
    run = WindowRun(plan, W.randn(lat, 33).to(dev), False, pipe.patch_size, pipe.sp_size)

    def predict(x, t):
        for k, f0 in enumerate(plan.starts):
            ops.window_gather(x, f0, run.lat)
            cond = m([run.lat], t=t, context=[prompts[0]], seq_len=run.seq_len, nag=(nag, [prompts[1]]))[0]
            ops.window_blend(run.cond, cond, f0, run.w[k], run.first[k])
        return run.cond
    want = _loop(pipe, 'unipc', dev, predict, lat=lat, steps=2)
    video, lats = _call(pipe, prompts, 'unipc', frames=25, lat=lat, steps=2, windows=cw, guidance=Guidance(interval=(0.0, 0.0)), nag=nag)
    assert pipe.last_window_plan == plan.starts
    _same(lats, want, steps=2)
    plain = _call(pipe, prompts, 'unipc', frames=25, lat=lat, steps=2, windows=cw, guidance=Guidance(interval=(0.0, 0.0)))[1]
    assert not torch.equal(plain[0][1], lats[0][1])


@gpu
def test_invalid_nag_raises_before_any_gpu_work(dev, pipe, prompts, monkeypatch):
    import wan
    from wan.utils.nag import NAG

    def no_gpu_work(*a, **kw):
        raise AssertionError('the prompt was encoded: the argument check came too late')
    monkeypatch.setattr(pipe, '_encode', no_gpu_work)
    for bad in (4.0, (4, 2.5, 0.25), 'nag', dict(scale=4)):
        with pytest.raises(ValueError, match='nag'):
            _call(pipe, prompts, 'unipc', nag=bad)
    with pytest.raises(ValueError, match='nag'):
        wan.WanT2V(pipe.config, '', device_id=0, model=pipe.model, vae=pipe.vae, nag=4.0)

    class Own(torch.nn.Module):             # a user's own model object: no `nag` keyword
        def forward(self, x, t, context, seq_len):
            raise AssertionError('a forward ran')
    monkeypatch.setattr(pipe, 'model', Own())
    with pytest.raises(ValueError, match='nag'):
        _call(pipe, prompts, 'unipc', nag=NAG(4))
