"""Step cache of WanT2V.generate: the plan (wan/utils/step_cache.py), the two kernels mg_step_resid_capture_f32 and
mg_resid_ln_modulate_f32, WanModel.step_cache('compute' | 'skip'), generate(step_cache=), the launcher flags and the calibration tool.

CPU: the plan rule against hand-worked sequences, the launcher flags, the declarations.
GPU: everything is either bit-equal to a composition of public ops / to the run without a step cache, or — the fp64 sums — held to
n x 2^-53 relative: all terms are non-negative, so every summation order of n terms is within that of the exact sum.
"""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

import weights as W
from abi_ref import header_declarations

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, S = True, False


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _launcher():
    spec = importlib.util.spec_from_file_location('mg_generate_sc', os.path.join(ROOT, 'scripts', 'inference', 'generate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tool():
    spec = importlib.util.spec_from_file_location('mg_step_cache_calibrate', os.path.join(ROOT, 'tools', 'step_cache_calibrate.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
def test_plan_from_distances_hand_worked():
    from wan.utils.step_cache import plan_from_distances as plan
    d = [9.0, 0.1, 0.2, 0.3, 0.1, 0.1, 0.4, 0.1]          # d[0] is never read
    assert plan(d, 0.0) == [C] * 8                                                # thresh 0: acc < 0 never holds
    assert plan(d, 1e30) == [C, S, S, S, S, S, S, C]                              # only step 0 and the last one
    assert plan(d, 1e30, keep_first=3, keep_last=2) == [C, C, C, S, S, S, C, C]
    assert plan(d, 1e30, keep_first=0, keep_last=0) == [C, S, S, S, S, S, S, S]   # step 0 is computed whatever keep_first says
    # the accumulator resets on a compute: 0.1, 0.3 (< 0.55), 0.6 -> C; 0.1, 0.2, 0.6 -> C; last kept
    assert plan(d, 0.55) == [C, S, S, C, S, S, C, C]
    # (without the reset steps 4 and 5 — 0.7, 0.8 — would compute as well.)  d_i is the distance to the PREVIOUS step also when that one
    # was skipped, so the distances of skipped steps add up: step 2 computes on d_1 + d_2 = 0.3 >= 0.25 although d_2 alone is 0.2
    assert plan(d, 0.25) == [C, S, C, C, S, S, C, C]
    # a non-identity polynomial, highest power first: p(d) = 10 d^2 + 1 -> 1.1, 1.4, 1.9, 1.1, 1.1, 2.6
    # 2.45: 1.1, 2.5|C, 1.9, 3.0|C, 1.1, 3.7|C     2.55: 1.1, 2.5, 4.4|C, 1.1, 2.2, 4.8|C
    assert plan(d, 2.45, coefficients=(10.0, 0.0, 1.0)) == [C, S, C, S, C, S, C, C]
    assert plan(d, 2.55, coefficients=(10.0, 0.0, 1.0)) == [C, S, S, C, S, S, C, C]
    # video-to-video: the loop starts at `first`, which takes step 0's place; the entries in front of it never run
    assert plan(d, 0.55, first=2) == [C, C, C, S, S, S, C, C]                     # acc from step 3 on: 0.3, 0.4, 0.5, 0.9|C
    assert plan(d, 1e30, first=5, keep_first=2) == [C, C, C, C, C, C, C, C]
    assert plan([], 0.5) == [] and plan([7.0], 0.5) == [C]
    for bad in (dict(thresh=-1.0), dict(thresh=float('nan')), dict(thresh=1.0, keep_first=-1), dict(thresh=1.0, coefficients=()),
                dict(thresh=1.0, first=8)):
        with pytest.raises(ValueError):
            plan(d, **bad)
    with pytest.raises(ValueError):
        plan([0.0, float('nan'), 0.1], 1.0)


def test_resolve_plan_explicit_and_v2v_start():
    from wan.utils.step_cache import resolve_plan
    ts = list(range(6))
    assert resolve_plan(None, None, ts) == (None, False)
    assert resolve_plan([C, S, C, S, C, C], None, ts) == ([C, S, C, S, C, C], False)
    assert resolve_plan([S, S, S, S, S, S], None, ts) == ([C, S, S, S, S, S], False)           # step 0 is forced
    assert resolve_plan([C, S, S, S, C, S], None, ts, i0=3) == ([C, S, S, C, C, S], False)       # v2v: the first step that runs is forced
    assert resolve_plan({'plan': [1, 0, 1, 0, 1, 1], 'stats': True}, None, ts) == ([C, S, C, S, C, C], True)
    with pytest.raises(ValueError, match='one entry per schedule index'):
        resolve_plan([C, S], None, ts)
    with pytest.raises(ValueError):
        resolve_plan({'keep_first': 2}, None, ts)
    with pytest.raises(ValueError):
        resolve_plan({'plan': [C] * 6, 'thresh': 0.1}, None, ts)
    for bad in (True, 'CS'):
        with pytest.raises(TypeError):
            resolve_plan(bad, None, ts)


def test_embedding_distances_fp64():
    from wan.utils.step_cache import embedding_distances
    e = np.array([[1.0, -3.0], [2.0, -1.0], [2.0, -1.0]], dtype=np.float32)
    assert embedding_distances(e).tolist() == [0.0, 3.0 / 4.0, 0.0]


def test_generate_parses_step_cache_flags():
    g = _launcher()
    a = g._parse_args(['--ckpt_dir', '/x'])
    assert a.step_cache is None and a.step_cache_spec is None
    a = g._parse_args(['--ckpt_dir', '/x', '--step_cache', '0.2'])
    assert a.step_cache_spec == {'thresh': 0.2}
    a = g._parse_args(['--ckpt_dir', '/x', '--step_cache', '0', '--step_cache_coefficients', '1e2,-3,0.5,1,-0.01', '--step_cache_keep', '2,3'])
    assert a.step_cache_spec == {'thresh': 0.0, 'coefficients': [100.0, -3.0, 0.5, 1.0, -0.01], 'keep_first': 2, 'keep_last': 3}
    with pytest.raises(AssertionError, match='need --step_cache'):
        g._parse_args(['--ckpt_dir', '/x', '--step_cache_keep', '1,1'])
    with pytest.raises(AssertionError, match='need --step_cache'):
        g._parse_args(['--ckpt_dir', '/x', '--step_cache_coefficients', '0,1'])
    with pytest.raises(AssertionError, match='>= 0'):
        g._parse_args(['--ckpt_dir', '/x', '--step_cache', '-0.1'])
    for bad in ('1,x', 'nan,1', ''):
        with pytest.raises(AssertionError, match='step_cache_coefficients'):
            g._parse_args(['--ckpt_dir', '/x', '--step_cache', '0.1', '--step_cache_coefficients=' + bad])
    for bad in ('1', '1,2,3', '-1,1', 'a,b'):
        with pytest.raises(AssertionError, match='step_cache_keep'):
            g._parse_args(['--ckpt_dir', '/x', '--step_cache', '0.1', '--step_cache_keep=' + bad])
    doc = g.__doc__
    assert '--step_cache THRESH' in doc and '--step_cache_coefficients' in doc and '--step_cache_keep' in doc


def test_declarations():
    """header and ctypes table agree on the new entries; generate and the constructor have the argument, default off."""
    from wan.backend import lib
    from wan.text2video import WanT2V
    decl = header_declarations()
    for name, n_args in (('mg_step_resid_capture_f32', 7), ('mg_resid_ln_modulate_f32', 12)):
        assert name in decl, name
        restype, want = decl[name]
        assert restype is lib.c_int and lib.SIGNATURES[name] == want and len(want) == n_args
    assert decl['mg_step_resid_partials_bytes'] == (lib.c_i64, [])
    assert lib.SIGNATURES['mg_step_resid_partials_bytes'] == [] and lib._RESTYPE['mg_step_resid_partials_bytes'] is lib.c_i64
    assert inspect.signature(WanT2V.generate).parameters['step_cache'].default is None
    assert inspect.signature(WanT2V.__init__).parameters['step_cache'].default is None


# ------------------------------------------------------------------------------------------------
# GPU: mg_step_resid_capture_f32
# ------------------------------------------------------------------------------------------------
def _capture_ref(x, xin, r_old):
    """(r_new fp32, (sum |r_new - r_old|, sum |r_old|)) — the differences in fp32, the sums in numpy fp64"""
    xn, xi, ro = (t.cpu().numpy() for t in (x, xin, r_old))
    rn = xn - xi
    assert rn.dtype == np.float32
    return rn, (np.abs(rn - ro).astype(np.float64).sum(), np.abs(ro).astype(np.float64).sum())


# 1, 3: tail only; 4: one vector, no tail; 4099: vectors + tail inside one workgroup's reach; 2^20 + 3: every one of the fixed grid's 1024
# workgroups (more than the device has CUs) has work and writes a non-zero partial; 5 x 2^20 + 1: lanes go round the unrolled loop twice
@gpu
@pytest.mark.parametrize('n', [1, 3, 4, 4099, 2 ** 20 + 3, 5 * 2 ** 20 + 1])
def test_step_resid_capture(dev, n):
    from wan.backend import ops
    g = torch.Generator(device='cpu').manual_seed(n)
    x, xin, r_old = (torch.randn(n, generator=g).to(dev) for _ in range(3))
    rn, (sd, so) = _capture_ref(x, xin, r_old)
    part = ops.step_resid_partials(dev)
    outs = []
    for _ in range(2):
        r, stats = r_old.clone(), torch.full((2,), float('nan'), dtype=torch.float64, device=dev)
        part.fill_(float('nan'))
        ops.step_resid_capture(r, x, xin, stats, part)
        assert np.array_equal(r.cpu().numpy(), rn) and torch.equal(r, x - xin)
        outs.append(stats.cpu().numpy().tobytes())
        got = stats.tolist()
        tol = n * 2.0 ** -53
        print(f'n={n}: stats {got} ref {(sd, so)} rel err {abs(got[0] - sd) / sd:.2e} {abs(got[1] - so) / so:.2e} tol {tol:.2e}')
        assert abs(got[0] - sd) <= tol * sd and abs(got[1] - so) <= tol * so
    assert outs[0] == outs[1] and len(outs[0]) == 16                      # the same inputs give the same 16 bytes
    # stats=None: no reduction, partials untouched, r the same
    r = r_old.clone()
    part.fill_(-7.0)
    ops.step_resid_capture(r, x, xin)
    assert np.array_equal(r.cpu().numpy(), rn) and bool((part == -7.0).all())


@gpu
def test_step_resid_capture_rejects(dev):
    from wan.backend import lib, ops
    n = 4099
    buf = [torch.ones(n + 4, device=dev) for _ in range(3)]
    stats, part = torch.zeros(2, dtype=torch.float64, device=dev), ops.step_resid_partials(dev)
    assert part.numel() * 8 == lib.load().mg_step_resid_partials_bytes() > 0
    # the contract is 16-byte aligned r, x, xin: a 4-byte-aligned offset is refused, whichever pointer carries it
    for k in range(3):
        args = [b[1:1 + n] if i == k else b[:n] for i, b in enumerate(buf)]
        assert args[k].data_ptr() % 16 == 4
        with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
            ops.step_resid_capture(*args, stats, part)
    with pytest.raises(lib.MoviigenHipError):                                      # empty tensors (their data pointers are NULL)
        ops.step_resid_capture(buf[0][:0], buf[1][:0], buf[2][:0])
    h = lib.load()
    P = lambda t: t.data_ptr()      # noqa: E731
    assert h.mg_step_resid_capture_f32(P(buf[0]), P(buf[1]), P(buf[2]), 0, None, None, None) == -2          # n < 1
    assert h.mg_step_resid_capture_f32(None, P(buf[1]), P(buf[2]), n, None, None, None) == -1
    assert h.mg_step_resid_capture_f32(P(buf[0]), None, P(buf[2]), n, None, None, None) == -1
    assert h.mg_step_resid_capture_f32(P(buf[0]), P(buf[1]), None, n, None, None, None) == -1
    assert h.mg_step_resid_capture_f32(P(buf[0]), P(buf[1]), P(buf[2]), n, P(stats), None, None) == -1      # stats without partials
    assert h.mg_step_resid_capture_f32(P(buf[0]), P(buf[1]), P(buf[2]), n, P(stats) + 4, P(part), None) == -2
    assert h.mg_step_resid_capture_f32(P(buf[0]), P(buf[1]), P(buf[2]), -5, None, None, None) == -2
    torch.cuda.synchronize()
    assert bool((buf[0] == 1).all())                                            # nothing ran: r would be x - xin = 0


# ------------------------------------------------------------------------------------------------
# GPU: mg_resid_ln_modulate_f32
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('dim', [128, 132, 5120, 8192])      # one kernel instantiation each for <= 2048, <= 5120, <= 8192 + a row that is no multiple of 128
@pytest.mark.parametrize('rows', [1, 5, 67])
def test_resid_ln_modulate_bit_equal(dev, rows, dim):
    from wan.backend import ops
    pad = 12 if rows == 5 else 0                                  # rows == 5: ldx > dim, and ldr, ldo differ from it
    xb = W.randn((rows, dim + pad), rows + dim).to(dev)
    rb = (W.randn((rows, dim + 2 * pad), rows + dim + 1) * 0.3).to(dev)
    ob = torch.full((rows, dim + pad // 3), float('nan'), device=dev)
    x, r, out = xb[:, :dim], rb[:, :dim], ob[:, :dim]
    scale, shift = W.randn((dim,), 5).to(dev) * 0.1, W.randn((dim,), 6).to(dev)
    x_before = xb.clone()
    ops.resid_ln_modulate(x, r, scale, shift, 1e-6, out)
    s = ops.lincomb(torch.empty(rows, dim, device=dev), [(x.contiguous(), 1.0), (r.contiguous(), 1.0)])
    assert torch.equal(s, x + r)
    ref = ops.ln_modulate(s, scale, shift, True, 1e-6, torch.empty(rows, dim, device=dev))
    assert torch.equal(out, ref)
    assert torch.equal(xb, x_before)
    if pad:
        assert bool(torch.isnan(ob[:, dim:]).all())               # nothing behind the row is written


@gpu
def test_resid_ln_modulate_rejects(dev):
    from wan.backend import lib, ops
    for dim in (8196, 130):
        x, r, out = (torch.zeros(2, dim, device=dev) for _ in range(3))
        with pytest.raises(lib.MoviigenHipError, match='MG_ERR_SHAPE'):
            ops.resid_ln_modulate(x, r, None, None, 1e-6, out)
    x, r, out = (torch.zeros(2, 128, device=dev) for _ in range(3))
    with pytest.raises(lib.MoviigenHipError):
        ops.resid_ln_modulate(x, r[:1], None, None, 1e-6, out)
    h = lib.load()
    assert h.mg_resid_ln_modulate_f32(x.data_ptr(), 128, None, 128, 2, 128, None, None, 1e-6, out.data_ptr(), 128, None) == -1
    assert h.mg_resid_ln_modulate_f32(x.data_ptr(), 128, r.data_ptr() + 4, 128, 1, 128, None, None, 1e-6, out.data_ptr(), 128, None) == -2
    assert h.mg_resid_ln_modulate_f32(x.data_ptr(), 64, r.data_ptr(), 128, 2, 128, None, None, 1e-6, out.data_ptr(), 128, None) == -2


# ------------------------------------------------------------------------------------------------
# GPU: WanModel.step_cache
# ------------------------------------------------------------------------------------------------
CFG = W.TINY_DIT
LAT, SEQ = (16, 2, 8, 12), 48            # 2 x 4 x 6 = 48 tokens


def _model(dev, seed=0):
    import wan
    m = wan.modules.WanModel(**CFG)
    m.load_state_dict(W.make_dit_params(CFG, seed))
    return m.to(dev)


@pytest.fixture(scope='module')
def model(dev):
    return _model(dev)


def _ws(m):
    (ws,) = m._ws.values()
    return ws


def _skip_composition(m, lat, t, r, dev):
    """a skipped forward from public ops: patchify -> gemm -> lincomb(x, r) -> ln_modulate -> head_gemm -> unpatchify"""
    from wan.backend import ops
    d, (_, F, H, Wd) = m.dim, lat.shape
    L = F * (H // 2) * (Wd // 2)
    tok = torch.empty(L, CFG['in_dim'] * 4, dtype=torch.bfloat16, device=dev)
    ops.patchify(lat, 2, 2, tok)
    x = torch.empty(L, d, device=dev)
    ops.gemm(tok, m.patch_embedding.weight.data.reshape(d, -1), m.patch_embedding.bias, ops.BIAS_F32, x)
    e, _ = m.time_embeddings(t)
    hmod = ops.add_rows(m.head.modulation.data.reshape(2, d), e.reshape(1, d), torch.empty(2, d, device=dev), 1)
    s = ops.lincomb(torch.empty_like(x), [(x, 1.0), (r, 1.0)])
    hf = ops.ln_modulate(s, hmod[1], hmod[0], True, m.eps, torch.empty_like(x))
    y = ops.head_gemm(hf, m.head.head.weight, m.head.head.bias, torch.empty(L, 4 * CFG['out_dim'], device=dev))
    return ops.unpatchify(y, CFG['out_dim'], F, H // 2, Wd // 2, 2, 2, torch.empty(CFG['out_dim'], F, H, Wd, device=dev))


@gpu
def test_model_compute_mode_is_bit_identical_and_skip_is_the_composition(dev, model, monkeypatch):
    from wan.backend import ops
    m = model
    c1, c2 = W.randn((9, CFG['text_dim']), 30).to(dev), W.randn((5, CFG['text_dim']), 31).to(dev)
    lat1, t1 = W.randn(LAT, 20).to(dev), torch.tensor([700], device=dev)
    lat2, t2 = W.randn(LAT, 21).to(dev), torch.tensor([640], device=dev)
    # (a) 'compute' changes no output bit: forward and forward_pair
    a = m([lat1], t=t1, context=[c1], seq_len=SEQ)[0].clone()
    pa, pb = (v[0].clone() for v in m.forward_pair([lat1], t1, [c1], [c2], SEQ))
    assert torch.equal(pa, a)
    with m.step_cache('compute'):
        assert torch.equal(m([lat1], t=t1, context=[c1], seq_len=SEQ)[0], a)
        ws = _ws(m)
        r1_single = (ws['x'] - ws['xin']).clone()                  # the stream behind the last block - behind the patch embedding
        assert torch.equal(ws['resid'][m._ctx_key(c1)][1], r1_single)
        qa, qb = m.forward_pair([lat1], t1, [c1], [c2], SEQ)
        assert torch.equal(qa[0], pa) and torch.equal(qb[0], pb)
        r2 = (ws['x'] - ws['xin']).clone()                          # the 'reuse' half ran last: the second context's stream
    r1 = ws['resid'][m._ctx_key(c1)][1].clone()
    assert torch.equal(r1, r1_single) and torch.equal(ws['resid'][m._ctx_key(c2)][1], r2) and not torch.equal(r1, r2)
    assert m._step_mode is None
    # (b) 'skip' at another latent and t = the composition of public ops, both branches; (d) only the patch-embedding GEMM runs
    want1, want2 = _skip_composition(m, lat2, t2, r1, dev), _skip_composition(m, lat2, t2, r2, dev)
    calls = []
    orig = ops.gemm

    def counting(a_, w, *args, **kw):
        calls.append(tuple(w.shape))
        return orig(a_, w, *args, **kw)
    monkeypatch.setattr(ops, 'gemm', counting)
    with m.step_cache('skip'):
        s1 = m([lat2], t=t2, context=[c1], seq_len=SEQ)[0].clone()
        assert calls == [(CFG['dim'], CFG['in_dim'] * 4)]
        del calls[:]
        sa, sb = m.forward_pair([lat2], t2, [c1], [c2], SEQ)
        assert calls == [(CFG['dim'], CFG['in_dim'] * 4)]              # the pair embeds once
    monkeypatch.setattr(ops, 'gemm', orig)
    assert torch.equal(s1, want1) and torch.equal(sa[0], want1) and torch.equal(sb[0], want2)
    assert not torch.equal(want1, want2)
    # the skip left the residuals and the weights' caches alone: the computed forward still gives its bits
    assert torch.equal(ws['resid'][m._ctx_key(c1)][1], r1)
    assert torch.equal(m([lat1], t=t1, context=[c1], seq_len=SEQ)[0], a)
    # stats=True: the sums of the capture, against the residuals (zeros before the first capture of a context)
    m.drop_step_cache()
    assert 'resid' not in ws and 'xin' not in ws
    with m.step_cache('compute', stats=True):
        m([lat1], t=t1, context=[c1], seq_len=SEQ)
        sd, so = m.step_cache_stats[m._ctx_key(c1)]
        n = r1.numel()
        ref = r1.abs().double().sum().item()
        assert so == 0.0 and abs(sd - ref) <= n * 2.0 ** -53 * ref
        m([lat2], t=t2, context=[c1], seq_len=SEQ)
        sd, so = m.step_cache_stats[m._ctx_key(c1)]
        r_new = ws['resid'][m._ctx_key(c1)][1]
        ref_d = (r_new - r1).abs().double().sum().item()
        assert abs(so - ref) <= n * 2.0 ** -53 * ref and abs(sd - ref_d) <= n * 2.0 ** -53 * ref_d
    m.drop_step_cache()


@gpu
def test_model_skip_needs_a_residual(dev):
    m = _model(dev, seed=1)
    c1, c2 = W.randn((9, CFG['text_dim']), 30).to(dev), W.randn((5, CFG['text_dim']), 31).to(dev)
    lat, t = W.randn(LAT, 20).to(dev), torch.tensor([700], device=dev)
    with pytest.raises(ValueError):
        with m.step_cache('cache'):
            pass
    with m.step_cache('skip'):
        with pytest.raises(RuntimeError, match='no residual'):                 # nothing computed yet
            m([lat], t=t, context=[c1], seq_len=SEQ)
    with m.step_cache('compute'):
        m([lat], t=t, context=[c1], seq_len=SEQ)
    with m.step_cache('skip'):
        m([lat], t=t, context=[c1], seq_len=SEQ)
        with pytest.raises(RuntimeError, match='no residual'):                 # another context
            m([lat], t=t, context=[c2], seq_len=SEQ)
        with pytest.raises(RuntimeError, match='no residual'):                 # another sequence length: another workspace
            m([W.randn((16, 2, 8, 8), 22).to(dev)], t=t, context=[c1], seq_len=32)
    with m.step_cache('compute'):
        m([lat], t=t, context=[c1], seq_len=SEQ)
    d = CFG['dim']
    m.load_lora({'diffusion_model.blocks.0.self_attn.q.lora_A.weight': W.randn((4, d), 40) * 0.1,
                 'diffusion_model.blocks.0.self_attn.q.lora_B.weight': W.randn((d, 4), 41) * 0.1})
    with m.step_cache('skip'):
        with pytest.raises(RuntimeError, match='no residual'):                 # other weights: the residual is gone
            m([lat], t=t, context=[c1], seq_len=SEQ)
    with m.step_cache('compute'):
        m([lat], t=t, context=[c1], seq_len=SEQ)
    m.unload_lora()
    with m.step_cache('skip'):
        with pytest.raises(RuntimeError, match='no residual'):
            m([lat], t=t, context=[c1], seq_len=SEQ)
    with m.step_cache('compute'):
        m([lat], t=t, context=[c1], seq_len=SEQ)
    m.set_gemm_precision('bf16')                                               # no change of precision: kept
    with m.step_cache('skip'):
        m([lat], t=t, context=[c1], seq_len=SEQ)


# ------------------------------------------------------------------------------------------------
# GPU: the plan from the model's time embedding
# ------------------------------------------------------------------------------------------------
def _time_embedding_f64(m, timesteps):
    """(e, e0) of reference model.py:541-545 in fp64 torch on the host"""
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items() if k.startswith('time_')}
    half = m.freq_dim // 2
    pos = timesteps.double().cpu().reshape(-1, 1)
    ang = pos * torch.pow(10000.0, -torch.arange(half, dtype=torch.float64) / half).reshape(1, -1)
    s = torch.cat([torch.cos(ang), torch.sin(ang)], 1)
    h = torch.nn.functional.silu(s @ sd['time_embedding.0.weight'].T + sd['time_embedding.0.bias'])
    e = h @ sd['time_embedding.2.weight'].T + sd['time_embedding.2.bias']
    e0 = torch.nn.functional.silu(e) @ sd['time_projection.1.weight'].T + sd['time_projection.1.bias']
    return e.numpy(), e0.numpy()


@gpu
@pytest.mark.parametrize('source', ['e0', 'e'])
def test_step_cache_plan_vs_fp64_reference(dev, model, source):
    from test_v2v import _scheduler
    from wan.utils.step_cache import embedding_distances, plan_from_distances, step_cache_plan, step_distances
    _, ts = _scheduler('unipc', 12, 5.0, device=dev)
    e, e0 = _time_embedding_f64(model, ts)
    d_ref = embedding_distances(e0 if source == 'e0' else e)
    d = step_distances(model, ts, source)
    print(f'{source}: distances max rel err vs fp64 {np.abs(d[1:] / d_ref[1:] - 1).max():.2e}')
    # fp32 kernels against fp64: ~2^-24 per operation over dot products of <= 128 terms, on distances >= 1e-2 of the embedding's scale;
    # a plan decision moves only when this reaches the 1e-3 margin the thresholds below keep
    assert np.abs(d[1:] / d_ref[1:] - 1).max() < 1e-4
    coef = (0.0, 0.0, 0.5, 1.0, 0.0)                               # p(d) = d + d^2 / 2
    p = np.polyval(coef, d_ref)
    # thresholds between consecutive values of the reference accumulator, so that no decision sits within 1e-3 relative of one
    for thresh in (0.5 * (p[1] + p[1] + p[2]), 0.5 * (p[1] + p[2] + p[1] + p[2] + p[3]), 0.5 * p[1:].min(), 2.0 * p.sum()):
        want, acc, accs = [], 0.0, []
        for i in range(12):
            if i == 0 or i == 11:
                want.append(True)
                acc = 0.0
                continue
            acc += p[i]
            accs.append(acc)
            want.append(not acc < thresh)
            if want[-1]:
                acc = 0.0
        assert all(abs(a / thresh - 1) > 1e-3 for a in accs), (thresh, accs)
        assert plan_from_distances(d_ref, thresh, coef) == want
        got = step_cache_plan(model, ts, thresh, coefficients=coef, source=source)
        print(f'{source} thresh {thresh:.4f}: ' + ''.join('C' if c else 's' for c in got))
        assert got == want
    with pytest.raises(ValueError):
        step_cache_plan(model, ts, 0.1, source='x')


# ------------------------------------------------------------------------------------------------
# GPU: WanT2V.generate(step_cache=) and the calibration tool
# ------------------------------------------------------------------------------------------------
SIZE, FRAMES, STEPS = (64, 64), 5, 6
PLAN = [C, S, C, S, C, C]


@pytest.fixture(scope='module')
def pipe(dev):
    import wan
    from test_v2v import _vae_params
    from wan.configs import Config
    vae = wan.modules.WanVAE(state_dict=_vae_params(8), device=dev)
    conf = Config(num_train_timesteps=1000, param_dtype=torch.bfloat16, vae_stride=(4, 8, 8), patch_size=(1, 2, 2), sample_neg_prompt='',
                  vae_checkpoint='', text_len=CFG['text_len'])
    return wan.WanT2V(conf, '', device_id=0, model=_model(dev), vae=vae)


@pytest.fixture(scope='module')
def prompts(dev):
    return W.randn((9, CFG['text_dim']), 31).to(dev), W.randn((5, CFG['text_dim']), 32).to(dev)


def _call(pipe, prompts, solver, **kw):
    lats = []
    kw.setdefault('callback', lambda i, l: lats.append((i, l.clone())))
    video = pipe.generate(prompts[0], size=SIZE, frame_num=FRAMES, shift=5.0, sample_solver=solver, sampling_steps=STEPS, guide_scale=5.0,
                          n_prompt=prompts[1], seed=0, offload_model=False, noise=W.randn((16, 2, 8, 8), 33), **kw)
    return video, lats


@pytest.fixture(scope='module')
def plain(pipe, prompts):
    """the run without a step cache, once per solver, shared"""
    return {s: _call(pipe, prompts, s) for s in ('unipc', 'dpm++')}


@gpu
@pytest.mark.parametrize('solver', ['unipc', 'dpm++'])
def test_generate_all_compute_is_bit_identical(dev, pipe, prompts, plain, solver):
    video, lats = plain[solver]
    for spec in (0.0, [C] * STEPS, {'thresh': 0.0, 'source': 'e'}):
        v, l = _call(pipe, prompts, solver, step_cache=spec)
        assert pipe.last_step_plan == [C] * STEPS
        assert torch.equal(v, video) and all(torch.equal(a[1], b[1]) for a, b in zip(l, lats))
    _call(pipe, prompts, solver)
    assert pipe.last_step_plan is None
    assert all('resid' not in ws and 'xin' not in ws for ws in pipe.model._ws.values())      # dropped when the loop ends


@gpu
@pytest.mark.parametrize('solver', ['unipc', 'dpm++'])
def test_generate_plan_equals_hand_written_loop(dev, pipe, prompts, plain, solver):
    from test_v2v import _scheduler
    from wan.backend import ops
    video, lats = _call(pipe, prompts, solver, step_cache=PLAN)
    assert pipe.last_step_plan == PLAN and [i for i, _ in lats] == list(range(STEPS))
    assert not torch.equal(lats[-1][1], plain[solver][1][-1][1])                  # the skipped steps did something else
    assert torch.equal(lats[0][1], plain[solver][1][0][1])                        # step 0 is computed either way
    # the same loop from forward_pair, the mode scope, cfg_combine and the scheduler
    m = pipe.model
    sched, ts = _scheduler(solver, STEPS, 5.0, device=dev)
    latent = W.randn((16, 2, 8, 8), 33).to(dev)
    pred = torch.empty_like(latent)
    ctx, ctx_null = [prompts[0]], [prompts[1]]
    for i, t_host in enumerate(ts.tolist()):
        with m.step_cache('compute' if PLAN[i] else 'skip'):
            cond, uncond = m.forward_pair([latent], ts[i:i + 1], ctx, ctx_null, 32)
        ops.cfg_combine(pred, uncond[0], cond[0], 5.0)
        latent = sched.step(pred.unsqueeze(0), t_host, latent.unsqueeze(0), return_dict=False)[0].squeeze(0)
        assert torch.equal(latent, lats[i][1]), i
    m.drop_step_cache()
    assert torch.equal(video, pipe.vae.decode([latent])[0])
    # the object's default is what generate(step_cache=None) uses
    pipe.step_cache = PLAN
    try:
        v2, _ = _call(pipe, prompts, solver)
        assert torch.equal(v2, video) and pipe.last_step_plan == PLAN
    finally:
        pipe.step_cache = None


@gpu
def test_generate_v2v_first_executed_step_is_computed(dev, pipe, prompts, monkeypatch):
    from test_v2v import _frames
    frames = _frames(FRAMES, 50, 70, 5)
    modes = []
    inner = pipe.model.step_cache

    def spy(mode, stats=False):
        modes.append(mode)
        return inner(mode, stats=stats)
    monkeypatch.setattr(pipe.model, 'step_cache', spy)
    plan = [C, S, C, S, C, S]                                                     # strength 0.5: steps 3, 4, 5 run, and 3 says skip
    video, lats = _call(pipe, prompts, 'unipc', step_cache=plan, init_video=frames, strength=0.5)
    assert [i for i, _ in lats] == [3, 4, 5]
    assert pipe.last_step_plan == [C, S, C, C, C, S]
    assert modes == ['compute', 'skip']          # 3: forced, keeps no residual (4 computes); 4: computed, kept for 5; 5: skipped
    assert torch.isfinite(video).all().item()
    ref, _ = _call(pipe, prompts, 'unipc', step_cache=[C, C, C, C, C, S], init_video=frames, strength=0.5)
    assert torch.equal(video, ref)


@gpu
def test_calibration_tool(dev, pipe, prompts):
    tool = _tool()
    m = pipe.model
    saved = []

    def keep(i, latent):
        (ws,) = m._ws.values()
        saved.append({k: r.clone() for k, (_, r) in ws['resid'].items()})
    out = tool.calibrate(pipe, prompts[0], callback=keep, size=SIZE, frame_num=FRAMES, shift=5.0, sample_solver='unipc', sampling_steps=STEPS,
                         guide_scale=5.0, n_prompt=prompts[1], seed=0, offload_model=False, noise=W.randn((16, 2, 8, 8), 33))
    assert len(out['coefficients']) == 5 and all(np.isfinite(c) for c in out['coefficients'])
    assert out['steps'] == [1, 2, 3, 4, 5] and len(out['pairs']) == 5 and len(saved) == STEPS and all(len(s) == 2 for s in saved)
    from wan.utils.step_cache import step_distances
    d = step_distances(m, pipe.last_step_timesteps, 'e0')
    n = sum(v.numel() for v in saved[0].values())
    tol = n * 2.0 ** -53
    for (dist, o), (sd, so), i in zip(out['pairs'], out['sums'], out['steps']):
        ref_d = sum((saved[i][k] - saved[i - 1][k]).abs().double().sum().item() for k in saved[i])
        ref_o = sum(saved[i - 1][k].abs().double().sum().item() for k in saved[i])
        print(f'step {i}: d {dist:.4e} o {o:.4e}  sums rel err {abs(sd / ref_d - 1):.1e} {abs(so / ref_o - 1):.1e} (tol {tol:.1e})')
        assert dist == d[i]
        assert abs(sd - ref_d) <= tol * ref_d and abs(so - ref_o) <= tol * ref_o
        assert abs(o - ref_d / ref_o) <= 2 * tol * (ref_d / ref_o) + 2.0 ** -52 * o      # a quotient of two such sums
    assert pipe.last_step_plan == [C] * STEPS
