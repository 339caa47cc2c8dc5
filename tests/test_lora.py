"""LoRA adapters for the DiT: the adapter-file reader (wan/utils/lora.py), the merge kernel mg_lora_merge (csrc/lora_merge.hip) through
ops.lora_merge, and WanModel.load_lora / unload_lora / WanT2V(lora=).

The kernel's bound, per element, against ref = w + up @ down in fp64:
    |got - ref| <= h(ref) + (R + 2) 2^-24 (|w| + sum_j |up_nj down_jk|)
h(ref) = half the bf16 spacing at |ref| for bf16 storage, 0 for fp32 storage: an fp32 sum of R + 1 terms (each product rounded once,
each addition once: R + 1 roundings of relative size 2^-24 on partial sums no larger than the sum of magnitudes, to first order; R + 2
leaves the second-order terms room) and ONE correct rounding to the storage type.  Merging in two roundings exceeds it.
"""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weights as W  # noqa: E402
from abi_ref import header_declarations  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
CFG = W.SMALL_DIT_HD128                           # head_dim 128, dim 256, ffn_dim 512, 2 layers


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _randn(shape, seed, std):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * std


def half_spacing_bf16(ref):
    """half the distance between neighbouring bf16 values at |ref| (fp64 tensor)"""
    e = torch.frexp(ref.abs())[1] - 1             # floor(log2 |ref|); frexp(0) gives exponent 0
    e = torch.where(ref == 0, torch.full_like(e, -126), e).clamp_min(-126)
    return torch.ldexp(torch.ones_like(ref), e - 8)


def merge_bound(w, up, down, ref):
    mag = w.double().abs() + up.double().abs() @ down.double().abs()
    h = half_spacing_bf16(ref) if w.dtype == torch.bfloat16 else 0.0
    return h + (up.shape[1] + 2) * 2.0 ** -24 * mag


def check_merge(got, w, up, down, tag):
    """got: the merged weights (CPU); w, up, down: what went in (CPU).  Prints the figures, then asserts the bound."""
    ref = w.double() + up.double() @ down.double()
    err = (got.double() - ref).abs()
    bound = merge_bound(w, up, down, ref)
    off = f', share != bf16_rne(ref) {(got != ref.float().bfloat16()).double().mean().item():.2e}' if w.dtype == torch.bfloat16 else ''
    print(f'{tag}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}{off}')
    assert torch.isfinite(got.double()).all()
    assert (err <= bound).all(), (tag, int((err > bound).sum()))


# ------------------------------------------------------------------------------------------------
# CPU: declarations
# ------------------------------------------------------------------------------------------------
def test_declarations():
    """header and ctypes table agree on mg_lora_merge; WanT2V and the launcher have the new surface."""
    from wan.backend import lib
    from wan.text2video import WanT2V
    decl = header_declarations()
    assert 'mg_lora_merge' in decl, 'include/moviigen_hip.h does not declare mg_lora_merge'
    restype, want = decl['mg_lora_merge']
    assert restype is lib.c_int and lib.SIGNATURES['mg_lora_merge'] == want
    assert len(want) == 11
    par = inspect.signature(WanT2V.__init__).parameters
    assert list(par)[-2:] == ['lora', 'lora_strength']           # appended: every positional call keeps its meaning
    assert par['lora'].default is None and par['lora_strength'].default == 1.0
    src = open(os.path.join(ROOT, 'scripts', 'inference', 'generate.py')).read()
    assert "'--lora'" in src


def test_generate_parses_lora_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location('mg_generate', os.path.join(ROOT, 'scripts', 'inference', 'generate.py'))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    a = g._parse_args(['--ckpt_dir', '/x', '--lora', 'a.safetensors:0.5', '--lora', 'b.safetensors'])
    assert a.lora == [('a.safetensors', 0.5), ('b.safetensors', 1.0)]
    assert g._parse_args(['--ckpt_dir', '/x']).lora == []
    assert g._lora_arg('dir:x/c.safetensors') == ('dir:x/c.safetensors', 1.0)
    assert g._lora_arg('c.safetensors:-1.25') == ('c.safetensors', -1.25)


# ------------------------------------------------------------------------------------------------
# CPU: adapter files
# ------------------------------------------------------------------------------------------------
READ_TARGETS = ('blocks.1.cross_attn.k', 'blocks.0.ffn.2', 'text_embedding.0')


@pytest.fixture(scope='module')
def shapes():
    import wan
    return {n: tuple(w.shape) for n, w in wan.modules.WanModel(**CFG).lora_targets().items()}


def _factors(shapes, names, rank, seed, std=0.05):
    """{name: (up [N, r], down [r, K])} fp32"""
    return {n: (_randn((shapes[n][0], rank), seed + 2 * i, std), _randn((rank, shapes[n][1]), seed + 2 * i + 1, std))
            for i, n in enumerate(names)}


def _spell(factors, style, alpha=None, no_alpha=()):
    """the adapter as a dict of tensors in one of the three spellings; alpha (a float) is stored for every module not in no_alpha"""
    out = {}
    for n, (up, down) in factors.items():
        if style == 'peft':
            m, d, u = 'diffusion_model.' + n, '.lora_A.weight', '.lora_B.weight'
        elif style == 'kohya':
            m, d, u = 'model.diffusion_model.' + n, '.lora_down.weight', '.lora_up.weight'
        else:
            m, d, u = 'lora_unet_' + n.replace('.', '_'), '.lora_down.weight', '.lora_up.weight'
        out[m + d], out[m + u] = down.clone(), up.clone()
        if alpha is not None and n not in no_alpha:
            out[m + '.alpha'] = torch.tensor(float(alpha))
    return out


def test_read_lora_three_spellings(shapes, tmp_path):
    from safetensors.torch import save_file
    from wan.utils.lora import read_lora
    fac = _factors(shapes, READ_TARGETS, 4, 100)
    got = {}
    for style in ('peft', 'kohya', 'flat'):
        path = str(tmp_path / f'{style}.safetensors')
        save_file(_spell(fac, style, alpha=2.0, no_alpha=('text_embedding.0',)), path)
        got[style] = read_lora(path, shapes)
    for style, g in got.items():
        assert set(g) == set(READ_TARGETS), (style, sorted(g))
        for n in READ_TARGETS:
            up, down, alpha = g[n]
            assert up.dtype == down.dtype == torch.float32
            assert torch.equal(up, fac[n][0]) and torch.equal(down, fac[n][1]), (style, n)
            assert alpha == (None if n == 'text_embedding.0' else 2.0), (style, n, alpha)
    # a dict is read like a file; fp16 / bf16 factors are widened; names alone (no shapes) are enough to resolve the targets
    half = {k: (v.half() if v.dim() == 2 else v) for k, v in _spell(fac, 'flat').items()}
    g = read_lora(half, list(shapes))
    assert all(torch.equal(g[n][0], fac[n][0].half().float()) and g[n][2] is None for n in READ_TARGETS)


def test_read_lora_refusals(shapes):
    from wan.utils.lora import read_lora
    fac = _factors(shapes, READ_TARGETS[:1], 4, 200)
    good = _spell(fac, 'kohya')
    assert set(read_lora(good, shapes)) == {READ_TARGETS[0]}
    diff_b = {**good, 'diffusion_model.blocks.0.ffn.2.diff_b': torch.zeros(256)}
    unknown = {**good, 'diffusion_model.blocks.7.self_attn.q.lora_down.weight': torch.zeros(4, 256),
               'diffusion_model.blocks.7.self_attn.q.lora_up.weight': torch.zeros(256, 4)}
    conv = {**good, 'diffusion_model.patch_embedding.lora_down.weight': torch.zeros(4, 64),
            'diffusion_model.patch_embedding.lora_up.weight': torch.zeros(256, 4)}
    for bad in (diff_b, unknown, conv):
        with pytest.raises(ValueError):
            read_lora(bad, shapes)
        assert set(read_lora(bad, shapes, strict=False)) == {READ_TARGETS[0]}
    dora = {**good, 'model.diffusion_model.blocks.1.cross_attn.k.dora_scale': torch.ones(256)}
    wrong = dict(good)
    wrong['model.diffusion_model.blocks.1.cross_attn.k.lora_down.weight'] = torch.zeros(4, 264)
    rank = dict(good)
    rank['model.diffusion_model.blocks.1.cross_attn.k.lora_up.weight'] = torch.zeros(256, 5)
    for bad in (dora, wrong, rank):
        for strict in (True, False):
            with pytest.raises(ValueError):
                read_lora(bad, shapes, strict=strict)


# ------------------------------------------------------------------------------------------------
# GPU: the kernel through ops.lora_merge
# ------------------------------------------------------------------------------------------------
def _random_operands(N, K, R, seed, dtype=torch.bfloat16):
    return _randn((N, K), seed, 0.02).to(dtype), _randn((N, R), seed + 1, 0.05), _randn((R, K), seed + 2, 0.05)


# the kernel's tile is 64 x 256 and its rank chunk 32: a single tile, tiles with edges in both dimensions, R below / across / several
# chunks (odd R: half a rank pair), and two matrices of the 14B model
@gpu
@pytest.mark.parametrize('N,K,R', [(64, 64, 16), (1, 8, 2), (200, 264, 1), (130, 72, 3), (257, 1032, 130), (5120, 5120, 128),
                                   (13824, 5120, 32)])
def test_merge_random_bf16(dev, N, K, R):
    from wan.backend import ops
    w, up, down = _random_operands(N, K, R, 1000 + N + K + R)
    wd = w.to(dev)
    assert ops.lora_merge(wd, up.to(dev), down.to(dev)) is wd
    check_merge(wd.cpu(), w, up, down, f'bf16 ({N}, {K}, {R})')


@gpu
def test_merge_random_fp32_storage(dev):
    from wan.backend import ops
    w, up, down = _random_operands(96, 256, 8, 77, torch.float32)
    wd = w.to(dev)
    ops.lora_merge(wd, up.to(dev), down.to(dev))
    check_merge(wd.cpu(), w, up, down, 'fp32 (96, 256, 8)')


@gpu
def test_merge_two_adapters_one_rounding(dev):
    """ranks 16 and 48 with scales 0.75 and -1.3 folded into `up` in fp32 and concatenated: one merge, one rounding.  The same update
    applied adapter by adapter, each rounded to bf16, does NOT satisfy the bound (checked on the CPU: the test tells the two apart)."""
    from wan.backend import ops
    N, K = 192, 320
    w = _randn((N, K), 1, 0.02).bfloat16()
    u1, d1, u2, d2 = _randn((N, 16), 2, 0.05), _randn((16, K), 3, 0.05), _randn((N, 48), 4, 0.05), _randn((48, K), 5, 0.05)
    up = torch.cat([u1 * torch.tensor(0.75), u2 * torch.tensor(-1.3)], 1)      # fp32 products, as the caller folds them
    down = torch.cat([d1, d2], 0)
    wd = w.to(dev)
    ops.lora_merge(wd, up.to(dev), down.to(dev))
    check_merge(wd.cpu(), w, up, down, 'two adapters, one merge')
    step = (w.double() + up[:, :16].double() @ d1.double()).bfloat16()
    step = (step.double() + up[:, 16:].double() @ d2.double()).bfloat16()
    ref = w.double() + up.double() @ down.double()
    over = ((step.double() - ref).abs() > merge_bound(w, up, down, ref)).double().mean().item()
    print(f'two roundings (CPU): share of elements outside the bound {over:.3f}')
    assert over > 0.05


def _exact_operands(N, K, R, seed, dtype=torch.bfloat16):
    """w = integers / 32 in [-0.5, 0.5], up = integers / 2 in [-1, 1], down = integers / 16 in [-1/8, 1/8]: every product is a multiple of
    1/32 of at most 1/8, so for R <= 56 every partial sum is a multiple of 1/32 below 8 — exact in fp32 in any order and representable in
    bf16 (8 significant bits).  Random, so a swapped row / column or a misplaced rank cannot cancel."""
    assert R <= 56
    g = torch.Generator().manual_seed(seed)
    w = (torch.randint(-16, 17, (N, K), generator=g).float() / 32).to(dtype)
    up = torch.randint(-2, 3, (N, R), generator=g).float() / 2
    down = torch.randint(-2, 3, (R, K), generator=g).float() / 16
    return w, up, down


@gpu
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('N,K,R', [(130, 264, 40), (67, 520, 7)])
def test_merge_exact_data_bit_equal(dev, dtype, N, K, R):
    from wan.backend import ops
    w, up, down = _exact_operands(N, K, R, N + K + R, dtype)
    ref = w.double() + up.double() @ down.double()
    assert torch.equal(ref.to(dtype).double(), ref)                  # representable
    wd = w.to(dev)
    ops.lora_merge(wd, up.to(dev), down.to(dev))
    assert torch.equal(wd.cpu().double(), ref), int((wd.cpu().double() != ref).sum())
    # a zero `up` leaves w bit-identical
    w2 = _randn((N, K), 5, 0.02).to(dtype)
    wd = w2.to(dev)
    ops.lora_merge(wd, torch.zeros(N, R, device=dev), down.to(dev))
    assert torch.equal(wd.cpu().view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       w2.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))


@gpu
def test_merge_strided_targets_write_nothing_else(dev):
    from wan.backend import ops
    d, K, R = 70, 72, 9
    # a row slice [d:2d] of a [3d, K] buffer (q | k | v of a fused weight)
    w, up, down = _exact_operands(3 * d, K, R, 11)
    buf = w.to(dev)
    ops.lora_merge(buf[d:2 * d], up[d:2 * d].to(dev), down.to(dev))
    want = w.double().clone()
    want[d:2 * d] += up[d:2 * d].double() @ down.double()
    assert torch.equal(buf.cpu().double(), want)
    # a view with ldw = K + 24: the 24 trailing elements of every row stay
    w, up, down = _exact_operands(d, K + 24, R, 12)
    buf = w.to(dev)
    view = buf[:, :K]
    assert view.stride(0) == K + 24
    ops.lora_merge(view, up.to(dev), down[:, :K].contiguous().to(dev))
    want = w.double().clone()
    want[:, :K] += up.double() @ down[:, :K].double()
    assert torch.equal(buf.cpu().double(), want)


@gpu
def test_merge_refused_arguments(dev):
    from wan.backend import lib, ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
    with pytest.raises(lib.MoviigenHipError):
        ops.lora_merge(z(4, 20, dt=torch.bfloat16), z(4, 2), z(2, 20))       # K % 8 != 0
    with pytest.raises(lib.MoviigenHipError):
        ops.lora_merge(z(4, 8, dt=torch.bfloat16), z(4, 0), z(0, 8))         # R = 0
    with pytest.raises(lib.MoviigenHipError):
        ops.lora_merge(z(4, 8, dt=torch.bfloat16), z(5, 2), z(2, 8))         # up does not fit w
    with pytest.raises(lib.MoviigenHipError):
        ops.lora_merge(z(4, 8, dt=torch.float16), z(4, 2), z(2, 8))
    w = z(4, 8, dt=torch.bfloat16)
    ops.lora_merge(w, z(4, 2), z(2, 8))                                        # the same call with legal arguments
    torch.cuda.synchronize()
    assert not w.any()


# ------------------------------------------------------------------------------------------------
# GPU: the model
# ------------------------------------------------------------------------------------------------
MODEL_TARGETS = [f'blocks.{i}.{a}.{p}' for i in range(CFG['num_layers']) for a in ('self_attn', 'cross_attn') for p in 'qkvo'] + \
    [f'blocks.{i}.ffn.{j}' for i in range(CFG['num_layers']) for j in (0, 2)] + ['time_projection.1']


def _model(dev, precision='bf16'):
    import wan
    m = wan.modules.WanModel(**CFG)
    m.load_state_dict(W.make_dit_params(CFG, 0))
    m.to(dev)
    return m.set_gemm_precision(precision)


def _shapes(m):
    return {n: tuple(w.shape) for n, w in m.lora_targets().items()}


def _forward(m, dev):
    lat = W.randn((16, 5, 16, 16), 20).to(dev)    # 5 x 8 x 8 = 320 tokens, as tests/test_gemm_mxfp8.py
    ctx = W.randn((33, 128), 30).to(dev)
    return m([lat], t=torch.tensor([700], device=dev), context=[ctx], seq_len=320)[0].clone()


def _sd(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _check_state(sd, base, adapters, tag):
    """sd against base + the fp64 merge of `adapters` = [(factors {name: (up, down)}, scale)], the scale folded into up in fp32 as
    load_lora does; every tensor no adapter names is bit-unchanged."""
    names = {n for fac, _ in adapters for n in fac}
    for n in sorted(names):
        fs = [(fac[n], s) for fac, s in adapters if n in fac]
        up = torch.cat([u * torch.tensor(s, dtype=torch.float32) for (u, _), s in fs], 1)
        down = torch.cat([d for (_, d), _ in fs], 0)
        check_merge(sd[n + '.weight'], base[n + '.weight'], up, down, f'{tag} {n}')
    for k, v in base.items():
        if k[:-len('.weight')] not in names or not k.endswith('.weight'):
            assert torch.equal(sd[k], v), k


@gpu
@pytest.mark.parametrize('precision', ['bf16', 'mxfp8'])
def test_model_forward_after_merge_equals_fresh_model(dev, precision):
    """a stale packed weight, cached cross k|v or quantised weight would show here"""
    import wan
    m = _model(dev, precision)
    fac = _factors(_shapes(m), MODEL_TARGETS, 8, 300)
    base = _sd(m)
    y0 = _forward(m, dev)
    assert m.lora == []
    m.load_lora(_spell(fac, 'kohya'), 0.8)
    assert m.lora == [('<dict>', 0.8)]
    y1 = _forward(m, dev)
    assert torch.isfinite(y1).all() and not torch.equal(y1, y0)
    fresh = wan.modules.WanModel(**CFG)
    fresh.load_state_dict(m.state_dict())
    fresh.to(dev).set_gemm_precision(precision)
    assert torch.equal(_forward(fresh, dev), y1)
    if precision == 'bf16':
        _check_state(_sd(m), base, [(fac, 0.8)], 'model')
    m.unload_lora()
    assert m.lora == []
    sd = _sd(m)
    assert all(torch.equal(sd[k], v) for k, v in base.items())
    assert torch.equal(_forward(m, dev), y0)


@gpu
def test_model_fused_siblings_untouched(dev):
    m = _model(dev)
    _forward(m, dev)                              # q | k | v and cross k | v are views of the fused storage from here on
    base = _sd(m)
    fac = _factors(_shapes(m), ['blocks.0.self_attn.k', 'blocks.1.cross_attn.v', 'text_embedding.2', 'head.head'], 8, 400)
    m.load_lora(_spell(fac, 'flat'))
    _check_state(_sd(m), base, [(fac, 1.0)], 'siblings')


@gpu
def test_model_two_adapters_strength_and_alpha(dev):
    m = _model(dev)
    base = _sd(m)
    shp = _shapes(m)
    a, b = _factors(shp, MODEL_TARGETS, 8, 500), _factors(shp, MODEL_TARGETS[:6], 24, 600)
    m.load_lora([_spell(a, 'peft'), _spell(b, 'kohya')], [0.5, 0.25])
    assert m.lora == [('<dict>', 0.5), ('<dict>', 0.25)]
    _check_state(_sd(m), base, [(a, 0.5), (b, 0.25)], 'two adapters')
    m.unload_lora()
    # strength 0: nothing moves
    m.load_lora(_spell(a, 'peft'), 0.0)
    sd = _sd(m)
    assert all(torch.equal(sd[k].view(torch.uint8), v.view(torch.uint8)) for k, v in base.items())
    m.unload_lora()
    # alpha = 4 at rank 8 is strength 0.5
    m.load_lora(_spell(a, 'kohya', alpha=4.0))
    with_alpha = _sd(m)
    m.unload_lora()
    m.load_lora(_spell(a, 'kohya'), 0.5)
    sd = _sd(m)
    assert all(torch.equal(sd[k], v) for k, v in with_alpha.items())
    assert not torch.equal(sd['blocks.0.ffn.0.weight'], base['blocks.0.ffn.0.weight'])


@gpu
def test_model_refusals(dev):
    import wan
    m = _model(dev)
    ad = _spell(_factors(_shapes(m), MODEL_TARGETS[:2], 8, 700), 'kohya')
    with pytest.raises(RuntimeError, match='nothing|no adapters'):
        m.unload_lora()
    m.load_lora(ad, keep_base=False)
    with pytest.raises(RuntimeError, match=r'unload_lora\(\) first'):
        m.load_lora(ad)
    with pytest.raises(RuntimeError, match='keep_base'):
        m.unload_lora()
    m2 = _model(dev)
    m2._shards = object()                         # what wan.distributed.fsdp.BlockShards installs
    with pytest.raises(NotImplementedError, match='shard'):
        m2.load_lora(ad)
    cpu = wan.modules.WanModel(**CFG)
    cpu.load_state_dict(W.make_dit_params(CFG, 0))
    with pytest.raises(RuntimeError, match='HIP device'):
        cpu.load_lora(ad)
    with pytest.raises(ValueError):
        _model(dev).load_lora({**ad, 'patch_embedding.lora_down.weight': torch.zeros(8, 64),
                               'patch_embedding.lora_up.weight': torch.zeros(256, 8)})


@gpu
def test_want2v_lora_argument(dev, tmp_path):
    import wan
    from safetensors.torch import save_file
    from wan.configs import Config
    m = _model(dev)
    path = str(tmp_path / 'adapter.safetensors')
    save_file(_spell(_factors(_shapes(m), MODEL_TARGETS, 8, 800), 'flat', alpha=8.0), path)
    m.load_lora(path, 0.8)
    model = wan.modules.WanModel(**CFG)
    model.load_state_dict(W.make_dit_params(CFG, 0))
    vae = wan.modules.WanVAE(state_dict=W.make_vae_params(8, 1), device=dev)
    conf = Config(num_train_timesteps=1000, param_dtype=torch.bfloat16, vae_stride=(4, 8, 8), patch_size=(1, 2, 2), sample_neg_prompt='',
                  vae_checkpoint='', text_len=CFG['text_len'])
    pipe = wan.WanT2V(conf, '', device_id=0, model=model, vae=vae, lora=path, lora_strength=0.8)
    assert pipe.model.lora == [(path, 0.8)] == m.lora
    sd, want = _sd(pipe.model), _sd(m)
    assert all(torch.equal(sd[k], v) for k, v in want.items())
    assert not torch.equal(sd['blocks.1.ffn.2.weight'], W.make_dit_params(CFG, 0)['blocks.1.ffn.2.weight'].bfloat16())
