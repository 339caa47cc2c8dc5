"""The VAE decoder's kernels (-m gpu), each called through wan.backend.ops and compared over EVERY output element with a plain fp64 torch
reference on the CPU that is written here: vae_conv / vae_upconv_phases (+ their W-band forms), vae_rmsnorm_silu, vae_attn / vae_attn_rows,
vae_latent_in, vae_video_out, vae_time_interleave, video_to_u8, image_to_u8 -- and the argument checks of their wrappers.

Every output is allocated with one extra trailing slab (a frame, a row or a channel plane) that holds GUARD; the kernel gets the leading view,
whose elements start as NaN.  After the call the view has to be finite, the slab untouched and every input bit-identical (`launch`).  Inputs
are drawn from +-[0.5, 1.5] unless a test says otherwise: no term of a sum is negligible and nothing is subnormal.

Kinds of check, named at each test:
  EXACT     torch.equal: copies, and results that have to be the bits of another launch (W bands, row subsets, tile overrides).
  DERIVED   |out - ref| <= n * 2^-24 * S per element: S = the sum of the absolute values of the element's terms (a second pass of the
            reference over the absolute values of the inputs), n = the roundings of the kernel's longest chain, counted at the test.
  MEASURED  where the device uses __expf / expf, whose error is not derivable here: the figure measured on an MI355X is written at the test,
            the assertion is 4 x that figure and has to stay under a cap that IS derived.

The CPU tests (no marker) pin the references themselves: the fp64 convolution against the point-sampled _conv_ref_f64 of test_gpu_parity.py,
and an fp32 CPU evaluation of each formula against each derived bound and cap, on the inputs the GPU tests use.

The rejection cases hand the wrappers views into larger allocations the test owns (never an undersized allocation, never pageable host
memory); behind every pytest.raises the parent still holds its fill, which shows that nothing was launched."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32
GUARD = 123.0           # the trailing slab of every output, and the fill of the rejection cases' parents


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def floats(shape, seed):
    """fp32 from +-[0.5, 1.5]"""
    g = _gen(seed)
    mag = 0.5 + torch.rand(tuple(shape), generator=g, dtype=torch.float32)
    return torch.where(torch.rand(tuple(shape), generator=g) < 0.5, -mag, mag)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def launch(dev, out_shape, call, *inputs, prefill=None):
    """Run call(out, *device copies of inputs) with out = the leading view of a tensor that has one more slab along dimension 0.
    -> out on the CPU, after checking: out finite, the slab still GUARD, the inputs bit-identical.  prefill(out) may prepare the view (default: NaN)."""
    buf = torch.full((out_shape[0] + 1, *out_shape[1:]), GUARD, dtype=torch.float32, device=dev)
    out = buf[:out_shape[0]]
    assert out.is_contiguous()
    if prefill is None:
        out.fill_(float('nan'))
    else:
        prefill(out)
    ins = [None if t is None else t.to(dev) for t in inputs]
    before = [None if t is None else t.clone() for t in ins]
    call(out, *ins)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), 'an output element was not written'
    assert bool((buf[out_shape[0]:] == GUARD).all()), 'the kernel wrote behind its output'
    for a, b in zip(ins, before):
        assert a is None or torch.equal(bits(a), bits(b)), 'the kernel changed an input'
    return out.cpu()


def worst(out, ref64, bound64):
    """max over all elements of |out - ref| / bound (0 / 0 counts as 0: an exact zero against a zero bound)"""
    err = (out.double() - ref64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound64)
    return ratio.max().item()


# ------------------------------------------------------------------------------------------------
# convolution: vae_conv, vae_upconv_fold_weights + vae_upconv_phases
# ------------------------------------------------------------------------------------------------
def conv_ref(x, w, bias=None, cache=None, residual=None, up2=False):
    """fp64 F.conv3d over [zeros | cache | x] (causal in time, zero 'same' padding in H and W, nearest-2x along H and W first when up2), bias
    and residual added behind it.  x [T,H,W,Cin], w [Cout,kt,kh,kw,Cin], cache [tc <= kt - 1,H,W,Cin], residual [T,Ho,Wo,Cout].
    -> (ref, S): S = the same evaluation on the absolute values = per element the sum of |term| over its terms."""
    def run(x, w, bias, cache, residual):
        Cout, kt, kh, kw, Cin = w.shape
        frames = x if cache is None else torch.cat([cache, x], 0)
        if up2:
            frames = frames.repeat_interleave(2, 1).repeat_interleave(2, 2)
        inp = frames.permute(3, 0, 1, 2)[None]                                     # [1,Cin,tc+T,H,W]
        inp = F.pad(inp, (kw // 2, kw // 2, kh // 2, kh // 2, kt - 1 - (frames.shape[0] - x.shape[0]), 0))
        y = F.conv3d(inp, w.permute(0, 4, 1, 2, 3))[0].permute(1, 2, 3, 0)         # [T,Ho,Wo,Cout]
        if bias is not None:
            y = y + bias
        if residual is not None:
            y = y + residual
        return y.contiguous()
    d = [None if t is None else t.double() for t in (x, w, bias, cache, residual)]
    return run(*d), run(*[None if t is None else t.abs() for t in d])


def conv_n(kt, kh, kw, Cin, phases=False):
    """roundings of one output's longest chain in vae_conv_kernel: one per step of the fma chain over taps x channels (the channels of a tap
    are padded to the 32-channel chunk; the phase form runs 2x2 taps), the epilogue's acc * scale, + bias, + residual, and for the phase form
    the up to three fp32 additions that fold a weight."""
    taps = 4 if phases else kt * kh * kw
    return taps * 32 * math.ceil(Cin / 32) + 3 + (3 if phases else 0)


def split_bf16(t):
    """the split of the bf16x3 mode: hi = bf16(x), lo = bf16(x - hi), both rounded to nearest"""
    hi = t.bfloat16().float()
    return hi, (t - hi).bfloat16().float()


def conv_inputs(Cin, Cout, k, T, H, W, tc, has_bias, has_res, form, seed):
    kt, kh, kw = k
    x = floats((T, H, W, Cin), seed)
    w = floats((Cout, kt, kh, kw, Cin), seed + 1)
    bias = floats((Cout,), seed + 2) if has_bias else None
    cache = floats((tc, H, W, Cin), seed + 3) if tc else None
    up = form != 'plain'
    res = floats((T, 2 * H if up else H, 2 * W if up else W, Cout), seed + 4) if has_res else None
    return x, w, bias, cache, res


# (Cin, Cout, (kt, kh, kw), T, H, W, tc, bias, residual, form).  launch_conv: Cout <= 4 -> the 4x4x1 form (not for phases), <= 32 -> one cout
# block, % 128 -> four, % 96 -> three, else four with a ragged last tile (40: one tile, 200: two).  M = T Ho Wo voxels against the 128 / 256 tile.
# cv_epilogue: Cout 40 and 200 skip whole quads behind Cout; a quad that CROSSES Cout goes element by element, which a convolution reaches with
# rows of Cout <= 4 only (phases_20_3_M322, with bias; no such call has a residual): Cout > 4 that is no multiple of 4 is refused, because the
# whole quads of its rows would be float4 accesses off their alignment (test_conv_refuses_ragged_rows).
CONV_CASES = {
    'head_cin4_M322':        (4, 3, (3, 3, 3), 2, 7, 23, 2, True, True, 'plain'),
    'head_T1_tc2':           (96, 3, (3, 3, 3), 1, 5, 9, 2, True, False, 'plain'),
    'c20_12_1x3x3':          (20, 12, (1, 3, 3), 3, 5, 7, 0, False, False, 'plain'),
    'c32_32_tc1_M306':       (32, 32, (3, 3, 3), 2, 9, 17, 1, True, True, 'plain'),
    'c36_40_ragged_res':     (36, 40, (3, 3, 3), 2, 7, 23, 2, True, True, 'plain'),
    'c36_40_1x1x1_H1':       (36, 40, (1, 1, 1), 1, 1, 130, 0, True, False, 'plain'),
    'c96_96_M567':           (96, 96, (3, 3, 3), 3, 9, 21, 2, True, True, 'plain'),
    'c96_128_W1':            (96, 128, (1, 3, 3), 2, 13, 1, 0, True, True, 'plain'),
    'c384_192_1x1x1':        (384, 192, (1, 1, 1), 1, 10, 13, 0, False, True, 'plain'),
    'c20_200_W2':            (20, 200, (3, 3, 3), 2, 75, 2, 1, True, True, 'plain'),
    'c384_384_T1_tc2':       (384, 384, (3, 3, 3), 1, 10, 13, 2, True, True, 'plain'),
    'c192_384_3x1x1':        (192, 384, (3, 1, 1), 2, 5, 13, 2, True, False, 'plain'),
    'c32_128_nobias_tc0':    (32, 128, (3, 3, 3), 2, 5, 13, 0, False, False, 'plain'),
    'up2_192_96':            (192, 96, (1, 3, 3), 2, 5, 7, 0, True, False, 'up2'),
    'up2_36_32_H1W1':        (36, 32, (1, 3, 3), 3, 1, 1, 0, False, True, 'up2'),
    'up2_4_3':               (4, 3, (1, 3, 3), 1, 3, 5, 0, True, True, 'up2'),
    'phases_192_96':         (192, 96, (1, 3, 3), 2, 5, 7, 0, True, False, 'phases'),
    'phases_20_3_M322':      (20, 3, (1, 3, 3), 2, 7, 23, 0, True, False, 'phases'),
    'phases_36_40':          (36, 40, (1, 3, 3), 1, 9, 17, 0, False, False, 'phases'),
    'phases_96_200_H1':      (96, 200, (1, 3, 3), 2, 1, 70, 0, True, False, 'phases'),
    'phases_384_128_W1':     (384, 128, (1, 3, 3), 1, 13, 1, 0, True, False, 'phases'),
    'phases_4_12_W2':        (4, 12, (1, 3, 3), 3, 25, 2, 0, True, False, 'phases'),
}


def conv_bound(n, S, mode_bf16x3):
    return ((3 * 2.0 ** -18 if mode_bf16x3 else 0.0) + n * U) * S


@gpu
@pytest.mark.parametrize('case', list(CONV_CASES))
def test_conv_every_element(dev, case):
    """DERIVED, both arithmetics, every element.
    exact:   |out - ref| <= n 2^-24 S, n = conv_n (the fma chain, the epilogue, the weight fold).
    bf16x3:  |out - ref| <= (3 * 2^-18 + n 2^-24) S: the split rounds to nearest, so x - hi - lo <= 2^-18 |x|, and the three dropped terms
             (w_lo x_lo, and the two remainders) are each <= 2^-18 |w x|.  Cout <= 4 runs the exact kernel in either mode: the exact bound.
    The tile overrides (mode bits 8-9) have to give the default's bits at Cout 96 and 128.
    Worst err / bound on an MI355X: exact 0.030 (c36_40_1x1x1_H1), bf16x3 0.275 (phases_4_12_W2); with the w_lo x_hi product taken out of the
    kernel the bf16x3 ratio is 1.1 .. 78 in every case but the exact-kernel ones and c384_384_T1_tc2 (0.17: 10368 terms hide one in 2^9)."""
    from wan.backend import ops
    Cin, Cout, k, T, H, W, tc, has_bias, has_res, form = CONV_CASES[case]
    x, w, bias, cache, res = conv_inputs(*CONV_CASES[case], seed=sum(map(ord, case)))
    ref, S = conv_ref(x, w, bias, cache, res, up2=form != 'plain')
    n = conv_n(*k, Cin, phases=form == 'phases')

    def call(mode):
        def f(out, x, w, bias, cache, res):
            if form == 'phases':
                ops.vae_upconv_phases(x, ops.vae_upconv_fold_weights(w), bias, out, mode=mode)
            else:
                ops.vae_conv(x, w, bias, out, *k, cache=cache, up2=form == 'up2', residual=res, mode=mode)
        return launch(dev, tuple(ref.shape), f, x, w, bias, cache, res)

    exact = call(ops.VAE_EXACT)
    r = worst(exact, ref, conv_bound(n, S, False))
    print(f'conv {case}: exact worst err/bound {r:.3f} (n = {n})')
    assert r <= 1, (case, 'exact', r)
    fast = call(ops.VAE_BF16X3)
    fast_is_exact = Cout <= 4 and form != 'phases'
    r = worst(fast, ref, conv_bound(n, S, not fast_is_exact))
    print(f'conv {case}: bf16x3 worst err/bound {r:.3f}')
    assert r <= 1, (case, 'bf16x3', r)
    if fast_is_exact:
        assert torch.equal(fast, exact)
    if Cout in (96, 128):
        for flag in (1, 2):
            assert torch.equal(call(ops.VAE_EXACT | (flag << 8)), exact), (case, 'tile flag', flag)


def test_conv_reference_cpu():
    """the references on the CPU: conv_ref against the point-sampled _conv_ref_f64 (plain with cache, and up2), S against a direct sum, and
    an fp32 evaluation -- F.conv3d in fp32, and the three bf16x3 products of the split operands -- against the bounds the GPU tests assert."""
    from test_gpu_parity import _conv_ref_f64
    for (Cin, Cout, k, T, H, W, tc, form) in ((8, 6, (3, 3, 3), 2, 4, 5, 2, 'plain'), (8, 6, (3, 3, 3), 3, 3, 4, 1, 'plain'), (4, 5, (1, 3, 3), 2, 3, 4, 0, 'up2')):
        x, w, bias, cache, res = conv_inputs(Cin, Cout, k, T, H, W, tc, True, True, form, seed=5)
        up = form == 'up2'
        ref, S = conv_ref(x, w, bias, cache, res, up2=up)
        Ho, Wo = ref.shape[1:3]
        pts = [(t, y, xx) for t in range(T) for y in range(Ho) for xx in range(Wo)]
        pr = _conv_ref_f64(x, cache, w, bias, pts, up2=up).reshape(T, Ho, Wo, Cout) + res.double()
        assert (ref - pr).abs().max().item() <= 1e-12 * S.max().item()
        pa = _conv_ref_f64(x.abs(), None if cache is None else cache.abs(), w.abs(), bias.abs(), pts, up2=up).reshape(T, Ho, Wo, Cout) + res.double().abs()
        assert (S - pa).abs().max().item() <= 1e-12 * S.max().item()
    for case in ('c20_12_1x3x3', 'c36_40_ragged_res', 'up2_4_3', 'phases_36_40'):
        Cin, Cout, k, T, H, W, tc, has_bias, has_res, form = CONV_CASES[case]
        x, w, bias, cache, res = conv_inputs(*CONV_CASES[case], seed=sum(map(ord, case)))
        up = form != 'plain'
        ref, S = conv_ref(x, w, bias, cache, res, up2=up)
        n = conv_n(*k, Cin, phases=form == 'phases')

        def f32(xx, ww, cc, with_tail=True):
            frames = xx if cc is None else torch.cat([cc, xx], 0)
            if up:
                frames = frames.repeat_interleave(2, 1).repeat_interleave(2, 2)
            inp = F.pad(frames.permute(3, 0, 1, 2)[None], (k[2] // 2, k[2] // 2, k[1] // 2, k[1] // 2, k[0] - 1 - tc, 0))
            y = F.conv3d(inp, ww.permute(0, 4, 1, 2, 3))[0].permute(1, 2, 3, 0)
            if with_tail and bias is not None:
                y = y + bias
            if with_tail and res is not None:
                y = y + res
            return y
        r = worst(f32(x, w, cache), ref, conv_bound(n, S, False))
        assert r <= 1, (case, r)
        (xh, xl), (wh, wl) = split_bf16(x), split_bf16(w)
        ch, cl = (None, None) if cache is None else split_bf16(cache)
        three = f32(xh, wl, ch, False).double() + f32(xl, wh, cl, False).double() + f32(xh, wh, ch).double()
        r = worst(three, ref, conv_bound(n, S, True))
        assert r <= 1, (case, 'bf16x3', r)
        # what the bf16x3 assertion is there to catch: without one cross product the result leaves the bound (where the sum is short: the
        # lost term is 2^-9 of a product with a random sign, the bound grows with the length of the sum)
        if k[0] * k[1] * k[2] * Cin > 200:
            continue
        assert worst(f32(xl, wh, cl, False).double() + f32(xh, wh, ch).double(), ref, conv_bound(n, S, True)) > 1


# ------------------------------------------------------------------------------------------------
# the W-band forms: vae_conv_cols, vae_upconv_phases_cols
# ------------------------------------------------------------------------------------------------
BAND_W = 7
BANDS = ((0, 2), (2, 2), (4, 1), (5, 2))     # (first column, columns): left edge (halo right only) | interior | one interior column | right edge


def band_of(t, c0, cols):
    """columns [c0, c0 + cols) of t [.,H,W,C] with the halo columns that exist attached, as _Band.halo builds it -> (band, col0 inside it)"""
    nl, nr = int(c0 > 0), int(c0 + cols < t.shape[2])
    return t[:, :, c0 - nl:c0 + cols + nr].contiguous(), nl


@gpu
@pytest.mark.parametrize('cin,cout', [(96, 96), (192, 384), (20, 3), (36, 40)])
def test_conv_cols_bands(dev, cin, cout):
    """EXACT: the four bands of a 7-column image, 3x3x3 with a two-frame cache (haloed like x) and a compact residual, in both arithmetics ==
    those columns of the whole-image launch."""
    from wan.backend import ops
    T, H = 2, 11
    x, w, bias, cache, res = conv_inputs(cin, cout, (3, 3, 3), T, H, BAND_W, 2, True, True, 'plain', seed=cin + cout)
    for mode in (ops.VAE_EXACT, ops.VAE_BF16X3):
        whole = launch(dev, (T, H, BAND_W, cout), lambda out, x, w, b, c, r: ops.vae_conv(x, w, b, out, 3, 3, 3, cache=c, residual=r, mode=mode),
                       x, w, bias, cache, res)
        for c0, cols in BANDS:
            xb, col0 = band_of(x, c0, cols)
            cb, _ = band_of(cache, c0, cols)
            got = launch(dev, (T, H, cols, cout),
                         lambda out, x, w, b, c, r: ops.vae_conv_cols(x, w, b, out, 3, 3, 3, col0, cache=c, residual=r, mode=mode),
                         xb, w, bias, cb, res[:, :, c0:c0 + cols].contiguous())
            assert torch.equal(got, whole[:, :, c0:c0 + cols]), (mode, c0, cols)


@gpu
@pytest.mark.parametrize('cin,cout', [(96, 96), (192, 384), (20, 3)])
def test_upconv_phases_cols_bands(dev, cin, cout):
    """EXACT: the same four bands through the phase up-convolution == columns [2 c0, 2 (c0 + cols)) of the whole-image launch."""
    from wan.backend import ops
    T, H = 2, 11
    x, w, bias, _, _ = conv_inputs(cin, cout, (1, 3, 3), T, H, BAND_W, 0, True, False, 'phases', seed=cin + cout + 1)
    for mode in (ops.VAE_EXACT, ops.VAE_BF16X3):
        whole = launch(dev, (T, 2 * H, 2 * BAND_W, cout), lambda out, x, w, b: ops.vae_upconv_phases(x, ops.vae_upconv_fold_weights(w), b, out, mode=mode),
                       x, w, bias)
        for c0, cols in BANDS:
            xb, col0 = band_of(x, c0, cols)
            got = launch(dev, (T, 2 * H, 2 * cols, cout),
                         lambda out, x, w, b: ops.vae_upconv_phases_cols(x, ops.vae_upconv_fold_weights(w), b, out, col0, mode=mode), xb, w, bias)
            assert torch.equal(got, whole[:, :, 2 * c0:2 * (c0 + cols)]), (mode, c0, cols)


# ------------------------------------------------------------------------------------------------
# vae_rmsnorm_silu: one wave per row, <= 2 float4 per lane
# ------------------------------------------------------------------------------------------------
NORM_C = (4, 8, 96, 252, 256, 260, 384, 512)       # C / 4 = 1, 2, 24, 63, 64, 65, 96, 128 float4 against 64 lanes
NORM_ROWS = (1, 3, 4, 5, 1027)                     # 4 rows per workgroup


def norm_inputs(rows, C):
    x, gamma = floats((rows, C), rows + C), floats((C,), C)
    if rows >= 3:
        x[1] *= 2.0 ** -30                         # squares down to 2^-62 and up to 2^61.2: neither subnormal nor infinite in fp32
        x[2] *= 2.0 ** 30
    if rows >= 4:
        x[3] = 0                                   # has to come out all zero: 0 / max(0, 1e-12)
    return x, gamma


def norm_ref(x, gamma):
    """-> (pre-activation, its SiLU) in fp64: x / max(|x|, 1e-12) * sqrt(C) * gamma"""
    x, gamma = x.double(), gamma.double()
    pre = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) * math.sqrt(x.shape[-1]) * gamma
    return pre, pre * torch.sigmoid(pre)


def norm_n(C):
    """relative roundings without SiLU: the sum of squares (all terms positive) carries at most C / 4 + 6 + 2 additions and one product, the
    square root halves that and adds one, then sqrtf(C), the division and the two multiplications; one to spare for second-order terms."""
    return (C // 4 + 6 + 2 + 1) / 2 + 1 + 1 + 1 + 2 + 1


# MEASURED on an MI355X: max |y - ref| / max(|ref|, |pre| 2^-24) over every case of test_rmsnorm_silu with do_silu (the seeds of norm_inputs):
# 3.838e-07 at C = 512, rows = 1027 -- 2^-21.3 (every other case 0.8e-07 .. 3.6e-07).  The assertion is 4 x that (the margin is for __expf at other arguments) and may not exceed 2^-18.
NORM_SILU_MEASURED = 3.838e-07
NORM_SILU_CAP = 2.0 ** -18
assert 4 * NORM_SILU_MEASURED <= NORM_SILU_CAP


@gpu
@pytest.mark.parametrize('C', NORM_C)
def test_rmsnorm_silu(dev, C):
    """DERIVED without SiLU (norm_n, relative to |ref|: a zero row has to be exactly zero); MEASURED with it (NORM_SILU_MEASURED)."""
    from wan.backend import ops
    for rows in NORM_ROWS:
        x, gamma = norm_inputs(rows, C)
        pre, act = norm_ref(x, gamma)
        for do_silu in (False, True):
            y = launch(dev, (rows, C), lambda out, x, g: ops.vae_rmsnorm_silu(x, g, out, do_silu), x, gamma)
            if rows >= 4:
                assert bool((y[3] == 0).all())
            if not do_silu:
                r = worst(y, pre, norm_n(C) * U * pre.abs())
                assert r <= 1, (C, rows, r)
                continue
            m = ((y.double() - act).abs() / torch.maximum(act.abs(), pre.abs() * U).clamp_min(1e-300)).max().item()
            print(f'rmsnorm+silu C = {C}, rows = {rows}: measured {m:.3e}')
            assert m <= NORM_SILU_CAP and m <= 4 * NORM_SILU_MEASURED, (C, rows, m)


@gpu
def test_rmsnorm_second_grid_trip(dev):
    """DERIVED: more rows than the capped grid of 65536 * 8 workgroups x 4 rows holds at once; the last rows belong to the second trip."""
    from wan.backend import ops
    rows, C = 65536 * 8 * 4 + 5, 4
    x, gamma = floats((rows, C), 1), floats((C,), 2)
    pre, _ = norm_ref(x, gamma)
    y = launch(dev, (rows, C), lambda out, x, g: ops.vae_rmsnorm_silu(x, g, out, False), x, gamma)
    assert worst(y, pre, norm_n(C) * U * pre.abs()) <= 1


def test_rmsnorm_reference_cpu():
    """the formula in fp32 on the CPU stays inside the derived bound on the GPU test's inputs, and SiLU in fp32 inside the cap of the measured one"""
    for C in NORM_C:
        x, gamma = norm_inputs(5, C)
        pre, act = norm_ref(x, gamma)
        ss = (x * x).sum(-1, keepdim=True)
        y = x * (torch.tensor(float(C)).sqrt() / ss.sqrt().clamp_min(1e-12)) * gamma
        assert worst(y, pre, norm_n(C) * U * pre.abs()) <= 1, C
        assert bool((y[3] == 0).all())
        s = y / (1 + torch.exp(-y))
        assert ((s.double() - act).abs() / torch.maximum(act.abs(), pre.abs() * U).clamp_min(1e-300)).max().item() <= NORM_SILU_CAP, C


# ------------------------------------------------------------------------------------------------
# vae_attn, vae_attn_rows: S = q k^T / sqrt(C) (exact-fp32 GEMM), a row softmax with expf, P.V in K slices
# ------------------------------------------------------------------------------------------------
ATTN_CASES = ((2, 1, 32), (1, 3, 4), (2, 5, 32), (1, 130, 4), (2, 130, 96), (1, 130, 384), (1, 2047, 32), (1, 2049, 32), (2, 2178, 32))   # frames, L, C
PEAK = 80.0


def walsh(m, C):
    """+-1 pattern number m < 4 over C channels (C % 4 == 0): the four patterns are mutually orthogonal"""
    c = torch.arange(C)
    return 1.0 - 2.0 * (((c & m) & 1) ^ (((c & m) >> 1) & 1)).float()


@functools.lru_cache(maxsize=None)
def attn_inputs(family, frames, L, C):
    """-> (qkv [frames, L, 3C], planted [L] or None; the planted key dominates the EVEN rows).
    soft:  q, k ~ N(0, 1): scores ~ N(0, 1); v from +-[0.5, 1.5].
    peaky: A = min(4, L // 2) anchor keys 3 h_m (h_m = walsh patterns) and their negatives among keys from +-[0.5, 1.5]; query i is
           b h_(i mod A) + noise / sqrt(C) with b = PEAK / (3 sqrt(C)): its score with its anchor is PEAK, with the negative -PEAK, with another
           anchor 0 and with any other key at most PEAK / 2 in magnitude -- the anchor dominates by e^-30 or less (checked in
           test_attn_reference_cpu), so the row's output has to be the anchor's value row.  L = 1: the only key.  That is for the even rows;
           an odd row asks for two anchors at once, b (h_m + h_(m+1)) / 2 (A >= 2): two scores near PEAK / 2 that differ by the noise only, so
           both keys count behind large logits -- the rows on which the metric measures something."""
    seed = 1000 * L + C + frames
    if family == 'soft':
        q, k = (torch.randn(frames, L, C, generator=_gen(seed + i)) for i in range(2))
        return torch.cat([q, k, floats((frames, L, C), seed + 2)], -1).contiguous(), None
    k, v = floats((frames, L, C), seed + 1), floats((frames, L, C), seed + 2)
    A = max(1, min(4, L // 2))
    pos = [(m * L) // (2 * A) for m in range(2 * A)] if L > 1 else [0]               # anchors at pos[0..A), their negatives at pos[A..2A)
    for m in range(A):
        k[:, pos[m]] = 3 * walsh(m, C)
        if L > 1:
            k[:, pos[A + m]] = -3 * walsh(m, C)
    rows = torch.arange(L) % A
    h = torch.stack([walsh(m, C) for m in range(A)])
    odd = (torch.arange(L) % 2 == 1)[:, None]
    q = torch.where(odd, (h[rows] + h[(rows + 1) % A]) / 2, h[rows])[None] * (PEAK / (3 * math.sqrt(C))) + floats((frames, L, C), seed) / math.sqrt(C)
    return torch.cat([q, k, v], -1).contiguous(), torch.tensor(pos)[rows]


def attn_ref(qkv, dtype=torch.float64):
    """softmax attention in `dtype` -> (out, denominator of the metric: sum_j p_ij |v_j|, cap of the metric per frame)"""
    q, k, v = qkv.to(dtype).chunk(3, -1)
    C, L = q.shape[-1], q.shape[1]
    p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C), -1)
    amax = (q.double().abs() @ k.double().abs().transpose(1, 2)).amax() / math.sqrt(C)
    # the scores' rounding (C products, relative to sum |q k| / sqrt(C)) enters exp on both sides of the normalisation; plus the two accumulations
    cap = (C + L + 8) * U * (1 + 2 * amax.item())
    return p @ v, p @ v.abs(), cap


# MEASURED on an MI355X, per case (frames, L, C) in the order of ATTN_CASES: max over all elements of |out - ref| / sum_j p_ij |v_j| against the
# fp64 reference.  Each case is asserted at 4 x its own figure.  0: the output is the value row of the one key that counts, bit for bit (L = 1;
# peaky L = 3 has a single anchor, so its odd row is decided too).  The largest of each family is at C = 384 (soft 5.011e-07, peaky 1.657e-05):
# the rounding of a score grows with the number of its products, and on the peaky odd rows scores of 40 enter expf.
ATTN_MEASURED = {'soft': dict(zip(ATTN_CASES, (0.0, 9.433e-08, 1.623e-07, 1.107e-07, 2.519e-07, 5.011e-07, 1.401e-07, 1.122e-07, 1.276e-07))),
                 'peaky': dict(zip(ATTN_CASES, (0.0, 0.0, 6.830e-06, 1.686e-06, 1.192e-05, 1.657e-05, 8.517e-06, 8.009e-06, 9.215e-06)))}


@gpu
@pytest.mark.parametrize('frames,L,C', ATTN_CASES)
@pytest.mark.parametrize('family', ['soft', 'peaky'])
def test_attn(dev, family, frames, L, C):
    """MEASURED, every element, metric |out - ref| / sum_j p_ij |v_j|: asserted at 4 x ATTN_MEASURED of the case, which has to stay under the derived cap
    (C + L + 8) 2^-24 (1 + 2 max_ij sum_c |q_ic k_jc| / sqrt(C)).  peaky: every row's output is bit for bit its planted key's value row."""
    from wan.backend import ops
    qkv, planted = attn_inputs(family, frames, L, C)
    ref, den, cap = attn_ref(qkv)

    def f(out, qkv):
        ops.vae_attn(qkv, out, torch.empty(ops.vae_attn_workspace_floats(L, C), device=dev))
    out = launch(dev, (frames, L, C), f, qkv)
    m = ((out.double() - ref).abs() / den).max().item()
    print(f'attn {family} frames = {frames}, L = {L}, C = {C}: measured {m:.3e}, cap {cap:.3e}')
    assert 4 * ATTN_MEASURED[family][frames, L, C] <= cap
    assert m <= 4 * ATTN_MEASURED[family][frames, L, C], (family, frames, L, C, m)
    if planted is not None:
        assert torch.equal(out[:, ::2], qkv[..., 2 * C:][:, planted[::2]]), 'a peaky row is not its planted value row'


def test_attn_reference_cpu():
    """an fp32 evaluation of the same formula stays under the cap on every case's inputs, and the peaky inputs are what their docstring says:
    scores reach +-PEAK, and the planted key leads every other by at least 30"""
    for frames, L, C in ATTN_CASES:
        for family in ('soft', 'peaky'):
            qkv, planted = attn_inputs(family, frames, L, C)
            ref, den, cap = attn_ref(qkv)
            m = ((attn_ref(qkv, torch.float32)[0].double() - ref).abs() / den).max().item()
            assert m <= cap, (family, frames, L, C, m, cap)
            assert 4 * ATTN_MEASURED[family][frames, L, C] <= cap, (family, frames, L, C, cap)
            if planted is None:
                continue
            q, k, v = qkv.double().chunk(3, -1)
            s = q @ k.transpose(1, 2) / math.sqrt(C)
            top = s.gather(2, planted.expand(frames, L)[..., None])
            assert bool((top[:, ::2] > PEAK - 10).all()) and bool((top[:, ::2] < PEAK + 10).all())
            if L > 1:
                assert bool((s.amin(-1)[:, ::2] < -(PEAK - 10)).all())
                lead = top - s.scatter(2, planted.expand(frames, L)[..., None], -1e9).amax(-1, keepdim=True)
                assert bool((lead[:, ::2] >= 30).all()), (frames, L, C, lead[:, ::2].min().item())
            if L >= 4:      # two anchors: on the odd rows the second key counts in fp32, behind scores of about PEAK / 2
                assert bool((torch.softmax(s, -1).topk(2).values[:, 1::2, 1] >= 1e-5).all()) and bool((s.amax(-1)[:, 1::2] > PEAK / 2 - 10).all())
            assert torch.equal(ref.float()[:, ::2], v[:, planted[::2]].float())


@functools.lru_cache(maxsize=None)
def attn_full(family, frames, L, C):
    """vae_attn of a case on the GPU, computed once for the row-subset tests -> (qkv, out), both on the CPU"""
    from wan.backend import ops
    d = torch.device('cuda:0')
    qkv, _ = attn_inputs(family, frames, L, C)
    out = torch.empty(frames, L, C, device=d)
    ops.vae_attn(qkv.to(d), out, torch.empty(ops.vae_attn_workspace_floats(L, C), device=d))
    return qkv, out.cpu()


@gpu
@pytest.mark.parametrize('frames,Lk,C,Lq', [(2, 2178, 32, 1), (2, 2178, 32, 37), (2, 2178, 32, 2049), (1, 130, 384, 1), (1, 130, 384, 37)])
@pytest.mark.parametrize('family', ['soft', 'peaky'])
def test_attn_rows(dev, family, frames, Lk, C, Lq):
    """EXACT: a subset of the query rows (strided through the image; 2049 rows = two query blocks, the second ragged) against all keys == those
    rows of vae_attn, with q compact and with q a column slice of a [frames, Lq, 3C] tensor."""
    from wan.backend import ops
    qkv, full = attn_full(family, frames, Lk, C)
    step = 17 if Lq > 100 else 3                                        # 17 is coprime to 2178: 2049 distinct rows
    idx = (torch.arange(Lq) * step + Lk // 2) % Lk
    rows3 = qkv[:, idx].contiguous()                                    # [frames, Lq, 3C]
    kv = qkv[..., C:].contiguous()

    def f(sliced):
        def g(out, q, kv):
            ops.vae_attn_rows(q[..., :C] if sliced else q, kv, out, torch.empty(ops.vae_attn_workspace_floats(Lk, C), device=dev))
        return g
    assert torch.equal(launch(dev, (frames, Lq, C), f(False), rows3[..., :C].contiguous(), kv), full[:, idx])
    assert torch.equal(launch(dev, (frames, Lq, C), f(True), rows3, kv), full[:, idx])


# ------------------------------------------------------------------------------------------------
# glue: vae_latent_in, vae_video_out, vae_time_interleave, video_to_u8, image_to_u8 (grid-stride loops under a capped grid)
# ------------------------------------------------------------------------------------------------
def distinct(shape):
    """fp32 tensor whose elements are all different (exact integers below 2^24): a copy that mixes up two elements fails"""
    n = math.prod(shape)
    assert n < 2 ** 24
    return torch.arange(n, dtype=torch.float32).reshape(shape)


@gpu
@pytest.mark.parametrize('shape', [(1, 1, 1, 2), (3, 5, 7, 6), (2, 1, 9, 10), (1, 3, 1, 8), (1, 540, 540, 16)], ids=str)
def test_time_interleave(dev, shape):
    """EXACT (a copy).  The last shape has 2 * 540 * 540 * 8 > 16384 * 256 elements: a second trip round the grid-stride loop."""
    from wan.backend import ops
    T, H, W, C2 = shape
    x = distinct(shape)
    ref = torch.stack([x[..., :C2 // 2], x[..., C2 // 2:]], 1).reshape(2 * T, H, W, C2 // 2)
    assert torch.equal(launch(dev, tuple(ref.shape), lambda out, x: ops.vae_time_interleave(x, out), x), ref)


@gpu
@pytest.mark.parametrize('shape', [(1, 1, 1, 1), (3, 5, 7, 3), (2, 9, 1, 3), (2, 1, 11, 5), (5, 540, 540, 3)], ids=str)
def test_video_out(dev, shape):
    """EXACT: x [T,H,W,C] -> out[:, t_off:t_off + T] clamped to [-1, 1], for t_off = 0, middle and last of a longer out; the frames outside
    the window keep their fill.  Values: all different, inside (-1, 1), exactly +-1, outside, and +-inf.
    NaN: the kernel's fminf(1, fmaxf(-1, x)) turns NaN into -1 where torch.clamp would propagate it.  That is the kernel's behaviour since the
    decoder exists and it is kept and pinned here (and stated in the wrapper's docstring): a video handed to the uint8 conversion holds numbers."""
    from wan.backend import ops
    T, H, W, C = shape
    n = math.prod(shape)
    x = (distinct(shape) / n * 2.5 - 1.25)                              # [-1.25, 1.25): different values on both sides of and inside the range
    flat = x.view(-1)
    special = torch.tensor([1.0, -1.0, float('inf'), float('-inf'), float('nan'), 1.0000001, -1.0000001])
    flat[:min(n, 7)] = special[:min(n, 7)]
    ref = x.clamp(-1, 1).nan_to_num(nan=-1.0).permute(3, 0, 1, 2)          # [C,T,H,W]
    extra = 4 if n < 10 ** 6 else 2
    for t_off in sorted({0, extra // 2, extra}):
        def prefill(out):
            out.fill_(GUARD)
            out[:, t_off:t_off + T] = float('nan')
        out = launch(dev, (C, T + extra, H, W), lambda out, x: ops.vae_video_out(x, out, t_off), x, prefill=prefill)
        assert torch.equal(out[:, t_off:t_off + T], ref), t_off
        assert bool((out[:, :t_off] == GUARD).all()) and bool((out[:, t_off + T:] == GUARD).all()), 'a frame outside the window was written'


def latent_in_case(shape):
    C = shape[0]
    z, mean, inv_std = floats(shape, sum(shape)), floats((C + 3,), 1), floats((C,), 2)
    q = z.double() / inv_std.double()[:, None, None, None]
    m = mean.double()[:C, None, None, None]
    return z, mean, inv_std, (q + m).permute(1, 2, 3, 0), 2 * U * (q.abs() + m.abs()).permute(1, 2, 3, 0)


LATENT_SHAPES = [(16, 3, 5, 7), (1, 1, 1, 1), (5, 1, 3, 1), (3, 2, 1, 9), (16, 3, 210, 210)]


@gpu
@pytest.mark.parametrize('shape', LATENT_SHAPES, ids=str)
def test_latent_in(dev, shape):
    """DERIVED: z [C,T,H,W] -> [T,H,W,C] = z / inv_std + mean, two roundings: <= 2 * 2^-24 (|z / inv_std| + |mean|).  mean may be longer than C.
    The last shape has 16 * 3 * 210 * 210 > 8192 * 256 elements: a second trip round the grid-stride loop."""
    from wan.backend import ops
    z, mean, inv_std, ref, bound = latent_in_case(shape)
    out = launch(dev, tuple(ref.shape), lambda out, z, m, s: ops.vae_latent_in(z, m, s, out), z, mean, inv_std)
    assert worst(out, ref, bound) <= 1


def test_latent_in_reference_cpu():
    for shape in LATENT_SHAPES[:4]:
        z, mean, inv_std, ref, bound = latent_in_case(shape)
        y = (z / inv_std[:, None, None, None] + mean[:shape[0], None, None, None]).permute(1, 2, 3, 0)
        assert worst(y, ref, bound) <= 1


def u8_values(lo, hi, n):
    """n fp32 values for the uint8 conversions of the range [lo, hi]: on the k/255 and (k + 1/2)/255 grids (where the truncating and the
    rounding cast change their result) and one fp32 step to either side of each, lo, hi, values outside, and random ones"""
    span = max(hi - lo, 1e-5)
    k = torch.arange(0, 256, dtype=torch.float64)
    grid = torch.cat([lo + k / 255 * span, lo + (k + 0.5) / 255 * span]).float()
    inf = torch.tensor(float('inf'))
    pts = torch.cat([grid, torch.nextafter(grid, inf), torch.nextafter(grid, -inf),
                     torch.tensor([lo, hi, lo - 1, hi + 1, lo - 1e-3, hi + 1e-3, 0.0, -0.0, 1e30, -1e30], dtype=torch.float32)])
    fill = lo - 0.1 * span + 1.2 * span * torch.rand(max(n - pts.numel(), 0), generator=_gen(n), dtype=torch.float32)
    v = torch.cat([pts, fill])[:n]
    return v[torch.randperm(n, generator=_gen(n + 1))]


def u8_ref(v, lo, hi, rounding):
    """the reference arithmetic, every step in fp32: clamp, (x - lo) / max(hi - lo, 1e-5) * 255, (+ 0.5, clamp to 0..255,) truncating cast"""
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    span = torch.maximum(hi32 - lo32, torch.tensor(1e-5, dtype=torch.float32))
    y = (torch.minimum(torch.maximum(v, lo32), hi32) - lo32) / span * 255.0
    if rounding:
        y = (y + 0.5).clamp(0.0, 255.0)
    return y.to(torch.int32).to(torch.uint8)


U8_RANGES = [(-1.0, 1.0), (0.0, 1.0), (-0.3, 0.9), (0.25, 0.25)]


@gpu
@pytest.mark.parametrize('lo,hi', U8_RANGES)
def test_video_to_u8(dev, lo, hi):
    """EXACT against the fp32 arithmetic of u8_ref (truncating), lo == hi included; shapes with odd sizes and sizes of 1, and one with
    5 * 920 * 920 > 16384 * 256 pixels (a second trip round the grid-stride loop) for the default range."""
    from wan.backend import ops
    shapes = [(1, 1, 1), (3, 5, 7), (1, 1, 1571), (2, 9, 1)] + ([(5, 920, 920)] if (lo, hi) == (-1.0, 1.0) else [])
    for T, H, W in shapes:
        v = u8_values(lo, hi, 3 * T * H * W).reshape(3, T, H, W)
        d = v.to(dev)
        got = ops.video_to_u8(d, lo, hi)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (T, H, W, 3) and torch.equal(bits(d.cpu()), bits(v))
        assert torch.equal(got.cpu(), u8_ref(v, lo, hi, False).permute(1, 2, 3, 0)), (T, H, W)


@gpu
@pytest.mark.parametrize('lo,hi', U8_RANGES)
def test_image_to_u8(dev, lo, hi):
    """EXACT against u8_ref with rounding (+ 0.5, clamp, truncate); 2050 * 2050 > 16384 * 256 pixels for the default range."""
    from wan.backend import ops
    shapes = [(1, 1), (5, 7), (1, 1571), (523, 1)] + ([(2050, 2050)] if (lo, hi) == (-1.0, 1.0) else [])
    for H, W in shapes:
        v = u8_values(lo, hi, 3 * H * W).reshape(3, H, W)
        d = v.to(dev)
        got = ops.image_to_u8(d, lo, hi)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (H, W, 3) and torch.equal(bits(d.cpu()), bits(v))
        assert torch.equal(got.cpu(), u8_ref(v, lo, hi, True).permute(1, 2, 0)), (H, W)


def test_u8_reference_cpu():
    """u8_ref against the same arithmetic in fp64 away from the cast's steps, and the test values do sit on those steps"""
    for lo, hi in U8_RANGES:
        v = u8_values(lo, hi, 4000)
        y = (v.double().clamp(lo, hi) - lo) / max(hi - lo, 1e-5) * 255
        for rounding in (False, True):
            yy = (y + 0.5).clamp(0, 255) if rounding else y
            away = (yy - yy.round()).abs() > 1e-3
            assert torch.equal(u8_ref(v, lo, hi, rounding)[away], yy.floor().to(torch.uint8)[away])
            assert hi == lo or int((~away).sum()) >= 256


# ------------------------------------------------------------------------------------------------
# the wrappers' argument checks
# ------------------------------------------------------------------------------------------------
def host(t):
    """the tensor in pinned host memory: not a CUDA tensor for the wrapper, yet memory the device may touch"""
    return t.cpu().pin_memory()


def wider(t):
    """a view of t's shape that is not dense: the leading columns of a tensor twice as wide (innermost stride 1), every second element for a vector"""
    big = torch.full((*t.shape[:-1], 2 * t.shape[-1]), GUARD, dtype=t.dtype, device=t.device)
    return big[::2] if t.dim() == 1 else big[..., :t.shape[-1]]


def rejects(call, parents):
    """call raises MoviigenHipError and no parent buffer changed"""
    from wan.backend import lib
    with pytest.raises(lib.MoviigenHipError):
        call()
    torch.cuda.synchronize()
    for p in parents:
        assert bool((p == GUARD).all()), 'a rejected call wrote to its output'


def each_bad(good, bad):
    """good: dict of valid arguments; bad: (argument, replacement) pairs -> one argument dict per pair, the others valid"""
    for name, value in bad:
        yield name, {**good, name: value}


def common_bad(good, names):
    """for every tensor argument in names: another dtype, host memory, a strided view of the same shape"""
    for n in names:
        t = good[n]
        yield n, t.double()
        yield n, t.to(torch.bfloat16)
        yield n, host(t)
        yield n, wider(t)


@gpu
def test_conv_wrappers_reject(dev):
    """vae_conv / vae_conv_cols: every operand's dtype, device and density; w against (kt, kh, kw, Cin); out and residual against the exact
    output shape (a short out, a long out, another Cout, the up2 shape for a plain call and the reverse); the cache's geometry and length;
    bias's length; the column window."""
    from wan.backend import ops
    T, H, W, Cin, Cout = 2, 3, 5, 8, 12
    parent = torch.full((T + 2, H, W, Cout), GUARD, device=dev)
    parent_up = torch.full((T + 1, 2 * H, 2 * W, Cout), GUARD, device=dev)
    good = dict(x=floats((T, H, W, Cin), 1).to(dev), w=floats((Cout, 3, 3, 3, Cin), 2).to(dev), bias=floats((Cout,), 3).to(dev), out=parent[:T],
                cache=floats((2, H, W, Cin), 4).to(dev), residual=floats((T, H, W, Cout), 5).to(dev))
    parents = [parent, parent_up]

    def conv(a, k=(3, 3, 3), up2=False):
        ops.vae_conv(a['x'], a['w'], a['bias'], a['out'], *k, cache=a['cache'], up2=up2, residual=a['residual'])

    def cols(a, col0=1, k=(3, 3, 3)):
        ops.vae_conv_cols(a['x'], a['w'], a['bias'], a['out'], *k, col0, cache=a['cache'], residual=a['residual'])
    shape_bad = [('x', good['x'].transpose(1, 2)), ('x', good['x'][0]), ('w', floats((Cout, 3, 3, 3, Cin + 4), 2).to(dev)), ('w', floats((Cout, 1, 3, 3, Cin), 2).to(dev)),
                 ('w', good['w'].reshape(Cout, 27, Cin)), ('w', good['w'].transpose(2, 3)), ('bias', floats((Cin,), 3).to(dev)), ('bias', floats((Cout + 4,), 3).to(dev)),
                 ('out', parent[:T - 1]), ('out', parent[:T + 1]), ('out', parent.view(-1)[:T * H * W * 8].view(T, H, W, 8)), ('out', parent_up[:T]),
                 ('out', parent[:T].transpose(1, 2)), ('out', parent[:T].view(T, H * W, Cout)), ('out', None),
                 ('residual', floats((T, H, W, 8), 5).to(dev)), ('residual', floats((T - 1, H, W, Cout), 5).to(dev)), ('residual', good['residual'].transpose(1, 2)),
                 ('cache', floats((3, H, W, Cin), 4).to(dev)), ('cache', floats((2, H, W - 1, Cin), 4).to(dev)), ('cache', floats((2, H, W, Cin + 4), 4).to(dev)),
                 ('cache', good['cache'].view(2, H * W, Cin))]
    for name, a in each_bad(good, list(common_bad(good, ('x', 'w', 'bias', 'out', 'cache', 'residual'))) + shape_bad):
        rejects(lambda: conv(a), parents)
    rejects(lambda: conv(good, k=(1, 3, 3)), parents)                                   # w is 3x3x3
    rejects(lambda: conv(good, up2=True), parents)                                      # out and residual have the plain shape
    rejects(lambda: conv({**good, 'out': parent_up[:T], 'residual': None}), parents)    # the up2 shape for a plain call
    w1 = floats((Cout, 1, 3, 3, Cin), 2).to(dev)
    rejects(lambda: conv({**good, 'w': w1}, k=(1, 3, 3)), parents)                      # kt = 1 admits no cache frame
    # the band form: out [T, H, cols, Cout] with cols = 3 of the W = 5 columns of x
    band = torch.full((T + 1, H, 3, Cout), GUARD, device=dev)
    parents.append(band)
    gb = {**good, 'out': band[:T], 'residual': floats((T, H, 3, Cout), 6).to(dev)}
    for name, a in each_bad(gb, list(common_bad(gb, ('x', 'w', 'bias', 'out', 'cache', 'residual'))) +
                            [('out', parent[:T]), ('out', band[:T - 1]), ('out', band[:T].transpose(1, 2)), ('residual', good['residual']),
                             ('cache', floats((2, H, 3, Cin), 4).to(dev)), ('w', floats((Cout, 3, 3, 3, Cin + 4), 2).to(dev)), ('bias', floats((Cin,), 3).to(dev))]):
        rejects(lambda: cols(a), parents)
    for col0 in (-1, 3, 5):                                                             # [col0, col0 + 3) leaves the 5 columns of x
        rejects(lambda: cols(gb, col0), parents)


@gpu
@pytest.mark.parametrize('Cout', [6, 42, 43])
def test_conv_refuses_ragged_rows(dev, Cout):
    """more than 4 output channels that are no multiple of 4: the kernel would move the whole quads of out / residual rows as float4 at addresses
    that are only 4- or 8-byte aligned.  Refused by every convolution -- by the wrapper where it checks shapes, by the library's launcher for all
    (vae_conv_strided and vae_conv_in3 reach it: their wrappers leave Cout to it)."""
    from wan.backend import ops
    T, H, W, Cin = 2, 4, 6, 8
    x, bias = floats((T, H, W, Cin), 1).to(dev), floats((Cout,), 2).to(dev)
    w3, w1 = floats((Cout, 3, 3, 3, Cin), 3).to(dev), floats((Cout, 1, 3, 3, Cin), 4).to(dev)
    wp = floats((4, Cout, 2, 2, Cin), 5).to(dev)
    xs, w4 = floats((T, H, W + 2, 4), 6).to(dev), floats((Cout, 3, 3, 3, 4), 7).to(dev)
    parent = torch.full((T + 1, 2 * H, 2 * W, Cout), GUARD, device=dev)

    def out(*shape):                                                    # a dense [T, *shape, Cout] inside parent
        n = T * math.prod(shape) * Cout
        return parent.view(-1)[:n].view(T, *shape, Cout)
    res = floats((T, H, W, Cout), 8).to(dev)
    rejects(lambda: ops.vae_conv(x, w3, bias, out(H, W), 3, 3, 3, residual=res), [parent])
    rejects(lambda: ops.vae_conv(x, w1, bias, out(2 * H, 2 * W), 1, 3, 3, up2=True), [parent])
    rejects(lambda: ops.vae_conv_cols(x, w3, bias, out(H, 3), 3, 3, 3, 1), [parent])
    rejects(lambda: ops.vae_upconv_phases(x, wp, bias, out(2 * H, 2 * W)), [parent])
    rejects(lambda: ops.vae_upconv_phases_cols(x, wp, bias, out(2 * H, 6), 1), [parent])
    shp = ops.vae_conv_strided_out_shape(x.shape, (1, 3, 3), (1, 2, 2), 0, (0, 1), (0, 1))
    rejects(lambda: ops.vae_conv_strided(x, w1, bias, out(*shp[1:]), (1, 2, 2), 0, (0, 1), (0, 1)), [parent])
    rejects(lambda: ops.vae_conv_in3(xs, w4, bias, out(H, W), cache=None), [parent])


@gpu
def test_upconv_wrappers_reject(dev):
    """vae_upconv_fold_weights, vae_upconv_phases, vae_upconv_phases_cols: wp is [4, Cout, 2, 2, Cin], out [T, 2H, 2W or 2 cols, Cout]"""
    from wan.backend import ops
    T, H, W, Cin, Cout = 2, 3, 5, 8, 12
    parent = torch.full((T + 2, 2 * H, 2 * W, Cout), GUARD, device=dev)
    band = torch.full((T + 1, 2 * H, 6, Cout), GUARD, device=dev)
    parents = [parent, band]
    w = floats((Cout, 1, 3, 3, Cin), 1).to(dev)
    for bad in (w.double(), host(w), wider(w), w.transpose(2, 3), w.view(Cout, 9, Cin)):
        rejects(lambda: ops.vae_upconv_fold_weights(bad), parents)
    good = dict(x=floats((T, H, W, Cin), 2).to(dev), wp=floats((4, Cout, 2, 2, Cin), 3).to(dev), bias=floats((Cout,), 4).to(dev), out=parent[:T])
    shape_bad = [('x', good['x'].transpose(1, 2)), ('wp', floats((4, Cout, 2, 2, Cin + 4), 3).to(dev)), ('wp', floats((3, Cout, 2, 2, Cin), 3).to(dev)),
                 ('wp', w), ('wp', good['wp'].view(4 * Cout, 2, 2, Cin)), ('bias', floats((Cin,), 4).to(dev)),
                 ('out', parent[:T - 1]), ('out', parent[:T + 1]), ('out', parent[:T, :H, :W]), ('out', parent[:T].transpose(1, 2)), ('out', band[:T])]
    for name, a in each_bad(good, list(common_bad(good, ('x', 'wp', 'bias', 'out'))) + shape_bad):
        rejects(lambda: ops.vae_upconv_phases(a['x'], a['wp'], a['bias'], a['out']), parents)
    gb = {**good, 'out': band[:T]}
    for name, a in each_bad(gb, list(common_bad(gb, ('x', 'wp', 'bias', 'out'))) +
                            [('out', parent[:T]), ('out', band[:T - 1]), ('out', band[:T, :, :5]), ('out', band[:T].view(T, 2 * H, 3, 2 * Cout)),
                             ('wp', floats((4, Cout, 2, 2, Cin + 4), 3).to(dev)), ('bias', floats((Cout + 4,), 4).to(dev))]):
        rejects(lambda: ops.vae_upconv_phases_cols(a['x'], a['wp'], a['bias'], a['out'], 1), parents)
    for col0 in (-1, 3):
        rejects(lambda: ops.vae_upconv_phases_cols(gb['x'], gb['wp'], gb['bias'], gb['out'], col0), parents)


@gpu
def test_rmsnorm_wrapper_rejects(dev):
    """vae_rmsnorm_silu: fp32, dense, gamma of C elements, out of x's shape; a C the library refuses (not a multiple of 4, above 512) and
    operands that are not 16-byte aligned (x, gamma and out go as float4) surface as the library's error."""
    from wan.backend import ops
    rows, C = 6, 8
    parent = torch.full((rows + 2, C), GUARD, device=dev)
    good = dict(x=floats((rows, C), 1).to(dev), gamma=floats((C,), 2).to(dev), out=parent[:rows])
    shape_bad = [('gamma', floats((C + 4,), 2).to(dev)), ('gamma', floats((C - 4,), 2).to(dev)), ('out', parent[:rows - 1]), ('out', parent[:rows + 1]),
                 ('out', parent[:rows].t()), ('x', floats((C, rows), 1).to(dev).t()), ('out', parent.view(-1)[:rows * 4].view(rows, 4))]
    # one float off a 16-byte boundary, each inside a larger tensor
    odd = {n: torch.full((t.numel() + 4,), GUARD, device=dev)[1:1 + t.numel()].view(t.shape) for n, t in good.items()}
    parents = [parent] + [t._base for t in odd.values()]
    for name, a in each_bad(good, list(common_bad(good, ('x', 'gamma', 'out'))) + shape_bad + list(odd.items())):
        rejects(lambda: ops.vae_rmsnorm_silu(a['x'], a['gamma'], a['out']), parents)
    for Cb in (6, 516):
        pb = torch.full((4, Cb), GUARD, device=dev)
        rejects(lambda: ops.vae_rmsnorm_silu(floats((3, Cb), 1).to(dev), floats((Cb,), 2).to(dev), pb[:3]), [pb])


@gpu
def test_attn_wrappers_reject(dev):
    """vae_attn: fp32, dense, a last dimension divisible by 3, out [frames, L, C], the workspace, a 16-byte aligned out; vae_attn_rows: the
    same for kv and out, q may be a column slice but not a row-overlapping view, and Lq > Lk has a message of its own."""
    from wan.backend import lib, ops
    frames, L, C = 2, 6, 8
    parent = torch.full((frames + 1, L, C), GUARD, device=dev)
    ws = torch.empty(ops.vae_attn_workspace_floats(L, C), device=dev)
    good = dict(qkv=floats((frames, L, 3 * C), 1).to(dev), out=parent[:frames], ws=ws)
    odd = torch.full((frames * L * C + 4,), GUARD, device=dev)
    parents = [parent, odd]
    shape_bad = [('qkv', floats((frames, L, 3 * C + 1), 1).to(dev)), ('qkv', good['qkv'].view(frames * L, 3 * C)), ('qkv', good['qkv'].transpose(0, 1)),
                 ('out', parent[:frames - 1]), ('out', parent[:frames, :L - 1]), ('out', parent[:frames].view(frames, L * 2, C // 2)), ('out', parent[:frames].transpose(0, 1)),
                 ('out', odd[1:1 + frames * L * C].view(frames, L, C)), ('ws', ws[:ws.numel() - 1]), ('ws', ws[::2])]
    for name, a in each_bad(good, list(common_bad(good, ('qkv', 'out', 'ws'))) + shape_bad):
        rejects(lambda: ops.vae_attn(a['qkv'], a['out'], a['ws']), parents)
    Lq = 4
    rows = torch.full((frames + 1, Lq, C), GUARD, device=dev)
    parents.append(rows)
    q3 = floats((frames, Lq, 3 * C), 2).to(dev)
    gr = dict(q=q3[..., :C], kv=floats((frames, L, 2 * C), 3).to(dev), out=rows[:frames], ws=ws)
    bad = [('q', q3[..., :C].double()), ('q', host(q3)[..., :C]), ('q', q3[..., ::3]), ('q', q3[:, :, :C - 4]), ('q', q3[0, :, :C]), ('q', q3[:, ::2, :C]),
           ('q', q3[:1, :, :C].expand(frames, Lq, C)), ('kv', floats((frames, L, 2 * C + 1), 3).to(dev)), ('kv', floats((frames + 1, L, 2 * C), 3).to(dev)),
           ('out', rows[:frames - 1]), ('out', rows[:frames, :Lq - 1]), ('out', rows[:frames].transpose(0, 1)), ('out', parent[:frames]),
           ('ws', ws[:ws.numel() - 1])] + list(common_bad(gr, ('kv', 'out', 'ws')))
    for name, a in each_bad(gr, bad):
        rejects(lambda: ops.vae_attn_rows(a['q'], a['kv'], a['out'], a['ws']), parents)
    with pytest.raises(lib.MoviigenHipError, match='Lq = 4 query rows exceed the Lk = 3 keys'):
        ops.vae_attn_rows(gr['q'], floats((frames, 3, 2 * C), 3).to(dev), gr['out'], ws)
    assert bool((rows == GUARD).all())


@gpu
def test_glue_wrappers_reject(dev):
    """vae_latent_in (out [T,H,W,C], mean and inv_std of at least C), vae_video_out (out [C,T_total,H,W], 0 <= t_off <= T_total - T),
    vae_time_interleave (an even last dimension, out [2T,H,W,C2/2]): fp32, dense, exact shapes."""
    from wan.backend import ops
    C, T, H, W = 4, 2, 3, 5
    p1 = torch.full((T + 1, H, W, C), GUARD, device=dev)
    good = dict(z=floats((C, T, H, W), 1).to(dev), mean=floats((C,), 2).to(dev), inv_std=floats((C + 2,), 3).to(dev), out=p1[:T])
    bad = [('z', good['z'].transpose(0, 1)), ('z', good['z'][0]), ('mean', good['mean'][:C - 1]), ('inv_std', good['inv_std'][:C - 1]), ('mean', good['inv_std'][::2]),
           ('out', p1[:T - 1]), ('out', p1[:T + 1]), ('out', p1[:T].permute(3, 0, 1, 2)), ('out', p1[:T].view(C, T, H, W)), ('out', p1[:T, :, :W - 1])]
    for name, a in each_bad(good, list(common_bad(good, ('z', 'mean', 'inv_std', 'out'))) + bad):
        rejects(lambda: ops.vae_latent_in(a['z'], a['mean'], a['inv_std'], a['out']), [p1])

    Tt = T + 2
    p2 = torch.full((C + 1, Tt, H, W), GUARD, device=dev)
    good = dict(x=floats((T, H, W, C), 4).to(dev), out=p2[:C])
    bad = [('x', good['x'].transpose(1, 2)), ('x', good['x'][0]), ('out', p2[:C - 1]), ('out', p2[:C, :, :H - 1]), ('out', p2[:C, :, :, :W - 1]), ('out', p2[:C, :T - 1]),
           ('out', p2[:C].transpose(0, 1)), ('out', p2[:C].view(C, Tt, H * W)), ('out', p2[:C, :T])]
    for name, a in each_bad(good, list(common_bad(good, ('x', 'out'))) + bad):
        rejects(lambda: ops.vae_video_out(a['x'], a['out'], 1), [p2])
    for t_off in (-1, Tt - T + 1, Tt):
        rejects(lambda: ops.vae_video_out(good['x'], good['out'], t_off), [p2])

    p3 = torch.full((2 * T + 1, H, W, C), GUARD, device=dev)
    good = dict(x=floats((T, H, W, 2 * C), 5).to(dev), out=p3[:2 * T])
    bad = [('x', floats((T, H, W, 2 * C + 1), 5).to(dev)), ('x', good['x'].transpose(1, 2)), ('x', good['x'][0]), ('out', p3[:2 * T - 1]), ('out', p3[:2 * T + 1]), ('out', p3[:T]),
           ('out', p3[:2 * T].view(T, H, W, 2 * C)), ('out', p3[:2 * T].transpose(1, 2)), ('out', p3[:2 * T, :, :, :C - 1])]
    for name, a in each_bad(good, list(common_bad(good, ('x', 'out'))) + bad):
        rejects(lambda: ops.vae_time_interleave(a['x'], a['out']), [p3])
