"""The small DiT and Ulysses kernels (-m gpu), each called through wan.backend.ops and compared with a plain torch reference on the CPU that is
written here: gemv, head_gemm, add_rows, lincomb, cfg_combine, sinusoid_embed, patchify, unpatchify, embed_rows (+ ew_bf16 mode 0), sp_pack_qkv,
sp_unpack_o, sp_copy_blocks — and the argument checks of their wrappers.

Three kinds of check, named in a comment at each test:
  EXACT     the result has to be torch.equal to the reference.  Either the kernel only moves data or rounds once, or its inputs are integer-valued
            fp32 numbers from {-3..3}: every product and partial sum is then an integer below 2^24, exact in fp32 in any order, fused or not.
  DERIVED   random floats from +-[0.5, 1.5] against an fp64 reference of the same fp32 inputs, elementwise
            |out - ref| <= n * 2^-24 * sum|terms|, n = the longest chain of roundings in the kernel (counted in the comment).  With K <= 260
            the bound is three orders of magnitude below one term: a dropped or doubled term fails.
  MEASURED  gemv(silu_in=True) only: the device silu uses __expf, whose error is measured, not derived (SILU_BOUND below).

The rejection cases hand the wrappers views into larger allocations (never an undersized allocation, never pageable host memory), so that even
a missing check could not make a kernel touch memory the test does not own; behind every pytest.raises the parent still holds its fill, which
shows that nothing was launched."""
import math

import pytest
import torch

from sentinels import FILL, FILL16, holds16, host, rejects, sentinel16

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, seed):
    """integer-valued fp32 from {-3..3}"""
    return torch.randint(-3, 4, tuple(shape), generator=_gen(seed)).to(torch.float32)


def floats(shape, seed):
    """fp32 from +-[0.5, 1.5]: no term of a sum is negligible"""
    g = _gen(seed)
    mag = 0.5 + torch.rand(tuple(shape), generator=g, dtype=torch.float32)
    return torch.where(torch.rand(tuple(shape), generator=g) < 0.5, -mag, mag)


def bits16(shape, start=0):
    """bf16 tensor whose element i has the bit pattern (start + i) mod 2^16: neighbours and blocks all differ"""
    n = math.prod(shape)
    return ((torch.arange(start, start + n, dtype=torch.int64) % 65536) - 32768).to(torch.int16).view(torch.bfloat16).reshape(shape)


def eq16(a, b):
    """bit equality of bf16 tensors (NaN patterns included)"""
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


def within(out, ref64, n, mag64):
    """the DERIVED bound, elementwise"""
    err = (out.detach().cpu().double() - ref64).abs()
    bound = n * U * mag64
    assert bool((err <= bound).all()), f'max err/bound {(err / bound).max().item():.3f} (n = {n})'


# ------------------------------------------------------------------------------------------------
# gemv: y[n] = sum_k w[n][k] f(x[k]) + bias[n]; one wave per row, 4 rows per workgroup, K/4 float4 vectors over 64 lanes
# ------------------------------------------------------------------------------------------------
GEMV_N = (1, 3, 5, 777)                  # 4 waves per workgroup: a partly idle last workgroup
GEMV_K = (4, 252, 256, 260, 5120)        # K/4 = 1, 63, 64, 65 vectors against 64 lanes (idle lanes, one trip, one lane with two), and the model's


@pytest.mark.parametrize('K', GEMV_K)
def test_gemv_exact(dev, K):
    """EXACT (integer inputs): every N, with and without bias"""
    from wan.backend import ops
    for N in GEMV_N:
        w, x, b = ints((N, K), N + K), ints((K,), K), ints((N,), N)
        for bias in (None, b):
            y = torch.full((N,), float('nan'), device=dev)
            ops.gemv(w.to(dev), None if bias is None else bias.to(dev), x.to(dev), y)
            ref = (w.double() @ x.double() + (0 if bias is None else bias.double())).float()
            assert torch.equal(y.cpu(), ref), (N, K, bias is not None)


def test_gemv_random(dev):
    """DERIVED.  Rounding chain of one output: per trip a lane rounds a product, a sum of two and the sum of the pairs (3) and adds that to
    its accumulator (ceil(K / 256) trips of 64 lanes x 4), the wave's butterfly adds 6 times, the bias once; one to spare
    -> n = ceil(K / 256) + 3 + 6 + 2."""
    from wan.backend import ops
    N, K = 5, 260
    w, x, b = floats((N, K), 1), floats((K,), 2), floats((N,), 3)
    y = torch.empty(N, device=dev)
    ops.gemv(w.to(dev), b.to(dev), x.to(dev), y)
    prod = w.double() * x.double()
    within(y, prod.sum(1) + b.double(), math.ceil(K / 256) + 3 + 6 + 2, prod.abs().sum(1) + b.double().abs())


# MEASURED: max |y - ref| / sum_k |w_k silu(x_k)| over every case of test_gemv_silu below (N in GEMV_N, with and without bias, seeds as written
# there, inputs from +-[0.5, 1.5]), ref in fp64 with silu in fp64, on an MI355X: 1.494e-07 at K = 4, 2.412e-08 at 252, 1.256e-07 at 256,
# 3.252e-08 at 260, 1.334e-08 at 5120 — the largest is 2^-22.7.  The assertion is 4 x that (the margin is for other seeds), 2^-20.7, and may
# not exceed 2^-18: at K <= 1024 a lost term is >= 2^-10 of the sum and has to fail.
SILU_MEASURED = 1.494e-07
SILU_BOUND = 4 * SILU_MEASURED
assert SILU_BOUND <= 2.0 ** -18


@pytest.mark.parametrize('K', GEMV_K)
def test_gemv_silu(dev, K):
    """MEASURED (see SILU_BOUND)"""
    from wan.backend import ops
    worst = 0.0
    for N in GEMV_N:
        w, x, b = floats((N, K), 10 + N + K), floats((K,), 11 + K), floats((N,), 12 + N)
        for bias in (None, b):
            y = torch.empty(N, device=dev)
            ops.gemv(w.to(dev), None if bias is None else bias.to(dev), x.to(dev), y, silu_in=True)
            xd = x.double()
            prod = w.double() * (xd / (1 + torch.exp(-xd)))
            ref = prod.sum(1) + (0 if bias is None else bias.double())
            worst = max(worst, ((y.cpu().double() - ref).abs() / prod.abs().sum(1)).max().item())
    print(f'gemv silu K={K}: max |y - ref| / sum|w silu(x)| = {worst:.3e}')
    assert worst <= SILU_BOUND


# ------------------------------------------------------------------------------------------------
# head_gemm: out[M][N <= 64] = x[M][K] w[N][K]^T + bias; 64 rows per workgroup, K staged 32 at a time, serial fmaf over K
# ------------------------------------------------------------------------------------------------
HEAD_M = (0, 1, 63, 64, 65, 333)         # no workgroup, one row, around the 64-row tile, several workgroups with a partial last one
HEAD_N = (1, 16, 37, 64)                 # around the 4-column micro-tile, the full 64
HEAD_K = (1, 31, 32, 33, 200)            # around the 32-deep k chunk: a dropped last chunk shows


def _head_case(dev, M, N, K, sliced, use_bias, gen):
    """-> (out on the host, the NaN tail behind it, x, w, bias)"""
    from wan.backend import ops
    xb = gen((M, K + 5), 7 * M + K)
    x = xb[:, 3:3 + K] if sliced else xb[:, :K].contiguous()          # sliced: ldx = K + 5 > K
    w, b = gen((N, K), N + K), gen((N,), N) if use_bias else None
    big = torch.full((M + 3, N), float('nan'), device=dev)             # out is the leading part of a larger allocation
    xd = xb.to(dev)
    ops.head_gemm(xd[:, 3:3 + K] if sliced else x.to(dev), w.to(dev), None if b is None else b.to(dev), big[:M])
    assert bool(torch.isnan(big[M:]).all()), 'head_gemm wrote behind its M rows'
    return big[:M].cpu(), x, w, b


@pytest.mark.parametrize('K', HEAD_K)
def test_head_gemm_exact(dev, K):
    """EXACT (integer inputs): x dense and as a column slice, with and without bias, out followed by NaN that has to stay"""
    for M in HEAD_M:
        for i, N in enumerate(HEAD_N):
            combos = [(False, True), (True, True), (False, False), (True, False)] if M == 65 else [(bool(i & 1), M != 63)]
            for sliced, use_bias in combos:
                out, x, w, b = _head_case(dev, M, N, K, sliced, use_bias, ints)
                ref = (x.double() @ w.double().T + (0 if b is None else b.double())).float()
                assert torch.equal(out, ref), (M, N, K, sliced, use_bias)


def test_head_gemm_exact_model_width(dev):
    """EXACT (integer inputs) at the model's K = 5120, N = 64: 160 k chunks, |sums| <= 9 * 5120 < 2^24"""
    out, x, w, b = _head_case(dev, 65, 64, 5120, True, True, ints)
    assert torch.equal(out, (x.double() @ w.double().T + b.double()).float())


def test_head_gemm_random(dev):
    """DERIVED.  acc = fmaf(x, w, acc) over k in order: K roundings, the bias add, one to spare -> n = K + 2."""
    M, N, K = 65, 37, 200
    out, x, w, b = _head_case(dev, M, N, K, True, True, floats)
    xd, wd = x.double(), w.double()
    within(out, xd @ wd.T + b.double(), K + 2, xd.abs() @ wd.abs().T + b.double().abs())


# ------------------------------------------------------------------------------------------------
# add_rows: out[r] = a[r] + b[r % period]
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,dim,period', [(6, 5120, 6), (12, 128, 6), (7, 33, 3), (2, 5120, 1), (5, 7, 5),
                                             (2051, 513, 6)])     # 1 052 163 elements > 4096 x 256 threads and no multiple of 256: the grid-stride loop
def test_add_rows(dev, rows, dim, period):
    """EXACT on arbitrary floats: one IEEE add per element"""
    from wan.backend import ops
    a = torch.randn(rows, dim, generator=_gen(rows)) * 3
    b = torch.randn(period + (dim == 33), dim, generator=_gen(dim))          # (7, 33, 3): b has a row more than the period uses
    out = torch.full((rows, dim), float('nan'), device=dev)
    ops.add_rows(a.to(dev), b.to(dev), out, period)
    assert torch.equal(out.cpu(), a + b[torch.arange(rows) % period])


# ------------------------------------------------------------------------------------------------
# lincomb (1..4 terms) and cfg_combine: grid-stride loops over 8192 x 256 threads
# ------------------------------------------------------------------------------------------------
FLAT_N = (1, 255, 257, 100003, 8192 * 256 + 77)


@pytest.mark.parametrize('n', FLAT_N)
def test_lincomb_exact(dev, n):
    """EXACT (integer inputs and coefficients), 1 to 4 terms"""
    from wan.backend import ops
    xs = [ints((n,), 40 + i) for i in range(4)]
    xd = [x.to(dev) for x in xs]
    coefs = (2.0, -3.0, 1.0, -1.0)
    for k in (1, 2, 3, 4):
        out = torch.full((n,), float('nan'), device=dev)
        ops.lincomb(out, [(xd[i], coefs[i]) for i in range(k)])
        assert torch.equal(out.cpu(), sum(coefs[i] * xs[i] for i in range(k))), (n, k)


def test_lincomb_zero_coefficient_is_not_skipped(dev):
    """EXACT: 0 * inf is NaN in the reference expression, so it is in the kernel — a term is never skipped for its coefficient"""
    from wan.backend import ops
    n = 257
    x0, x1 = ints((n,), 1), ints((n,), 2)
    x1[5], x1[200] = float('inf'), float('-inf')
    out = torch.empty(n, device=dev)
    ops.lincomb(out, [(x0.to(dev), 2.0), (x1.to(dev), 0.0)])
    ref = 2.0 * x0 + 0.0 * x1
    assert torch.isnan(ref[5]) and torch.isnan(ref[200]) and int(torch.isnan(ref).sum()) == 2
    assert torch.equal(torch.isnan(out.cpu()), torch.isnan(ref)) and torch.equal(torch.nan_to_num(out.cpu()), torch.nan_to_num(ref))


def test_lincomb_random(dev):
    """DERIVED.  Four products and three sums, fused or not, are at most 7 roundings; one to spare -> n = 8."""
    from wan.backend import ops
    n = 100003
    xs, cs = [floats((n,), 50 + i) for i in range(4)], [0.75, -1.3, 0.6180339887, 1.1]
    out = torch.empty(n, device=dev)
    ops.lincomb(out, [(x.to(dev), c) for x, c in zip(xs, cs)])
    c32 = [torch.tensor(c, dtype=torch.float32).double() for c in cs]          # the coefficients reach the kernel as fp32
    terms = [c * x.double() for c, x in zip(c32, xs)]
    within(out, sum(terms), 8, sum(t.abs() for t in terms))


def test_cfg_combine_reference_expression(dev):
    """against the reference pipeline's own expression (its op order) on normal inputs: 1e-6 of the scale"""
    import weights as W
    from wan.backend import ops
    u, c = W.randn((1000,), 20), W.randn((1000,), 21)
    o = torch.empty(1000, dtype=torch.float32, device=dev)
    ops.cfg_combine(o, u.to(dev), c.to(dev), 5.0)
    ref = u + 5.0 * (c - u)
    assert ((o.cpu().double() - ref.double()).abs().max() / ref.double().abs().max()).item() < 1e-6


@pytest.mark.parametrize('n', FLAT_N)
def test_cfg_combine_exact(dev, n):
    """EXACT (integer inputs, integer g): out = u + g (c - u)"""
    from wan.backend import ops
    u, c = ints((n,), 60), ints((n,), 61)
    ud, cd = u.to(dev), c.to(dev)
    for g in (1.0, 5.0, 0.0):
        out = torch.full((n,), float('nan'), device=dev)
        ops.cfg_combine(out, ud, cd, g)
        assert torch.equal(out.cpu(), u + g * (c - u)), (n, g)


def test_cfg_combine_random(dev):
    """DERIVED.  c - u, g *, u +: 3 roundings (2 when fused), one to spare -> n = 4; the terms are u, g c and g u."""
    from wan.backend import ops
    n, g = 100003, 7.5
    u, c = floats((n,), 62), floats((n,), 63)
    out = torch.empty(n, device=dev)
    ops.cfg_combine(out, u.to(dev), c.to(dev), g)
    ud, cd = u.double(), c.double()
    within(out, ud + g * (cd - ud), 4, ud.abs() + g * cd.abs() + g * ud.abs())


# ------------------------------------------------------------------------------------------------
# sinusoid_embed: fp64 evaluation, fp32 result; 128 threads per workgroup over n * dim/2
# ------------------------------------------------------------------------------------------------
def _sinusoid_ref(pos, dim):
    """the reference formula in fp64, rounded once: half = dim/2, frequencies 10000^(-j/half), [cos | sin]"""
    half = dim // 2
    freq = torch.pow(torch.tensor(10000.0, dtype=torch.float64), -torch.arange(half, dtype=torch.float64) / half)
    a = torch.outer(pos.double(), freq)
    return torch.cat([torch.cos(a), torch.sin(a)], 1).float()


SIN_TOL = 2.0 ** -23     # DERIVED: both sides evaluate in fp64 on arguments <= 1000 (they differ by far less than an fp32 ulp) and round once to fp32 in [-1, 1]


def test_sinusoid_vs_oracle(dev):
    """against the oracle (1e-6 of the scale), and SIN_TOL on the same call"""
    from oracle import dit
    from wan.backend import ops
    t = torch.tensor([999, 500, 3])
    out = torch.empty(3, 256, dtype=torch.float32, device=dev)
    ops.sinusoid_embed(t.to(dev), 256, out)
    ref = dit.sinusoid(256, t).float()
    assert ((out.cpu().double() - ref.double()).abs().max() / ref.double().abs().max()).item() < 1e-6
    assert (out.cpu() - _sinusoid_ref(t, 256)).abs().max().item() <= SIN_TOL


@pytest.mark.parametrize('dtype', [torch.int64, torch.float32, torch.float64])
def test_sinusoid(dev, dtype):
    """DERIVED (SIN_TOL): n * dim/2 around and below the 128-thread workgroup, positions 0, 0.5, 999, 1000"""
    from wan.backend import ops
    positions = [0, 1, 999, 1000, 37] if dtype == torch.int64 else [0.0, 0.5, 999.0, 1000.0, 37.25]
    for k, dim in enumerate((2, 6, 256, 258)):
        for n in (1, 3, 5):
            pos = torch.tensor([positions[(k + i) % 5] for i in range(n)], dtype=dtype)      # rotated: every position is used at every n overall
            out = torch.full((n, dim), float('nan'), device=dev)
            ops.sinusoid_embed(pos.to(dev), dim, out)
            assert (out.cpu() - _sinusoid_ref(pos, dim)).abs().max().item() <= SIN_TOL, (dtype, dim, n)


# ------------------------------------------------------------------------------------------------
# patchify / unpatchify: index plumbing, grid-stride loops over 8192 x 256 threads
# ------------------------------------------------------------------------------------------------
PATCH_CASES = [(16, 3, 8, 12, 2, 2), (3, 1, 3, 6, 1, 3), (5, 2, 4, 4, 2, 1), (16, 1, 2, 2, 2, 2),
               (16, 3, 210, 212, 2, 2)]         # 2 136 960 elements > 8192 x 256


def _patch_index(C, F, H, W, ph, pw):
    """for token row t = (f, hg, wg) and column k = (c, i, j): the latent coordinates, as index tensors [L, 1] / [1, Kd]"""
    Hg, Wg = H // ph, W // pw
    t = torch.arange(F * Hg * Wg)[:, None]
    k = torch.arange(C * ph * pw)[None, :]
    f, hg, wg = t // (Hg * Wg), (t // Wg) % Hg, t % Wg
    c, i, j = k // (ph * pw), (k // pw) % ph, k % pw
    return c, f, hg * ph + i, wg * pw + j, i, j


def _ties(x):
    """exact ties of the fp32 -> bf16 rounding at the start of x: 1 + 2^-8 rounds down to even, 1 + 3 * 2^-8 up to even, both signs"""
    flat = x.view(-1)
    vals = [1 + 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 3 * 2.0 ** -8, -(1 + 3 * 2.0 ** -8)]
    flat[:min(4, flat.numel())] = torch.tensor(vals[:min(4, flat.numel())])
    return x


@pytest.mark.parametrize('C,F,H,W,ph,pw', PATCH_CASES)
def test_patchify(dev, C, F, H, W, ph, pw):
    """EXACT: one round-to-nearest-even fp32 -> bf16 per element; out dense, and with ldo > C ph pw where the gap keeps its bits"""
    from wan.backend import ops
    lat = _ties(torch.randn(C, F, H, W, generator=_gen(C + H)))
    c, f, h, w, _, _ = _patch_index(C, F, H, W, ph, pw)
    ref = lat[c, f, h, w].bfloat16()
    L, Kd = ref.shape
    assert eq16(_ties(torch.zeros(4)).bfloat16(), torch.tensor([1.0, -1.0, 1 + 2.0 ** -6, -(1 + 2.0 ** -6)]).bfloat16())     # the ties are ties
    for pad in (0, 3):
        buf = sentinel16((L + 1, Kd + pad), dev)
        ops.patchify(lat.to(dev), ph, pw, buf[:L, :Kd] if pad else buf[:L])
        assert eq16(buf[:L, :Kd], ref), pad
        assert holds16(buf[L:]) and holds16(buf[:, Kd:]), pad


def test_unpatchify_vs_oracle(dev):
    """EXACT: bit equality with the golden-checked oracle"""
    import weights as W
    from oracle import dit
    from wan.backend import ops
    tok = W.randn((24, 64), 13)
    lat = torch.empty(16, 2, 6, 8, dtype=torch.float32, device=dev)
    ops.unpatchify(tok.to(dev), 16, 2, 3, 4, 2, 2, lat)
    assert torch.equal(lat.cpu(), dit.unpatchify(tok, (2, 3, 4), (1, 2, 2), 16))


@pytest.mark.parametrize('C,F,H,W,ph,pw', PATCH_CASES)
def test_unpatchify(dev, C, F, H, W, ph, pw):
    """EXACT (a copy): lat[c][f][h][w] = tok[(f, h/ph, w/pw)][(h%ph, w%pw, c)]; tok dense, and as a column slice (ldt > ph pw C)"""
    from wan.backend import ops
    c, f, h, w, i, j = _patch_index(C, F, H, W, ph, pw)
    L, Kd = f.shape[0], c.shape[1]
    tokb = torch.randn(L, Kd + 5, generator=_gen(F + W))
    tok = tokb[:, 2:2 + Kd]
    ref = torch.full((C, F, H, W), float('nan'))
    ref[c, f, h, w] = tok[torch.arange(L)[:, None], (i * pw + j) * C + c]
    assert not bool(torch.isnan(ref).any())
    for sliced in (False, True):
        big = torch.full((C + 1, F, H, W), float('nan'), device=dev)
        ops.unpatchify(tokb.to(dev)[:, 2:2 + Kd] if sliced else tok.contiguous().to(dev), C, F, H // ph, W // pw, ph, pw, big[:C])
        assert torch.equal(big[:C].cpu(), ref), sliced
        assert bool(torch.isnan(big[C:]).all())


# ------------------------------------------------------------------------------------------------
# embed_rows (128 threads per row over dim/8 vectors) and ew_bf16 mode 0
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dim', [8, 128, 1032])          # dim/8 = 1, 16, 129 vectors against 128 threads
def test_embed_rows(dev, dim):
    """EXACT (a copy): first and last id of the table, repeated ids, and no ids at all"""
    from wan.backend import ops
    vocab = 50
    tab = bits16((vocab, dim), start=dim)
    ids = torch.tensor([0, vocab - 1, 7, 7, vocab - 1, 0, 3], dtype=torch.int64)
    buf = sentinel16((ids.numel() + 1, dim), dev)
    ops.embed_rows(tab.to(dev), ids.to(dev), buf[:ids.numel()])
    assert eq16(buf[:ids.numel()], tab[ids]) and holds16(buf[ids.numel():])
    empty = torch.empty(0, dim, dtype=torch.bfloat16, device=dev)
    assert ops.embed_rows(tab.to(dev), torch.empty(0, dtype=torch.int64, device=dev), empty) is empty


def test_ew_bf16_add(dev):
    """EXACT: mode 0 is one fp32 add of two bf16 values and one rounding; 8 * 259 elements, a multiple of 8 and not of 8 x 256"""
    from wan.backend import ops
    n = 8 * 259
    a, b = torch.randn(n, generator=_gen(1)).bfloat16(), (torch.randn(n, generator=_gen(2)) * 2).bfloat16()
    buf = sentinel16((n + 8,), dev)
    ops.ew_bf16(a.to(dev), b.to(dev), buf[:n], 0)
    assert eq16(buf[:n], (a.float() + b.float()).bfloat16()) and holds16(buf[n:])


# ------------------------------------------------------------------------------------------------
# the Ulysses layouts: sp_pack_qkv, sp_unpack_o, sp_copy_blocks (16-byte vectors, grid-stride over 4096 x 256 threads per block)
# ------------------------------------------------------------------------------------------------
def _pack_ref(srcs, P, cpd, col0, w):
    """send[p, t, i*w:(i+1)*w] = src_i[t, p*cpd + col0 : p*cpd + col0 + w]"""
    Lloc = srcs[0].shape[0]
    send = torch.empty(P, Lloc, 3 * w, dtype=torch.bfloat16)
    for p in range(P):
        for i, s in enumerate(srcs):
            send[p, :, i * w:(i + 1) * w] = s[:, p * cpd + col0:p * cpd + col0 + w]
    return send


def _sp_cases():
    for Lloc in (0, 1, 37):
        for w in (8, 128, 640):
            for col0 in (0, 128):
                yield Lloc, w, col0, col0 + w + (16 if w == 128 else 0)        # the group ends with the block, or 16 columns before its end


@pytest.mark.parametrize('P', [1, 2, 8])
def test_sp_pack_qkv(dev, P):
    """EXACT (a copy): q, k, v as column slices of one fused [Lloc, 3 P cols] buffer; what lies behind send keeps its bits"""
    from wan.backend import ops
    for Lloc, w, col0, cpd in _sp_cases():
        d = P * cpd
        fused = bits16((Lloc, 3 * d), start=Lloc + w)
        fd = fused.to(dev)
        n = P * Lloc * 3 * w
        buf = sentinel16((n + 16,), dev)
        ops.sp_pack_qkv(fd[:, :d], fd[:, d:2 * d], fd[:, 2 * d:], P, cpd, col0, w, buf[:n].view(P, Lloc, 3 * w))
        assert eq16(buf[:n].view(P, Lloc, 3 * w), _pack_ref([fused[:, :d], fused[:, d:2 * d], fused[:, 2 * d:]], P, cpd, col0, w)), (Lloc, w, col0)
        assert holds16(buf[n:])


def test_sp_pack_qkv_separate_and_long(dev):
    """EXACT: q, k, v as three dense tensors of different widths, and 13 200 rows x 640 columns = 1 056 000 vectors > 4096 x 256 threads"""
    from wan.backend import ops
    P, Lloc, w, col0, cpd = 1, 13200, 640, 0, 640
    srcs = [bits16((Lloc, cpd + 8 * i), start=1000 * i) for i in range(3)]
    send = sentinel16((P, Lloc, 3 * w), dev)
    ops.sp_pack_qkv(*(s.to(dev) for s in srcs), P, cpd, col0, w, send)
    assert eq16(send, _pack_ref(srcs, P, cpd, col0, w))


@pytest.mark.parametrize('P', [1, 2, 8])
def test_sp_unpack_o(dev, P):
    """EXACT (a copy): o[t, p*cps + col0 : + w] = recv[p, t, :]; every other column of o, and of the buffer o is a slice of, keeps its bits"""
    from wan.backend import ops
    for Lloc, w, col0, cps in _sp_cases():
        recv = bits16((P, Lloc, w), start=7 * w)
        ob = sentinel16((Lloc, P * cps + 24), dev)
        ops.sp_unpack_o(recv.to(dev), P, cps, col0, w, ob[:, 8:8 + P * cps])         # ldo > P cps, o starts 16 bytes into its row
        got = ob.cpu()
        written = torch.zeros(P * cps + 24, dtype=torch.bool)
        for p in range(P):
            lo = 8 + p * cps + col0
            assert eq16(got[:, lo:lo + w], recv[p]), (Lloc, w, col0, p)
            written[lo:lo + w] = True
        assert holds16(got[:, ~written]), (Lloc, w, col0)


def test_sp_unpack_o_long(dev):
    """EXACT: 13 200 rows x 640 columns, more vectors than 4096 x 256 threads"""
    from wan.backend import ops
    Lloc, w = 13200, 640
    recv = bits16((1, Lloc, w), start=3)
    o = sentinel16((Lloc, w + 8), dev)
    ops.sp_unpack_o(recv.to(dev), 1, w + 8, 8, w, o)
    assert eq16(o[:, 8:], recv[0]) and holds16(o[:, :8])


def test_sp_pack_unpack_round_trip(dev):
    """EXACT: pack, the identity exchange of a group of one (recv = send), unpack -> the packed columns of q | k | v side by side"""
    from wan.backend import ops
    Lloc, w, col0, cpd = 37, 128, 128, 384
    fused = bits16((Lloc, 3 * cpd), start=11).to(dev)
    q, k, v = fused[:, :cpd], fused[:, cpd:2 * cpd], fused[:, 2 * cpd:]
    send = sentinel16((1, Lloc, 3 * w), dev)
    ops.sp_pack_qkv(q, k, v, 1, cpd, col0, w, send)
    o = sentinel16((Lloc, 3 * w), dev)
    ops.sp_unpack_o(send, 1, 3 * w, 0, 3 * w, o)
    for i, s in enumerate((q, k, v)):
        assert eq16(o[:, i * w:(i + 1) * w], s[:, col0:col0 + w]), i


def test_sp_copy_blocks_strided(dev):
    """EXACT: dst[b*d_blk + r*d_row + c] = src[b*s_blk + r*s_row + c], written out with explicit indices; the rest of dst keeps its bits"""
    from wan.backend import ops
    blocks, rows, width = 3, 5, 16
    s_blk, s_row, d_blk, d_row = 24, 200, 400, 40          # src: blocks interleaved inside a row; dst: rows 40 apart, blocks 400 apart
    src = bits16((rows * s_row,), start=77)
    dst = sentinel16((blocks * d_blk,), dev)
    ops.sp_copy_blocks(src.to(dev), s_blk, s_row, dst, d_blk, d_row, blocks, rows, width)
    ref = torch.full((blocks * d_blk,), FILL16, dtype=torch.int16)
    s16 = src.view(torch.int16)
    for b in range(blocks):
        for r in range(rows):
            for c in range(width):
                ref[b * d_blk + r * d_row + c] = s16[b * s_blk + r * s_row + c]
    assert torch.equal(dst.cpu().view(torch.int16), ref)


@pytest.mark.parametrize('P,Lloc,nl', [(1, 37, 128), (2, 1, 8), (8, 37, 640), (4, 0, 128), (1, 13200, 640)])      # the last: more vectors than threads
def test_sp_copy_blocks_ulysses_round_trip(dev, P, Lloc, nl):
    """EXACT: the two calls of wan/distributed/ulysses.py (seq_to_head's send layout, head_to_seq's way back) against reshape / transpose"""
    from wan.backend import ops
    xb = bits16((Lloc, P * nl + 8), start=P + nl)
    x = xb.to(dev)[:, :P * nl]                                                           # row stride free, as seq_to_head documents
    send = sentinel16((P, Lloc, nl), dev)
    ops.sp_copy_blocks(x, nl, x.stride(0), send, Lloc * nl, nl, P, Lloc, nl)
    assert eq16(send, xb[:, :P * nl].reshape(Lloc, P, nl).transpose(0, 1))
    ob = sentinel16((Lloc, P * nl + 8), dev)
    out = ob[:, :P * nl]
    ops.sp_copy_blocks(send, Lloc * nl, nl, out, nl, out.stride(0), P, Lloc, nl)
    assert eq16(out, xb[:, :P * nl]) and holds16(ob[:, P * nl:])


# ------------------------------------------------------------------------------------------------
# argument checks: every misuse raises before anything is launched
# ------------------------------------------------------------------------------------------------
def test_rejects_sinusoid_embed(dev):
    from wan.backend import ops
    ob = torch.full((4, 12), FILL, device=dev)
    t = torch.tensor([1, 2, 3], device=dev)
    out = ob[:3, :6].contiguous().fill_(FILL)
    rejects(lambda: ops.sinusoid_embed(host(t), 6, out), out)                           # t on the host
    rejects(lambda: ops.sinusoid_embed(t.to(torch.int32), 6, out), out)                 # t of a dtype the kernel does not read
    rejects(lambda: ops.sinusoid_embed(torch.arange(6, device=dev)[::2], 6, out), out)  # t strided
    rejects(lambda: ops.sinusoid_embed(t, 6, host(out)))                                # out on the host
    rejects(lambda: ops.sinusoid_embed(t, 6, ob.double()[:3, :6].contiguous()))         # out fp64
    rejects(lambda: ops.sinusoid_embed(t, 6, ob[:3, :6]), ob)                           # out not contiguous
    rejects(lambda: ops.sinusoid_embed(t, 6, ob.view(-1)[:12]), ob)                     # out holds 2 rows for 3 timesteps
    rejects(lambda: ops.sinusoid_embed(t, 5, ob.view(-1)[:15]), ob)                     # odd dim


def test_rejects_gemv(dev):
    from wan.backend import ops
    N, K = 3, 8
    wb, xb, yb, bb = (torch.full(s, FILL, device=dev) for s in ((N + 1, K + 4), (K + 4,), (N + 2,), (N + 2,)))
    w, x, y, b = wb.view(-1)[:N * K].view(N, K), xb[:K], yb[:N], bb[:N]
    ops.gemv(w, b, x, y)                                                                # the valid call, so that the parents below prove something
    assert bool((yb[N:] == FILL).all()) and not bool((y == FILL).any())
    y.fill_(FILL)
    rejects(lambda: ops.gemv(host(w), b, x, y), yb)                                     # w on the host
    rejects(lambda: ops.gemv(w.to(torch.int32), b, x, y), yb)                           # w dtype
    rejects(lambda: ops.gemv(w, b.to(torch.int32), x, y), yb)                           # bias dtype
    rejects(lambda: ops.gemv(wb[:N, :K], b, x, y), yb)                                  # w.stride(0) != K
    rejects(lambda: ops.gemv(w, b, xb[:K - 4], y), yb)                                  # x.numel() != K
    rejects(lambda: ops.gemv(w, b, xb[:K + 4], y), yb)
    rejects(lambda: ops.gemv(w, b, x, yb[:N - 1]), yb)                                  # y.numel() != N
    rejects(lambda: ops.gemv(w, b, x, yb[:N + 1]), yb)
    rejects(lambda: ops.gemv(w, bb[:N - 1], x, y), yb)                                  # bias.numel() != N
    rejects(lambda: ops.gemv(w, b, x, yb[::2][:N]), yb)                                 # y strided
    rejects(lambda: ops.gemv(wb.view(-1)[:N * 6].view(N, 6), b, xb[:6], y), yb)         # K = 6: not a multiple of 4


def test_rejects_add_rows(dev):
    from wan.backend import ops
    rows, dim, period = 6, 8, 3
    ab, bb, ob = (torch.full(s, FILL, device=dev) for s in ((rows + 1, dim + 4), (period + 1, dim + 4), (rows + 1, dim + 4)))
    a, b, out = (t.view(-1)[:r * dim].view(r, dim) for t, r in ((ab, rows), (bb, period), (ob, rows)))
    rejects(lambda: ops.add_rows(host(a), b, out, period), ob)                          # on the host
    rejects(lambda: ops.add_rows(a, b, host(out), period))
    rejects(lambda: ops.add_rows(a.to(torch.int32), b, out, period), ob)                # dtypes (of the same width)
    rejects(lambda: ops.add_rows(a, b.to(torch.int32), out, period), ob)
    rejects(lambda: ops.add_rows(a, b, out.to(torch.int32), period))
    rejects(lambda: ops.add_rows(ab[:rows, :dim], b, out, period), ob)                  # a, b, out not contiguous
    rejects(lambda: ops.add_rows(a, bb[:period, :dim], out, period), ob)
    rejects(lambda: ops.add_rows(a, b, ob[:rows, :dim], period), ob)
    rejects(lambda: ops.add_rows(a, b[:period - 1], out, period), ob)                   # b has fewer than `period` rows
    rejects(lambda: ops.add_rows(a, bb.view(-1)[:period * (dim - 1)].view(period, dim - 1), out, period), ob)      # b rows of another dim
    rejects(lambda: ops.add_rows(a, b, out[:rows - 1], period), ob)                     # out.shape != a.shape
    rejects(lambda: ops.add_rows(a, b, out.view(dim, rows), period), ob)
    rejects(lambda: ops.add_rows(a, b, out, 0), ob)


def test_rejects_head_gemm(dev):
    from wan.backend import ops
    M, N, K = 5, 4, 8
    xb, wb, ob, bb = (torch.full(s, FILL, device=dev) for s in ((M + 1, K + 4), (66, K + 4), (M + 1, 66), (N + 2,)))
    x, w, out, b = xb[:M, :K], wb.view(-1)[:N * K].view(N, K), ob.view(-1)[:M * N].view(M, N), bb[:N]
    rejects(lambda: ops.head_gemm(host(x), w, b, out), ob)                              # on the host
    rejects(lambda: ops.head_gemm(x.to(torch.int32), w, b, out), ob)                    # dtypes
    rejects(lambda: ops.head_gemm(x, w, b.to(torch.int32), out), ob)
    rejects(lambda: ops.head_gemm(x, wb[:N, :K], b, out), ob)                           # w.stride(0) != K
    rejects(lambda: ops.head_gemm(x, w, b, ob[:M, :N]), ob)                             # out.stride(0) != N: the kernel would write m*N + n
    rejects(lambda: ops.head_gemm(x, w, b, out[:M - 1]), ob)                            # out.shape != (M, N)
    rejects(lambda: ops.head_gemm(x, w, b, out.view(N, M)), ob)
    rejects(lambda: ops.head_gemm(x, wb.view(-1)[:N * (K + 4)].view(N, K + 4), b, out), ob)      # w of another K
    rejects(lambda: ops.head_gemm(x, w, bb[:N - 1], out), ob)                           # bias.numel() != N
    rejects(lambda: ops.head_gemm(torch.full((K + 4, M + 1), FILL, device=dev).t()[:M, :K], w, b, out), ob)      # x with a strided innermost dimension
    rejects(lambda: ops.head_gemm(x, wb.view(-1)[:65 * K].view(65, K), None, ob.view(-1)[:M * 65].view(M, 65)), ob)      # N = 65


def test_rejects_patchify_unpatchify(dev):
    from wan.backend import ops
    C, F, H, W, ph, pw = 3, 2, 4, 6, 2, 3
    L, Kd = F * (H // ph) * (W // pw), C * ph * pw
    latb = torch.full((C + 1, F, H, W + 2), FILL, device=dev)
    lat = latb.view(-1)[:C * F * H * W].view(C, F, H, W)
    tb = sentinel16((L + 1, Kd + 8), dev)
    tok = tb[:L, :Kd]
    rejects(lambda: ops.patchify(host(lat), ph, pw, tok), tb)                           # on the host
    rejects(lambda: ops.patchify(lat.to(torch.int32), ph, pw, tok), tb)                 # dtypes
    rejects(lambda: ops.patchify(lat, ph, pw, tok.view(torch.int16)), tb)
    rejects(lambda: ops.patchify(latb[:C, :, :, :W], ph, pw, tok), tb)                  # a sliced latent would be read flat
    rejects(lambda: ops.patchify(lat, ph, pw, tb[:L - 1, :Kd]), tb)                     # out has too few rows
    rejects(lambda: ops.patchify(lat, ph, pw, tb[:L, :Kd - 1]), tb)                     # out has too few columns
    tt = sentinel16((Kd + 8, L + 1), dev)
    rejects(lambda: ops.patchify(lat, ph, pw, tt.t()[:L, :Kd]), tt)                     # out with a strided innermost dimension
    rejects(lambda: ops.patchify(lat.view(C, F, 3, 8), 2, 2, tb), tb)                   # H not divisible by ph
    rejects(lambda: ops.patchify(lat.view(C, F, 8, 3), 2, 2, tb), tb)                   # W not divisible by pw

    fb = torch.full((L + 1, Kd + 4), FILL, device=dev)
    ftok = fb[:L, :Kd]
    args = (C, F, H // ph, W // pw, ph, pw)
    rejects(lambda: ops.unpatchify(host(ftok), *args, lat), latb)                       # on the host
    rejects(lambda: ops.unpatchify(ftok.to(torch.int32), *args, lat), latb)             # dtype
    rejects(lambda: ops.unpatchify(fb[:L - 1, :Kd], *args, lat), latb)                  # tok has too few rows
    rejects(lambda: ops.unpatchify(fb[:L, :Kd - 1], *args, lat), latb)                  # tok has too few columns
    rejects(lambda: ops.unpatchify(ftok, *args, latb[:C, :, :, :W]), latb)              # a sliced latent would be written flat
    rejects(lambda: ops.unpatchify(ftok, *args, lat[:C - 1]), latb)                     # lat too small for (C, F, Hg, Wg, ph, pw)
    rejects(lambda: ops.unpatchify(ftok, C, F, 0, W // pw, ph, pw, lat), latb)


def test_rejects_lincomb_cfg_combine(dev):
    from wan.backend import ops
    n = 24
    ob, xb = torch.full((4, n), FILL, device=dev), torch.full((4, n), FILL, device=dev)
    out, x = ob.view(-1)[:n], xb.view(-1)[:n]
    rejects(lambda: ops.lincomb(out, []), ob)                                           # no terms
    rejects(lambda: ops.lincomb(out, [(x, 1.0)] * 5), ob)                               # more than 4
    rejects(lambda: ops.lincomb(out, [(x, 1.0), (xb.view(-1)[:n - 1], 1.0)]), ob)       # a term of another size
    rejects(lambda: ops.lincomb(out, [(xb.view(-1)[:n + 1], 1.0)]), ob)
    rejects(lambda: ops.lincomb(out, [(x, 1.0), (None, 0.0)]), ob)                      # a term without a tensor
    rejects(lambda: ops.lincomb(out, [(xb[:, :6], 1.0)]), ob)                           # a sliced term would be read flat
    rejects(lambda: ops.lincomb(ob[:, :6], [(x, 1.0)]), ob)                             # a sliced out would be written flat
    rejects(lambda: ops.lincomb(out, [(x.to(torch.int32), 1.0)]), ob)                   # dtypes
    rejects(lambda: ops.lincomb(out.to(torch.int32), [(x, 1.0)]))
    rejects(lambda: ops.lincomb(host(out), [(x, 1.0)]))                                 # on the host
    rejects(lambda: ops.lincomb(out, [(host(x), 1.0)]), ob)

    rejects(lambda: ops.cfg_combine(out, x, xb.view(-1)[:n - 1], 5.0), ob)              # sizes differ
    rejects(lambda: ops.cfg_combine(out, xb.view(-1)[:n + 1], x, 5.0), ob)
    rejects(lambda: ops.cfg_combine(ob.view(-1)[:n - 1], x, x, 5.0), ob)
    rejects(lambda: ops.cfg_combine(ob[:, :6], x, x, 5.0), ob)                          # sliced tensors
    rejects(lambda: ops.cfg_combine(out, xb[:, :6], x, 5.0), ob)
    rejects(lambda: ops.cfg_combine(out, x, xb[:, :6], 5.0), ob)
    rejects(lambda: ops.cfg_combine(out.to(torch.int32), x, x, 5.0))                    # dtypes
    rejects(lambda: ops.cfg_combine(out, x.to(torch.int32), x, 5.0), ob)
    rejects(lambda: ops.cfg_combine(host(out), x, x, 5.0))                              # on the host
    rejects(lambda: ops.cfg_combine(out, x, host(x), 5.0), ob)


def test_rejects_embed_rows(dev):
    from wan.backend import ops
    vocab, dim, n = 10, 16, 4
    tab = bits16((vocab, dim)).to(dev)
    ids = torch.tensor([0, 9, 3, 3], device=dev)
    ob = sentinel16((n + 1, dim + 8), dev)
    out = ob.view(-1)[:n * dim].view(n, dim)
    rejects(lambda: ops.embed_rows(host(tab), ids, out), ob)                            # on the host
    rejects(lambda: ops.embed_rows(tab, ids.to(torch.float64), out), ob)                # dtypes
    rejects(lambda: ops.embed_rows(tab.view(torch.int16), ids, out), ob)
    rejects(lambda: ops.embed_rows(tab, ids, out[:n - 1]), ob)                          # out.shape != (n, dim)
    rejects(lambda: ops.embed_rows(tab, ids, out.view(n * 2, dim // 2)), ob)
    rejects(lambda: ops.embed_rows(tab, ids, ob[:n, :dim]), ob)                         # a sliced out would be written flat
    rejects(lambda: ops.embed_rows(tab, torch.arange(8, device=dev)[::2], out), ob)     # strided ids
    rejects(lambda: ops.embed_rows(tab.view(-1)[:vocab * 12].view(vocab, 12), ids, ob.view(-1)[:n * 12].view(n, 12)), ob)      # dim not a multiple of 8


def test_rejects_sp_pack_unpack(dev):
    from wan.backend import ops
    P, Lloc, cpd, col0, w = 2, 5, 32, 8, 16
    fb = bits16((Lloc + 1, 3 * P * cpd + 8)).to(dev)
    q, k, v = (fb[:Lloc, i * P * cpd:(i + 1) * P * cpd] for i in range(3))
    sb = sentinel16((2 * P * Lloc * 3 * w + 64,), dev)
    send = sb[:P * Lloc * 3 * w]
    ops.sp_pack_qkv(q, k, v, P, cpd, col0, w, send)                                     # the valid call
    assert holds16(sb[P * Lloc * 3 * w:]) and not holds16(send)
    send.view(torch.int16).fill_(FILL16)
    rejects(lambda: ops.sp_pack_qkv(host(q), k, v, P, cpd, col0, w, send), sb)          # on the host
    rejects(lambda: ops.sp_pack_qkv(q, k.view(torch.int16), v, P, cpd, col0, w, send), sb)      # dtype
    rejects(lambda: ops.sp_pack_qkv(q, fb[:Lloc - 1, :P * cpd], v, P, cpd, col0, w, send), sb)  # k rows != Lloc
    rejects(lambda: ops.sp_pack_qkv(q, k, fb[:Lloc + 1, :P * cpd], P, cpd, col0, w, send), sb)  # v rows != Lloc
    for i in range(3):                                                                  # q, k or v narrower than P * cols_per_dest
        args = [q, k, v]
        args[i] = fb[:Lloc, :P * cpd - 8]
        rejects(lambda: ops.sp_pack_qkv(*args, P, cpd, col0, w, send), sb)
    rejects(lambda: ops.sp_pack_qkv(q, k, v, P, cpd, col0, w, sb[:P * Lloc * 3 * w - 8]), sb)   # send too small
    rejects(lambda: ops.sp_pack_qkv(q, k, v, P, cpd, col0, w, sb[:2 * P * Lloc * 3 * w:2]), sb)  # send strided
    rejects(lambda: ops.sp_pack_qkv(q, k, v, P, cpd, col0, 12, send), sb)               # w = 12
    rejects(lambda: ops.sp_pack_qkv(q, k, v, P, cpd, 3, w, send), sb)                   # odd col0
    rejects(lambda: ops.sp_pack_qkv(q, k, v, P, cpd, 24, w, send), sb)                  # col0 + w > cols_per_dest

    cps = cpd
    ob = sentinel16((Lloc + 1, P * cps + 8), dev)
    o = ob[:Lloc, :P * cps]
    rb = bits16((2 * P * Lloc * w + 64,)).to(dev)
    recv = rb[:P * Lloc * w].view(P, Lloc, w)
    rejects(lambda: ops.sp_unpack_o(host(recv), P, cps, col0, w, o), ob)                # on the host
    rejects(lambda: ops.sp_unpack_o(recv.view(torch.int16), P, cps, col0, w, o), ob)    # dtype
    rejects(lambda: ops.sp_unpack_o(recv, P, cps, col0, w, ob[:Lloc, :P * cps - 8]), ob)        # o narrower than P * cols_per_src
    rejects(lambda: ops.sp_unpack_o(rb[:P * Lloc * w - 8], P, cps, col0, w, o), ob)     # recv too small
    rejects(lambda: ops.sp_unpack_o(rb[:2 * P * Lloc * w:2].view(P, Lloc, w), P, cps, col0, w, o), ob)   # recv strided
    rejects(lambda: ops.sp_unpack_o(recv, P, cps, col0, 12, o), ob)                     # w = 12
    rejects(lambda: ops.sp_unpack_o(recv, P, cps, 3, w, o), ob)                         # odd col0
    rejects(lambda: ops.sp_unpack_o(recv, P, cps, 24, w, o), ob)                        # col0 + w > cols_per_src


def _own_storage(parent, first, numel):
    """a bf16 tensor over elements [first, first + numel) of `parent` whose storage IS that range (a storage slice aliases its parent's
    memory): past its end lies more of the parent, which the test owns — and which the wrapper has to refuse to address"""
    st = parent.untyped_storage()[2 * first:2 * (first + numel)]
    t = torch.empty(0, dtype=torch.bfloat16, device=parent.device).set_(st, 0, (numel,), (1,))
    assert t.untyped_storage().nbytes() == 2 * numel and t.data_ptr() == parent.data_ptr() + 2 * first
    return t


def test_rejects_sp_copy_blocks(dev):
    from wan.backend import ops
    blocks, rows, width = 2, 3, 16
    n = blocks * rows * width
    sp, dp = bits16((2 * n,)).to(dev), sentinel16((2 * n,), dev)
    src, dst = _own_storage(sp, 0, n), _own_storage(dp, 0, n)
    ops.sp_copy_blocks(src, rows * width, width, dst, rows * width, width, blocks, rows, width)          # the valid call fills dst exactly
    assert eq16(dp[:n], sp[:n]) and holds16(dp[n:])
    dp.view(torch.int16).fill_(FILL16)
    ok = (rows * width, width)
    rejects(lambda: ops.sp_copy_blocks(src, *ok, dst, rows * width, width + 8, blocks, rows, width), dp)         # dst: last row past the storage
    rejects(lambda: ops.sp_copy_blocks(src, *ok, dst, rows * width + 8, width, blocks, rows, width), dp)         # dst: last block past it
    rejects(lambda: ops.sp_copy_blocks(src, rows * width, width + 8, dst, *ok, blocks, rows, width), dp)         # src: the same two
    rejects(lambda: ops.sp_copy_blocks(src, rows * width + 8, width, dst, *ok, blocks, rows, width), dp)
    rejects(lambda: ops.sp_copy_blocks(src, *ok, dst, *ok, blocks + 1, rows, width), dp)                         # one block too many
    rejects(lambda: ops.sp_copy_blocks(src, *ok, dst, *ok, blocks, rows + 1, width), dp)                         # one row too many in the last block
    rejects(lambda: ops.sp_copy_blocks(src, *ok, dst[8:], *ok, blocks, rows, width), dp)                         # a view that starts 8 elements in
    rejects(lambda: ops.sp_copy_blocks(src, *ok, dst, -rows * width, width, blocks, rows, width), dp)            # negative strides
    rejects(lambda: ops.sp_copy_blocks(src, rows * 8, 8, dst, rows * 8, 8, blocks, rows, 12), dp)                # width = 12
    rejects(lambda: ops.sp_copy_blocks(host(src), *ok, dst, *ok, blocks, rows, width), dp)                       # on the host
    rejects(lambda: ops.sp_copy_blocks(src.view(torch.int16), *ok, dst, *ok, blocks, rows, width), dp)           # dtype
