"""GPU parity tests (-m gpu): the HIP path, called through the C-ABI, against
  (1) the oracle (oracle/*.py) on the same seeded inputs,
  (2) the committed golden vectors produced by the imported reference (tests/golden/*.npz),
  (3) size-independent properties at BASELINE.json's full sizes (L = 75 600, d = 5120).

Stated tolerances (floating-point path):
  fp32 kernels (VAE, head, schedulers, layout)            : <= 1e-4 of the tensor scale
  bf16-output kernels vs the bf16-emulating oracle          : <= 2 bf16 ulp-ish, 2e-2 of the scale
  whole DiT forward in bf16 mode vs fp32 reference output   : rel-L2 <= 2e-2 (north-star tolerance)
"""
import math

import numpy as np
import pytest
import torch

import weights as W

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.asarray(a))


def scale_err(a, b):
    a, b = a.detach().double().cpu(), T(b).double() if not torch.is_tensor(b) else b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), T(b).double() if not torch.is_tensor(b) else b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def test_native_library_is_loaded():
    """the test process must really be running the in-tree HIP library."""
    from wan.backend import lib
    lib.load()
    maps = open('/proc/self/maps').read()
    assert 'libmoviigen_hip.so' in maps


# ------------------------------------------------------------------------------------------------
# kernels through the C-ABI vs oracle functions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,dim', [(37, 5120), (5, 128), (300, 256), (0, 128)])
def test_ln_modulate(dev, rows, dim):
    from oracle import dit
    from wan.backend import ops
    x = W.randn((rows, dim), 1) * 3
    sc, sh = W.randn((dim,), 2), W.randn((dim,), 3)
    ref = dit.layernorm(x, 1e-6) * (1 + sc) + sh
    out = torch.empty(rows, dim, dtype=torch.float32, device=dev)
    ops.ln_modulate(x.to(dev), sc.to(dev), sh.to(dev), True, 1e-6, out)
    outb = torch.empty(rows, dim, dtype=torch.bfloat16, device=dev)
    ops.ln_modulate(x.to(dev), sc.to(dev), sh.to(dev), True, 1e-6, outb)
    if rows:
        assert scale_err(out, ref) < 1e-5
        assert scale_err(outb.float(), ref.bfloat16().float()) < 1e-2
    # norm3: affine weight/bias, no (1+)
    ref3 = dit.layernorm(x, 1e-6, sc, sh)
    ops.ln_modulate(x.to(dev), sc.to(dev), sh.to(dev), False, 1e-6, out)
    if rows:
        assert scale_err(out, ref3) < 1e-5


@pytest.mark.parametrize('dim,hd,grid,rows,pos0', [(5120, 128, (2, 5, 5), 60, 0), (5120, 128, (2, 5, 5), 25, 25),
                                                   (128, 32, (1, 4, 4), 16, 0), (256, 128, (2, 4, 6), 48, 0)])
def test_rmsnorm_rope(dev, dim, hd, grid, rows, pos0):
    from oracle import dit
    from wan.backend import ops
    from wan.modules.model import rope_cos_sin
    x = (W.randn((rows, dim), 4) * 2).bfloat16()
    w = 1 + 0.1 * W.randn((dim,), 5)
    n = dim // hd
    ref = dit.rope(dit.rmsnorm(x.float(), w, 1e-6, True).view(rows, n, hd), grid, dit.rope_table(hd), pos0)
    ref = ref.reshape(rows, dim).bfloat16().float()
    out = torch.empty(rows, dim, dtype=torch.bfloat16, device=dev)
    ops.rmsnorm_rope(x.to(dev), w.to(dev), 1e-6, hd, out, rope_cos_sin(hd, grid).to(dev), grid, pos0)
    assert scale_err(out.float(), ref) < 1e-2
    # strided input (column slice of a fused qkv buffer) and no-rope variant (cross attention)
    wide = torch.zeros(rows, 3 * dim, dtype=torch.bfloat16, device=dev)
    wide[:, dim:2 * dim] = x.to(dev)
    ops.rmsnorm_rope(wide[:, dim:2 * dim], w.to(dev), 1e-6, hd, out)
    ref2 = dit.rmsnorm(x.float(), w, 1e-6, True).bfloat16().float()
    assert scale_err(out.float(), ref2) < 1e-2
    # out_scale: the factor enters the fp32 value before its one rounding to bf16
    ops.rmsnorm_rope(wide[:, dim:2 * dim], w.to(dev), 1e-6, hd, out, out_scale=0.1275174)
    ref3 = (dit.rmsnorm(x.float(), w, 1e-6, True) * 0.1275174).bfloat16().float()
    assert scale_err(out.float(), ref3) < 1e-2


@pytest.mark.parametrize('M,N,K', [(300, 256, 128), (129, 200, 192), (1, 64, 64), (1000, 1280, 1024), (77, 5120, 5120)])
@pytest.mark.parametrize('epi', [0, 1, 2, 3])
def test_gemm_epilogues(dev, M, N, K, epi):
    from oracle import dit
    from wan.backend import ops
    a = (W.randn((M, K), 6)).bfloat16()
    w = (W.randn((N, K), 7) * 0.05).bfloat16()
    b, g = W.randn((N,), 8), W.randn((N,), 9)
    y = dit.linear(a.float(), w.float(), b, True)  # bf16-rounded Linear output
    ad, wd, bd, gd = a.to(dev), w.to(dev), b.to(dev), g.to(dev)
    if epi == 0:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        ops.gemm(ad, wd, bd, epi, out)
        ref = y
    elif epi == 1:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        ops.gemm(ad, wd, bd, epi, out)
        ref = torch.nn.functional.gelu(y, approximate='tanh').bfloat16().float()
    elif epi == 2:
        r0 = W.randn((M, N), 10)
        out = r0.to(dev).clone()
        ops.gemm(ad, wd, bd, epi, out, gate=gd)
        ref = r0 + y * g
    else:
        out = torch.empty(M, N, dtype=torch.float32, device=dev)
        ops.gemm(ad, wd, bd, epi, out)
        ref = y
    # one bf16 ulp of slack for accumulation-order differences at a rounding boundary
    assert scale_err(out.float(), ref) < 1.2e-2


@pytest.mark.parametrize('M,N,K', [(700, 520, 256), (257, 132, 64), (1030, 1284, 640), (4200, 4100, 128), (9000, 2304, 64),
                                   (2100, 8448, 128), (4200, 4100, 8256)])
def test_gemm_tile_variants_agree(dev, M, N, K):
    """the tile schedules (128x128, 256x128, 256x256 with one wave per SIMD: one tile per workgroup, and the persistent
    tile loop — the last three shapes have more tiles than CUs, so its workgroups iterate: two with < 32 tile columns = the
    chip-wide 8x32 super-tile raster of variant 8, incl. a partial band, one with 33 = the per-XCD band raster, one narrow with
    K > 8192 = the 16x16 super-tile raster —, variant 11 (one barrier per k-tile, generated schedule, rotated tail; K = 64 is its
    one-k-tile case, K = 8256 its second schedule) and the product's variant 12 (a stage refilled while it is consumed; K = 64 goes to
    the 256x128 kernel, K = 128 is its two-k-tile edge) give the same bits, ragged edges included — in the A/B library and in the
    PRODUCT library, which has no switch."""
    from wan.backend import lib, ops
    a = W.randn((M, K), 16).bfloat16().to(dev)
    w = (W.randn((N, K), 17) * 0.05).bfloat16().to(dev)
    b = W.randn((N,), 18).to(dev)
    outs = []

    def run():
        o = torch.full((M + 1, N), -7.0, dtype=torch.float32, device=dev)      # guard row: no write past M
        ops.gemm(a, w, b, ops.BIAS_F32, o[:M])
        assert (o[M] == -7.0).all()
        outs.append(o[:M].clone())
    run()                                   # the PRODUCT library (its own rule by shape: 12, else 2 / 1)
    with lib.ab_library() as h:             # the measurement partners live in the A/B library
        for v in (0, 1, 2, 7, 8, 11, 12):
            assert h.mg_gemm_set_variant(v) == 0
            run()
        assert h.mg_gemm_set_variant(9) != 0 and h.mg_gemm_set_variant(13) != 0       # unknown numbers are refused, not aliased
    assert all(torch.equal(outs[0], o) for o in outs[1:])


@pytest.mark.parametrize('M,N,K', [(1030, 1284, 640), (4200, 4100, 128), (9000, 2304, 64), (2100, 8448, 8256)])
@pytest.mark.parametrize('epi', [0, 1, 2, 3])
def test_gemm_default_epilogues_match_direct_ones(dev, M, N, K, epi):
    """variants 11 and 12 (the product's kernel for M > 256, N > 128) share their own epilogues — bf16 outputs: W rows staged in a permuted order so that
    a lane stores 8 consecutive features (16 bytes); fp32 outputs: the wave's block transposed through LDS and written as whole row
    segments, with the residual read the same way — against variant 8's direct epilogue: EVERY element, bit for bit, full and ragged
    blocks, one k-tile and both k-loop schedules, outputs with a row pitch > N, and a bf16 pitch that only allows 8-byte stores (the
    launcher's fallback)."""
    from wan.backend import lib, ops
    a = W.randn((M, K), 26).bfloat16().to(dev)
    w = (W.randn((N, K), 27) * 0.05).bfloat16().to(dev)
    b, g = W.randn((N,), 28).to(dev), W.randn((N,), 29).to(dev)
    f32 = epi >= 2
    for pitch in (N, N + 24, N + 4):
        r0 = W.randn((M + 1, pitch), 30).to(dev)
        outs = []

        def run():
            o = r0.clone() if f32 else r0.bfloat16()
            ops.gemm(a, w, b, epi, o[:M, :N], gate=g if epi == 2 else None)
            outs.append(o)
        with lib.ab_library() as h:
            for v in (8, 11, 12):
                h.mg_gemm_set_variant(v)
                run()
        run()                               # the product library
        ref = r0 if f32 else r0.bfloat16()
        for o in outs[1:]:
            assert torch.equal(outs[0], o), (pitch, (outs[0].float() - o.float()).abs().max().item())
            assert torch.equal(o[M], ref[M]) and torch.equal(o[:, N:], ref[:, N:])      # nothing outside [M, N]


def test_gemm_rejects_bad_shapes(dev):
    from wan.backend import lib, ops
    a = torch.zeros(8, 96, dtype=torch.bfloat16, device=dev)      # K % 64 != 0
    w = torch.zeros(8, 96, dtype=torch.bfloat16, device=dev)
    with pytest.raises(lib.MoviigenHipError):
        ops.gemm(a, w, None, 0, torch.zeros(8, 8, dtype=torch.bfloat16, device=dev))
    with pytest.raises(lib.MoviigenHipError):
        ops.gemm(a.cpu(), w, None, 0, torch.zeros(8, 8, dtype=torch.bfloat16, device=dev))


@pytest.mark.parametrize('Lq,Lk,heads,hd', [(300, 300, 2, 128), (700, 512, 3, 128), (64, 64, 1, 128), (1000, 77, 1, 128),
                                             (16, 16, 4, 32), (50, 37, 2, 64), (1, 1, 1, 128)])
def test_attention_vs_oracle(dev, Lq, Lk, heads, hd, attn_variant):
    from oracle import dit
    from wan.modules.attention import flash_attention
    q = (W.randn((1, Lq, heads, hd), 11) * 1.5).bfloat16()
    k = (W.randn((1, Lk, heads, hd), 12) * 1.5).bfloat16()
    v = W.randn((1, Lk, heads, hd), 13).bfloat16()
    ref = dit.attention(q[0].float(), k[0].float(), v[0].float(), Lk, True)
    out = flash_attention(q.to(dev), k.to(dev), v.to(dev))
    assert out.dtype == torch.bfloat16 and out.shape == q.shape
    assert scale_err(out[0].float(), ref) < 2e-2
    # k_lens masking (reference attention.py:71-79) and fp32 in -> fp32 out dtype contract
    if Lk > 8:
        kl = Lk - 5
        ref2 = dit.attention(q[0].float(), k[0].float(), v[0].float(), kl, True)
        out2 = flash_attention(q.float().to(dev), k.float().to(dev), v.float().to(dev), k_lens=torch.tensor([kl]))
        assert out2.dtype == torch.float32
        assert scale_err(out2[0], ref2) < 2e-2


@pytest.mark.parametrize('spikes', [(3, 4), (4, 6), (6, 9), (9, 14)], ids=['2^49_2^65', '2^65_2^98', '2^98_2^147', '2^147_2^229'])
def test_attention_rescale_branch(dev, attn_variant, spikes):
    """keys whose scores dwarf the rest of their row (cdna guide 5.4 rule 26: a data-dependent branch needs an input that
    forces it and a full independent reference).  m16 (row reference = the first key tile's maximum raised by 2^64, folded
    into the MFMA): spikes up to 2^147 above the first tile must come through the branch-free pipelined pass, 2^229 must
    flag its block, which is then repeated with swept row maxima — never the exact loop; w64 (reference = the row's
    first 32 keys): the spikes sit in tiles 4 and 7, far above the reference."""
    from oracle import dit
    from wan.backend import lib
    from wan.modules.attention import flash_attention
    Lq, Lk = 256, 640
    q = (W.randn((1, Lq, 1, 128), 14)).bfloat16()
    k = (W.randn((1, Lk, 1, 128), 15) * 0.2).bfloat16()
    v = W.randn((1, Lk, 1, 128), 16).bfloat16()
    k[0, 300] = (q[0, 7] * spikes[0]).clone()          # tile 4 spikes for query 7
    k[0, 500] = (q[0, 100] * spikes[1]).clone()        # tile 7 spikes for query 100
    ref = dit.attention(q[0].float(), k[0].float(), v[0].float(), Lk, True)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    out_product = flash_attention(q.to(dev), k.to(dev), v.to(dev))[0].float() if attn_variant == 0 else None
    with lib.ab_library() as h:             # the flag counter is a hook of the A/B build (the same kernel source)
        h.mg_attn_w64_flag_counter(cnt.data_ptr())
        out = flash_attention(q.to(dev), k.to(dev), v.to(dev))[0].float()
        torch.cuda.synchronize()
    if out_product is not None:
        assert torch.equal(out, out_product)       # the product library's kernel is that kernel
    assert scale_err(out, ref) < 2e-2
    # the spiked rows themselves (they are one-hot: the output row is the spiked key's value row)
    assert (out[7, 0].cpu() - v[0, 300, 0].float()).abs().max().item() < 2e-2
    assert (out[100, 0].cpu() - v[0, 500, 0].float()).abs().max().item() < 2e-2
    if attn_variant == 0:
        sc = 1.4426950408889634 / math.sqrt(128)
        qk = q[0, :, 0].float() @ k[0, :, 0].float().T * sc             # exponents (bits) of every score
        above = [(qk[r].max() - qk[r, :64].max()).item() for r in (7, 100)]     # the spike over the row's first-tile best
        assert all(abs(a - 154) > 4 for a in above), above                  # no case sits on the limit itself
        expect_flag = max(above) > 154          # reference = first-tile maximum + 64 bits, a row sum above 2^90 flags
        assert (cnt[0].item() > 0) == expect_flag, (above, cnt.tolist())
        assert cnt[1].item() == 0, cnt.tolist()     # finite scores never reach the exact loop


def test_attention_prescaled_q(dev, attn_variant):
    """the form WanModel.forward uses: RMS-norm + RoPE of q with out_scale = scale*log2(e), then
    mg_attn_fwd_bf16_hd128_prescaled — against the oracle's attention of the unscaled operands."""
    from oracle import dit
    from wan.backend import ops
    from wan.modules.model import rope_cos_sin
    L, N, hd = 700, 3, 128
    grid = (7, 10, 10)
    x = W.randn((L, N * hd), 31).bfloat16()
    kx = W.randn((L, N * hd), 32).bfloat16()
    v = W.randn((L, N * hd), 33).bfloat16()
    wq, wk = W.randn((N * hd,), 34) * 0.2 + 1.5, W.randn((N * hd,), 35) * 0.2 + 1.5     # peaky rows: |logit| up to ~20
    tabs = dit.rope_table(hd)
    qn = dit.rope(dit.rmsnorm(x.float(), wq, 1e-6, True).view(L, N, hd), grid, tabs).bfloat16().float()
    kn = dit.rope(dit.rmsnorm(kx.float(), wk, 1e-6, True).view(L, N, hd), grid, tabs).bfloat16().float()
    ref = dit.attention(qn, kn, v.float().view(L, N, hd), L, True).reshape(L, N * hd)
    rope = rope_cos_sin(hd, grid).to(dev)
    sc = 1 / math.sqrt(hd)
    outs = {}
    for prescaled in (False, True):
        qd, kd = torch.empty(L, N * hd, dtype=torch.bfloat16, device=dev), torch.empty(L, N * hd, dtype=torch.bfloat16, device=dev)
        ops.rmsnorm_rope(x.to(dev), wq.to(dev), 1e-6, hd, qd, rope, grid, 0, out_scale=sc * ops.ATTN_LOG2E if prescaled else 1.0)
        ops.rmsnorm_rope(kx.to(dev), wk.to(dev), 1e-6, hd, kd, rope, grid, 0)
        n_pk = ops.packed_kv_numel(L, N)
        kp, vp = torch.empty(n_pk, dtype=torch.bfloat16, device=dev), torch.empty(n_pk, dtype=torch.bfloat16, device=dev)
        ops.pack_kv(kd, v.to(dev), N, kp, vp)
        o = torch.empty(L, N * hd, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(N, L, dtype=torch.float32, device=dev)
        ops.attention_hd128_lse(qd, kp, vp, o, lse, L, N, sc, prescaled=prescaled)
        assert scale_err(o.float(), ref) < 2e-2, prescaled
        outs[prescaled] = (o.float().cpu(), lse.cpu())
    # the two forms differ by where q's one rounding to bf16 is taken: same tolerance class, and the SAME lse
    assert scale_err(outs[True][0], outs[False][0]) < 2e-2
    s = torch.einsum('qhd,khd->hqk', qn, kn) * sc
    assert (outs[True][1] - torch.logsumexp(s, -1)).abs().max().item() < 5e-2
    assert (outs[False][1] - torch.logsumexp(s, -1)).abs().max().item() < 5e-2


def test_attention_reserved_cus_same_bits(dev):
    """mg_attn_fwd_bf16_hd128_prescaled(..., reserve_cus): a persistent grid that leaves 8 / 64 CUs free (what a sequence-
    parallel layer may ask for while an exchange kernel is in flight) walks the same (head, query block) items on fewer
    workgroups — the result must be the same bits; a negative count is refused."""
    from wan.backend import lib, ops
    L, N = 20000, 4                                        # 79 query blocks x 4 heads = 316 items > 256 CUs: the persistent path
    gen = torch.Generator(device=dev).manual_seed(5)
    q = (torch.randn(L, N * 128, device=dev, generator=gen) * 0.3).bfloat16()
    k = torch.randn(L, N * 128, device=dev, generator=gen).bfloat16()
    v = torch.randn(L, N * 128, device=dev, generator=gen).bfloat16()
    n_pk = ops.packed_kv_numel(L, N)
    kp, vp = torch.empty(n_pk, dtype=torch.bfloat16, device=dev), torch.empty(n_pk, dtype=torch.bfloat16, device=dev)
    ops.pack_kv(k, v, N, kp, vp)
    outs = []
    for rs in (0, 8, 64):
        o = torch.zeros(L, N * 128, dtype=torch.bfloat16, device=dev)
        ops.attention_hd128(q, kp, vp, o, L, N, 1.0, prescaled=True, reserve_cus=rs)
        outs.append(o)
    assert torch.isfinite(outs[0].float()).all().item() and outs[0].float().abs().max().item() > 0
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    with pytest.raises(lib.MoviigenHipError):
        ops.attention_hd128(q, kp, vp, outs[0], L, N, 1.0, prescaled=True, reserve_cus=-1)


def test_attention_items_by_ticket(dev):
    """the persistent attention grid hands out its (head, query block) items by ticket from 32 rounds on (csrc/attn_hd128_m16.hip: the static
    per-XCD partition lost 2 % of the metric's launch to the slowest XCD).  Which workgroup computes an item must not show in the result: the same
    bits as the static partition (A/B library, debug bit 4); the {next ticket, workgroups done} pair a launch used is re-armed by its last
    workgroup — launch after launch on one stream, two launches in flight on two streams, a smaller grid (reserve_cus) — always the same bits."""
    from wan.backend import lib, ops
    L, N = 8192, 260                                       # 32 query blocks x 260 heads = 8320 items = 32.5 rounds of 256 workgroups
    gen = torch.Generator(device=dev).manual_seed(11)
    q = (torch.randn(L, N * 128, device=dev, generator=gen) * 0.3).bfloat16()
    k = torch.randn(L, N * 128, device=dev, generator=gen).bfloat16()
    v = torch.randn(L, N * 128, device=dev, generator=gen).bfloat16()
    n_pk = ops.packed_kv_numel(L, N)
    kp, vp = torch.empty(n_pk, dtype=torch.bfloat16, device=dev), torch.empty(n_pk, dtype=torch.bfloat16, device=dev)
    ops.pack_kv(k, v, N, kp, vp)

    def run(**kw):
        o = torch.zeros(L, N * 128, dtype=torch.bfloat16, device=dev)
        ops.attention_hd128(q, kp, vp, o, L, N, 1.0, prescaled=True, **kw)
        return o
    with lib.ab_library() as h:
        h.mg_attn_w64_debug(16)
        static = run()
        torch.cuda.synchronize()
    assert torch.isfinite(static.float()).all().item() and static.float().abs().max().item() > 0
    _attn_rows_check(q, k, v, static, [0, 255, 256, L - 1], [0, N - 1], math.log(2.0))      # pre-scaled entry: p = 2^(q.k)
    for _ in range(3):
        assert torch.equal(run(), static)
    assert torch.equal(run(reserve_cus=8), static)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    outs = []
    for _ in range(2):                                     # two rounds: the second finds the pairs the first round's launches left behind
        for st in streams:
            with torch.cuda.stream(st):
                outs.append(run())
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, static)
    # ABI 9: the pair lives in a CALLER-owned workspace (mg_attn_workspace_bytes() zeroed bytes); the library allocates nothing and
    # synchronises nothing on a launch path.  A launch leaves the workspace zeroed; NULL = the static partition.
    nbytes = int(lib.load().mg_attn_workspace_bytes())
    assert 8 <= nbytes <= 4096
    for st in [torch.cuda.current_stream()] + streams:
        assert int(ops.attention_workspace(dev, st).count_nonzero()) == 0
    assert torch.equal(run(workspace=None), static)
    mine = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    o = torch.zeros(L, N * 128, dtype=torch.bfloat16, device=dev)
    fresh = torch.cuda.Stream(device=dev)                  # a stream no TICKETED launch has run on (the runtime's own first-use
    with torch.cuda.stream(fresh):                         # allocations of a new stream — queue, signals, kernel-argument pool — are
        ops.attention_hd128(q[:256], kp, vp, o[:256], L, 4, 1.0, prescaled=True, workspace=None)   # made by this plain launch)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]                # hipMemGetInfo
    with torch.cuda.stream(fresh):
        ops.attention_hd128(q, kp, vp, o, L, N, 1.0, prescaled=True, workspace=mine)
    free1 = torch.cuda.mem_get_info(dev)[0]
    torch.cuda.synchronize()
    assert free1 == free0 and torch.equal(o, static) and int(mine.count_nonzero()) == 0
    # ... and the FIRST ticketed launch of a process/stream is capturable: capture it, replay it twice
    o.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.attention_hd128(q, kp, vp, o, L, N, 1.0, prescaled=True, workspace=mine)
    for _ in range(2):
        o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, static) and int(mine.count_nonzero()) == 0
    with pytest.raises(lib.MoviigenHipError):              # a misaligned workspace is refused, not used
        ops.attention_hd128(q, kp, vp, o, L, N, 1.0, prescaled=True, workspace=mine[4:])


@pytest.fixture(params=[0, 3], ids=['m16', 'w64'])
def attn_variant(request):
    """run a test on the product library's head-dim-128 kernel (m16) and, inside an A/B-library scope, on its measurement partner (w64)."""
    from wan.backend import lib
    if request.param == 0:
        yield 0
        return
    with lib.ab_library() as h:
        assert h.mg_attn_set_variant(request.param) == 0
        yield request.param


# (sinusoid_embed, unpatchify, cfg_combine and the other small fp32 / layout kernels: tests/test_small_kernels.py)


# ------------------------------------------------------------------------------------------------
# whole DiT forward: HIP engine vs golden (reference outputs) and vs the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,cfg', [('hd128', W.SMALL_DIT_HD128), ('tiny', W.TINY_DIT), ('tiny_pad', W.TINY_DIT)])
def test_dit_forward_vs_reference(dev, golden, tag, cfg):
    import wan
    from oracle import dit
    g = golden(f'g3_dit_{tag}')
    P = W.make_dit_params(cfg, 0)
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(P)
    m.to(dev)
    j = 0
    while f'ctx{j}' in g:
        lat, t, ctx = T(g['lat']), T(g[f't{j}']), T(g[f'ctx{j}'])
        out = m([lat.to(dev)], t=t.to(dev), context=[ctx.to(dev)], seq_len=int(g['seq_len']))[0]
        assert out.dtype == torch.float32 and tuple(out.shape) == tuple(lat.shape)
        # (a) reference fp32 output, stated bf16 tolerance
        assert rel_l2(out, g[f'out_fp32_{j}']) < 2e-2, (tag, j)
        # (b) reference under bf16 autocast (same rounding points) — tighter
        assert rel_l2(out, g[f'out_bf16_{j}']) < 1.2e-2, (tag, j)
        # (c) our bf16-emulating oracle on the same inputs
        orc = dit.dit_forward(P, cfg, lat, t, ctx, int(g['seq_len']), emulate_bf16=True)
        assert rel_l2(out, orc) < 1.2e-2, (tag, j)
        j += 1


def test_dit_full_width_vs_oracle(dev):
    """the REAL width (dim 5120, 40 heads x 128, ffn 13824, text 4096 -> 512 tokens), 2 layers, 512 video
    tokens: w64 attention, 256x256 GEMMs and the fp32 head against the bf16-emulating oracle on the CPU."""
    import wan
    from oracle import dit
    cfg = dict(model_type='t2v', patch_size=(1, 2, 2), text_len=512, in_dim=16, dim=5120, ffn_dim=13824, freq_dim=256,
               text_dim=4096, out_dim=16, num_heads=40, num_layers=2, eps=1e-6)
    P = W.make_dit_params(cfg, 3)
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(P)
    m.to(dev)
    lat = W.randn((16, 2, 32, 32), 21)                 # grid (2, 16, 16) = 512 tokens
    ctx = W.randn((77, 4096), 22)
    t = torch.tensor([417.0])
    out = m([lat.to(dev)], t=t.to(dev), context=[ctx.to(dev)], seq_len=512)[0]
    orc = dit.dit_forward(P, cfg, lat, t, ctx, 512, emulate_bf16=True)
    assert rel_l2(out, orc) < 1.2e-2
    ref32 = dit.dit_forward(P, cfg, lat, t, ctx, 512, emulate_bf16=False)
    assert rel_l2(out, ref32) < 2e-2                   # the stated bf16 tolerance against the fp32 algorithm


def test_dit_hd128_padded_seq_len(dev):
    """seq_len > the video's token count (reference model.py:534-538 pads x to seq_len and masks the padded keys,
    attention.py k_lens): the packed-tile attention path must mask them too — 48 valid tokens inside seq_len 200
    (1 key tile vs 4)."""
    import wan
    from oracle import dit
    cfg = W.SMALL_DIT_HD128
    P = W.make_dit_params(cfg, 0)
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(P)
    m.to(dev)
    lat, ctx, t = W.randn((16, 2, 8, 12), 20), W.randn((33, cfg['text_dim']), 30), torch.tensor([999])
    out = m([lat.to(dev)], t=t.to(dev), context=[ctx.to(dev)], seq_len=200)[0]
    ref = dit.dit_forward(P, cfg, lat, t, ctx, 200, emulate_bf16=True)
    assert rel_l2(out, ref) < 1.2e-2
    out48 = m([lat.to(dev)], t=t.to(dev), context=[ctx.to(dev)], seq_len=48)[0]
    assert rel_l2(out, out48) < 1e-6          # padding never changes the video tokens


def test_operator_seam_self_attention(dev):
    """operator seam (2) of the reference (text2video.py:97-100): block.self_attn is callable with
    WanSelfAttention.forward's arguments; a caller-installed replacement (types.MethodType) is really called by
    WanModel.forward; the reference's own usp_attn_forward / usp_dit_forward installation keeps the fused path."""
    import types
    import wan
    from oracle import dit
    from wan.distributed.xdit_context_parallel import usp_attn_forward, usp_dit_forward
    cfg = W.SMALL_DIT_HD128
    P = W.make_dit_params(cfg, 0)
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(P)
    m.to(dev)
    # (a) the stand-alone operator vs the oracle's restatement of model.py:127-156 (bf16 rounding model)
    L, grid, N, hd = 48, (2, 4, 6), cfg['num_heads'], cfg['dim'] // cfg['num_heads']
    x = W.randn((1, 60, cfg['dim']), 91)                      # 48 video tokens + 12 padded rows, k_lens masks them
    sa = 'blocks.1.self_attn.'
    got = m.blocks[1].self_attn(x.to(dev), torch.tensor([L]), torch.tensor([list(grid)]), m.freqs)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (1, 60, cfg['dim'])
    h = x[0]
    tabs = dit.rope_table(hd)
    q = dit.rmsnorm(dit.linear(h, P[sa + 'q.weight'], P[sa + 'q.bias'], True), P[sa + 'norm_q.weight'], 1e-6, True)
    k = dit.rmsnorm(dit.linear(h, P[sa + 'k.weight'], P[sa + 'k.bias'], True), P[sa + 'norm_k.weight'], 1e-6, True)
    v = dit.linear(h, P[sa + 'v.weight'], P[sa + 'v.bias'], True)
    a = dit.attention(dit.rope(q.view(60, N, hd), grid, tabs), dit.rope(k.view(60, N, hd), grid, tabs),
                      v.view(60, N, hd), L, True)
    ref = dit.linear(a.reshape(60, -1), P[sa + 'o.weight'], P[sa + 'o.bias'], True)
    assert scale_err(got[0, :L], ref[:L]) < 2e-2
    # (b) a caller-installed forward is honoured by the fused loop
    lat, ctx, t = W.randn((16, 2, 8, 12), 20).to(dev), W.randn((33, cfg['text_dim']), 30).to(dev), torch.tensor([999], device=dev)
    base = m([lat], t=t, context=[ctx], seq_len=48)[0].clone()
    calls = []

    def my_attn(self, x, seq_lens, grid_sizes, freqs):
        calls.append((tuple(x.shape), int(seq_lens[0]), tuple(grid_sizes[0].tolist()), tuple(freqs.shape)))
        return type(self).forward(self, x, seq_lens, grid_sizes, freqs)
    for blk in m.blocks:
        blk.self_attn.forward = types.MethodType(my_attn, blk.self_attn)
    out = m([lat], t=t, context=[ctx], seq_len=48)[0]
    assert len(calls) == cfg['num_layers'] and calls[0] == ((1, 48, cfg['dim']), 48, (2, 4, 6), (1024, hd // 2))
    assert rel_l2(out, base) < 1e-6
    # (c) the reference's installation sequence: fused path, same result, replacement NOT treated as foreign
    calls.clear()
    for blk in m.blocks:
        blk.self_attn.forward = types.MethodType(usp_attn_forward, blk.self_attn)
    m.forward = types.MethodType(usp_dit_forward, m)
    out = m([lat], t=t, context=[ctx], seq_len=48)[0]
    assert torch.equal(out, base) and not calls
    one = m.blocks[0].self_attn.forward(x.to(dev), torch.tensor([L]), torch.tensor([list(grid)]), m.freqs)
    assert tuple(one.shape) == (1, 60, cfg['dim'])


@pytest.mark.parametrize('cfg', [W.SMALL_DIT_HD128, W.TINY_DIT], ids=['hd128', 'hd32'])
def test_operator_seam_flash_attention(dev, cfg):
    """operator seam (1) of the reference: model.py:10 binds `flash_attention` by name and calls that
    module-level name for every self-attention (:146-151) and cross-attention (:176), so a replacement is installed by
    assigning `wan.modules.model.flash_attention`.  The same assignment here must be honoured: the bound function is
    called with the reference's arguments (q / k roped and UNSCALED, [1, L, N, hd]; k_lens; window_size) 2 x layers
    times per forward, its result is what the block uses, and un-binding restores the fused path bit for bit.  (One
    difference in the call: the engine never materialises the rows that pad a video to seq_len — the reference carries
    them through every block and drops them in unpatchify — so q / k / v hold the L valid tokens, k_lens == L.)"""
    import wan
    import wan.modules.model as wm
    from wan.modules.attention import flash_attention as engine_fa
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(W.make_dit_params(cfg, 0))
    m.to(dev)
    N, hd = cfg['num_heads'], cfg['dim'] // cfg['num_heads']
    lat, ctx, t = W.randn((16, 2, 8, 12), 20).to(dev), W.randn((29, cfg['text_dim']), 30).to(dev), torch.tensor([999], device=dev)
    base = m([lat], t=t, context=[ctx], seq_len=60)[0].clone()        # 48 video tokens inside seq_len 60: k_lens matters
    assert wm.flash_attention is engine_fa
    calls = []

    def my_fa(q, k, v, q_lens=None, k_lens=None, dropout_p=0., softmax_scale=None, q_scale=None, causal=False,
              window_size=(-1, -1), deterministic=False, dtype=torch.bfloat16, version=None):
        calls.append((tuple(q.shape), tuple(k.shape), tuple(v.shape), None if k_lens is None else int(k_lens[0]), tuple(window_size)))
        return engine_fa(q, k, v, q_lens=q_lens, k_lens=k_lens, softmax_scale=softmax_scale, window_size=window_size)
    wm.flash_attention = my_fa
    try:
        out = m([lat], t=t, context=[ctx], seq_len=60)[0].clone()
        assert len(calls) == 2 * cfg['num_layers']
        assert calls[0] == ((1, 48, N, hd), (1, 48, N, hd), (1, 48, N, hd), 48, (-1, -1))                # self-attention
        assert calls[1] == ((1, 48, N, hd), (1, cfg['text_len'], N, hd), (1, cfg['text_len'], N, hd), None, (-1, -1))   # cross
        # same operator underneath: equal up to where q's scale is folded in (before / after its rounding to bf16)
        assert rel_l2(out, base) < 1e-2
        # the function's result really is what the block uses
        wm.flash_attention = lambda q, k, v, **kw: torch.zeros_like(q)
        zero = m([lat], t=t, context=[ctx], seq_len=60)[0]
        assert rel_l2(zero, base) > 1e-2
    finally:
        wm.flash_attention = engine_fa
    again = m([lat], t=t, context=[ctx], seq_len=60)[0]
    assert torch.equal(again, base)


def test_gate_residual_kernel(dev):
    from wan.backend import ops
    x = W.randn((37, 256), 5).to(dev)
    y = W.randn((37, 256), 6).to(dev).bfloat16()
    g = W.randn((256,), 7).to(dev)
    ref = x + y.float() * g
    ops.gate_residual(x, y, g)
    assert torch.equal(x, ref)
    ops.gate_residual(x, y, None)
    assert torch.equal(x, ref + y.float())


def test_dit_context_cache_and_determinism(dev):
    import wan
    cfg = W.SMALL_DIT_HD128
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(W.make_dit_params(cfg, 0))
    m.to(dev)
    lat = W.randn((16, 2, 8, 12), 20).to(dev)
    c1, c2 = W.randn((33, 128), 30).to(dev), W.randn((9, 128), 31).to(dev)
    t = torch.tensor([700], device=dev)
    a1 = m([lat], t=t, context=[c1], seq_len=48)[0].clone()
    b1 = m([lat], t=t, context=[c2], seq_len=48)[0].clone()
    a2 = m([lat], t=t, context=[c1], seq_len=48)[0].clone()     # served from the prompt cache
    assert torch.equal(a1, a2) and not torch.equal(a1, b1)
    c1.mul_(2.0)                                                 # in-place edit must invalidate
    a3 = m([lat], t=t, context=[c1], seq_len=48)[0]
    assert not torch.equal(a1, a3)


def test_forward_pair_shares_block0_prefix_bit_equal(dev, monkeypatch):
    """WanModel.forward_pair = the two guidance branches of a step (reference text2video.py:237-240) with everything in front of block 0's
    cross-attention computed once: equal, bit for bit, to two plain forwards — in either order of the contexts, step after step (a stale
    prefix of the previous latent / t would show), with padding rows (seq_len > L), and it skips the launches it says it skips."""
    import wan
    from wan.backend import ops
    cfg = W.SMALL_DIT_HD128
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(W.make_dit_params(cfg, 0))
    m.to(dev)
    c1, c2 = W.randn((33, 128), 30).to(dev), W.randn((9, 128), 31).to(dev)
    calls = {'attn': 0}
    orig = ops.attention_hd128

    def counting(*a, **k):
        calls['attn'] += 1
        return orig(*a, **k)
    monkeypatch.setattr(ops, 'attention_hd128', counting)
    for step, (tv, seed, seq_len) in enumerate([(700, 20, 48), (310, 21, 48), (310, 22, 64)]):
        lat = W.randn((16, 2, 8, 12), seed).to(dev)
        t = torch.tensor([tv], device=dev)
        a = m([lat], t=t, context=[c1], seq_len=seq_len)[0].clone()
        b = m([lat], t=t, context=[c2], seq_len=seq_len)[0].clone()
        n0 = calls['attn']
        pa, pb = m.forward_pair([lat], t, [c1], [c2], seq_len)
        assert calls['attn'] - n0 == 4 * cfg['num_layers'] - 1, 'one self-attention launch fewer than two forwards'
        assert torch.equal(pa[0], a) and torch.equal(pb[0], b), step
        qb, qa = m.forward_pair([lat], t, [c2], [c1], seq_len)
        assert torch.equal(qa[0], a) and torch.equal(qb[0], b), step
    monkeypatch.setenv('MOVIIGEN_CFG_SHARED_PREFIX', '0')
    n0 = calls['attn']
    pa, pb = m.forward_pair([lat], t, [c1], [c2], seq_len)
    assert calls['attn'] - n0 == 4 * cfg['num_layers'] and torch.equal(pa[0], a) and torch.equal(pb[0], b)


@pytest.mark.parametrize('cfg', [W.SMALL_DIT_HD128, W.TINY_DIT], ids=['hd128', 'hd32'])
def test_dit_forward_launch_sequence(dev, monkeypatch, cfg):
    """The library entry points one WanModel.forward calls, in order, at 48 tokens: the literal sequence, so that a change of the
    Python that drives the kernels cannot add, drop or reorder a launch unnoticed (every launch of a block is paid 40 x 50 x 2 times
    per video).  Second forward of a prompt = prelude + num_layers x block + tail: 15 launches per block at head_dim 128, 14 at
    head_dim 32 (no K/V tile packing, the generic attention kernel).  The first forward of a new prompt adds the two text-embedding
    GEMMs once and, per block, the cross-attention k|v GEMM, k's RMS-norm and (head_dim 128) the packing of K/V into tiles."""
    import wan
    from wan.backend import lib
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(W.make_dit_params(cfg, 0))
    m.to(dev)
    lat, ctx, t = W.randn((16, 2, 8, 12), 20).to(dev), W.randn((29, cfg['text_dim']), 30).to(dev), torch.tensor([999], device=dev)
    names, real = [], lib.call
    monkeypatch.setattr(lib, 'call', lambda name, *args: (names.append(name), real(name, *args))[1])

    def forward():
        names.clear()
        m([lat], t=t, context=[ctx], seq_len=48)
        return list(names)
    first, second = forward(), forward()
    hd128 = cfg['dim'] // cfg['num_heads'] == 128
    ln, gemm, norm = 'mg_ln_modulate', 'mg_gemm_bf16', 'mg_rmsnorm_rope_bf16'
    attn = 'mg_attn_fwd_bf16_hd128_prescaled' if hd128 else 'mg_attn_fwd_bf16_generic'
    pack = ['mg_pack_kv_bf16'] if hd128 else []
    prelude = ['mg_patchify_bf16', gemm, 'mg_sinusoid_embed', 'mg_gemv_f32', 'mg_gemv_f32', 'mg_gemv_f32', 'mg_add_rows_f32',
               'mg_add_rows_f32']
    self_attn = [ln, gemm, norm, norm] + pack + [attn, gemm]
    cross_attn = [ln, gemm, norm, attn, gemm]
    ffn = [ln, gemm, gemm]
    tail = [ln, 'mg_head_gemm_f32', 'mg_unpatchify_f32']
    assert len(self_attn + cross_attn + ffn) == (15 if hd128 else 14)
    assert second == prelude + cfg['num_layers'] * (self_attn + cross_attn + ffn) + tail
    cross_kv = [gemm, norm] + pack                      # made when block i first meets the prompt, in front of its cross-attention
    assert first == prelude + [gemm, gemm] + cfg['num_layers'] * (self_attn + cross_kv + cross_attn + ffn) + tail


# ------------------------------------------------------------------------------------------------
# schedulers on the GPU (fused lincomb kernel) vs the reference trajectories
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,n,shift', [('unipc', 6, 3.0), ('unipc', 2, 5.0), ('dpm', 6, 3.0), ('dpm', 2, 5.0),
                                          ('unipc', 50, 5.0), ('dpm', 50, 5.0)])
def test_scheduler_gpu(dev, golden, name, n, shift):
    """(50, 5.0) = the production setting (text2video.py:114-124): timestep/sigma tables equal the reference's and all
    50 steps of its trajectory (g9_sampling50: order ramp-up, lower_order_final) are followed to 5e-6."""
    from wan.utils import (FlowDPMSolverMultistepScheduler, FlowUniPCMultistepScheduler, get_sampling_sigmas,
                           retrieve_timesteps)
    g = golden('g4_schedulers')
    g9 = golden('g9_sampling50')
    if name == 'unipc':
        s = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
        s.set_timesteps(n, device=dev, shift=shift)
        ts = s.timesteps
    else:
        s = FlowDPMSolverMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
        ts, _ = retrieve_timesteps(s, device=dev, sigmas=get_sampling_sigmas(n, shift))
    assert np.array_equal(ts.cpu().numpy(), g[f'{name}_t_{n}'])
    assert np.array_equal(s.sigmas.cpu().numpy(), g[f'{name}_sigma_{n}'])
    traj = g9[f'traj_{name}'] if n == 50 else g[f'traj_{name}_{n}']
    assert len(traj) == n
    lat = T(g['traj_x0']).to(dev)
    for i, t in enumerate(ts.tolist()):
        v = 0.5 * torch.tanh(lat) + 0.1 * math.sin(t / 100.0)
        lat = s.step(v, t, lat, return_dict=False)[0]
        assert scale_err(lat, traj[i]) < 5e-6, (name, i)


# ------------------------------------------------------------------------------------------------
# VAE decode (fp32-exact mode)
# ------------------------------------------------------------------------------------------------
def _cl(x):   # [1,C,T,H,W] -> channels-last [T,H,W,C]
    return x[0].permute(1, 2, 3, 0).contiguous()


def test_vae_conv_pieces(dev, golden):
    from wan.backend import ops
    g = golden('g5_vae_d8_t3')
    P = W.make_vae_params(8, 1)
    w = P['decoder.middle.0.residual.2.weight'].permute(0, 2, 3, 4, 1).contiguous().to(dev)
    b = P['decoder.middle.0.residual.2.bias'].to(dev)
    x, c = _cl(T(g['conv_x'])).to(dev), _cl(T(g['conv_cache'])).to(dev)
    for cache, key in ((None, 'conv_nocache'), (c, 'conv_cache2'), (c[-1:].contiguous(), 'conv_cache1')):
        out = torch.empty(*x.shape[:3], w.shape[0], dtype=torch.float32, device=dev)
        ops.vae_conv(x, w, b, out, 3, 3, 3, cache=cache)
        assert scale_err(out, _cl(T(g[key]))) < 1e-5, key


@pytest.mark.parametrize('dim,t', [(8, 3), (8, 5), (32, 2)])
def test_vae_decode_vs_reference(dev, golden, dim, t):
    import wan
    g = golden(f'g5_vae_d{dim}_t{t}')
    vae = wan.modules.WanVAE(state_dict=W.make_vae_params(dim, 1), device=dev)
    out = vae.decode([T(g['z']).to(dev)])[0]
    assert out.dtype == torch.float32 and tuple(out.shape) == g['video'].shape
    assert out.min() >= -1 and out.max() <= 1
    assert scale_err(out, g['video']) < 1e-4
    if t >= 3:   # chunking freedom: the default (4 latent frames per call), the reference's
        out2 = vae.model.decode(T(g['z']).to(dev), chunks=[1, t - 1])      # one-frame chunks and one big chunk agree
        assert scale_err(out2, g['video']) < 1e-4
        out1 = vae.model.decode(T(g['z']).to(dev), chunks=[1] * t)
        assert scale_err(out1, g['video']) < 1e-4 and torch.equal(out1, out2) and torch.equal(out1, out)


def test_vae_modules_vs_oracle(dev, golden):
    """AttentionBlock and Resample pieces against the reference's module outputs."""
    import wan
    from wan.modules.vae import _Run
    g = golden('g5_vae_d8_t3')
    vae = wan.modules.WanVAE(state_dict=W.make_vae_params(8, 1), device=dev).model
    x = _cl(T(g['conv_x'])).to(dev)
    assert scale_err(vae._attn('decoder.middle.1.', x), _cl(T(g['attn']))) < 1e-5
    run = _Run()
    o1 = vae._res('decoder.middle.0.', x[:1], run)
    o2 = vae._res('decoder.middle.0.', x[1:], run)
    assert scale_err(torch.cat([o1, o2]), _cl(T(g['res_chunked']))) < 1e-5
    xu = _cl(T(g['up_x'])).to(dev)
    run = _Run()
    for i in range(3):
        o = vae._up('decoder.upsamples.3.', xu[i:i + 1], run)
        assert scale_err(o, _cl(T(g[f'up_c{i}']))) < 1e-5, i


@pytest.fixture(scope='module')
def vae_walk(dev):
    """the tiny decoder walked over all stages on two one-frame chunks [1,4,6,16] with one cache: the model, the chunks, the two
    outputs and the cache as it stood behind each chunk (the entries are never written in place: a shallow copy is a snapshot)."""
    import wan
    from wan.modules.vae import _Run
    m = wan.modules.WanVAE(state_dict=W.make_vae_params(8, 1), device=dev).model
    xs = [W.randn((1, 4, 6, 16), 51 + i).to(dev) for i in range(2)]
    run, outs, caches = _Run(), [], []
    for x in xs:
        outs.append(m._decoder_chunk(x, run))
        caches.append(dict(run.cache))
    return m, xs, outs, caches


@pytest.mark.gpu
def test_vae_cache_by_name(vae_walk):
    """what a decode leaves in its cache: one entry per cached convolution, under the convolution's name, in execution order; behind
    the first chunk one frame each and the first-chunk marker for every time_conv; behind a second one-frame chunk two frames each.  A
    time_conv that was fed ONE frame then (the first temporal up-sampler's) keeps [zero frame | that frame]: the zero frame stands in for
    the skipped first chunk.  The second up-sampler's is fed the TWO frames the first made of the chunk and keeps those, as the reference
    does (no frame is missing, nothing is padded)."""
    from wan.modules.vae import _REP, _Run
    m, xs, outs, (c1, c2) = vae_walk
    st = m._stages()
    names = [n for s in st for n in s[2]]
    tc = [n for n in names if n.endswith('time_conv')]
    assert len(tc) == 2 and list(c1) == names and list(c2) == names
    for n in names:
        if n in tc:
            assert c1[n] is _REP
        else:
            assert torch.is_tensor(c1[n]) and c1[n].shape[0] == 1, n
        assert torch.is_tensor(c2[n]) and c2[n].shape[0] == 2, n
    fed = []
    for n in tc:                                 # what the time_conv read in the second chunk: the stages in front of it, on the first chunk's cache
        run = _Run()
        run.cache.update(c1)
        xin = m._decoder_chunk(xs[1], run, 0, next(i for i, s in enumerate(st) if n in s[2]))
        fed.append(xin.shape[0])
        if xin.shape[0] == 1:
            assert not c2[n][0].any().item() and xin.any().item() and torch.equal(c2[n][1:], xin), n
        else:
            assert torch.equal(c2[n], xin[-2:]), n
    assert fed == [1, 2]
    assert tuple(outs[0].shape) == (1, 32, 48, 3) and tuple(outs[1].shape) == (4, 32, 48, 3)


@pytest.mark.gpu
def test_vae_cache_splits_at_a_stage_cut(vae_walk):
    """the property decode_pipelined relies on: stages [0, k) on one empty cache and [k, end) on another, fed the first part's output,
    give the bits of the uncut walk on both chunks, and the two caches hold disjoint names that together are all of them — at a cut
    in the middle of the list and on either side of the first temporal up-sampler."""
    from wan.modules.vae import _Run
    m, xs, outs, _ = vae_walk
    st = m._stages()
    names = {n for s in st for n in s[2]}
    up = next(i for i, s in enumerate(st) if s[2] and s[0] == 'up')
    for k in sorted({len(st) // 2, up, up + 1}):
        a, b = _Run(), _Run()
        for x, want in zip(xs, outs):
            y = m._decoder_chunk(m._decoder_chunk(x, a, 0, k), b, k)
            assert torch.equal(y, want), k
        assert a.cache and b.cache and not set(a.cache) & set(b.cache) and set(a.cache) | set(b.cache) == names, k
        assert set(a.cache) == {n for s in st[:k] for n in s[2]}, k


# ------------------------------------------------------------------------------------------------
# BASELINE.json configs[0] end to end through WanT2V.generate
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,C', [(3000, 32), (5001, 96), (700, 384), (14400, 384)])
def test_vae_attention_query_blocks(dev, L, C):
    """AttentionBlock arithmetic (vae.py:247-256) with more tokens than one 2048-row query block of the score
    workspace (and a ragged last block): fp32 single-head softmax attention vs an fp64 evaluation.  (14 400, 384) is the
    1280x720 decode's shape: its last block has 64 rows, so half of a 128-row tile lies past M while the channel offset
    runs to 14 400 floats — those rows must not be pointed at the 4 KB zero page.)"""
    from wan.backend import ops
    gen = torch.Generator(device=dev).manual_seed(L)
    frames = 1 if L > 10000 else 2
    qkv = torch.randn(frames, L, 3 * C, device=dev, generator=gen)
    out = torch.empty(frames, L, C, device=dev)
    ws = torch.empty(ops.vae_attn_workspace_floats(L, C), device=dev)
    assert ws.numel() <= (2048 + C) * (L + 3) + 8 * 2048 * C       # score block + V^T + the split-K partial sums of P.V
    ops.vae_attn(qkv, out, ws)
    q, k, v = qkv.double().split(C, dim=-1)
    ref = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(C), -1) @ v
    assert ((out.double() - ref).abs().max() / ref.abs().max()).item() < 1e-5


@pytest.mark.parametrize('solver', ['unipc', 'dpm++'])
def test_pipeline_cfg1(dev, golden, solver):
    import wan
    from wan.configs import Config
    g = golden('g6_pipeline_cfg1')
    cfg = W.TINY_DIT
    model = wan.modules.WanModel(**cfg)
    model.load_state_dict(W.make_dit_params(cfg, 0))
    vae = wan.modules.WanVAE(state_dict=W.make_vae_params(8, 1), device=dev)
    conf = Config(num_train_timesteps=1000, param_dtype=torch.bfloat16, vae_stride=(4, 8, 8), patch_size=(1, 2, 2),
                  sample_neg_prompt='', vae_checkpoint='', text_len=32)
    pipe = wan.WanT2V(conf, '', device_id=0, model=model, vae=vae)
    lats = []
    video = pipe.generate(T(g['ctx']), size=(64, 64), frame_num=1, shift=5.0, sample_solver=solver, sampling_steps=2,
                          guide_scale=5.0, n_prompt=T(g['ctx_null']), seed=0, offload_model=False,
                          noise=T(g['noise']), callback=lambda i, l: lats.append(l.clone()))
    # final latent vs the reference loop (fp32 reference; bf16 engine) and decoded video
    assert rel_l2(lats[-1], g[f'x0_{solver}']) < 2e-2
    assert tuple(video.shape) == (3, 1, 64, 64) and video.dtype == torch.float32
    if solver == 'unipc':
        assert rel_l2(video, g['video_unipc']) < 5e-2
    with pytest.raises(NotImplementedError):
        pipe.generate(T(g['ctx']), size=(64, 64), frame_num=1, sample_solver='euler', sampling_steps=2,
                      n_prompt=T(g['ctx_null']), noise=T(g['noise']))


# Stated end-to-end tolerances of the production sampling setting: rel-L2 of the latent against the
# reference's fp32 loop.  The reference's OWN bf16-autocast run drifts 4.4e-5 / 3.6e-4 / 8.3e-4 / 1.6e-3 / 2.6e-3 / 3.9e-3
# from its fp32 run at these steps (printed by make_golden_sampling50.py); the engine is allowed 1.65x that (measured,
# profiles/r06_pytest_sampling50.log: 4.4e-5 ... 4.0e-3 = the reference's own drift), and must stay within the
# reference's bf16 drift (+1e-4) of the reference's bf16 run itself (measured: half of it).
DRIFT_BOUND_50 = {1: 1e-4, 10: 6e-4, 20: 1.4e-3, 30: 2.6e-3, 40: 4.5e-3, 50: 6.5e-3}


@pytest.mark.parametrize('solver', ['unipc', 'dpm++'])
def test_pipeline_50_steps_drift(dev, golden, solver):
    """WanT2V.generate at the PRODUCTION sampling setting (50 steps, shift 5.0, guide 5.0; text2video.py:114-124,
    228-254) on the small head-dim-128 DiT: the bf16 engine's latents after steps 1, 10, 20, 30, 40, 50 against the
    imported reference's fp32 loop, and the decoded video against the reference's WanVAE_ decode of its final latent."""
    import wan
    from wan.configs import Config
    g = golden('g9_sampling50')
    cfg = W.SMALL_DIT_HD128
    model = wan.modules.WanModel(**cfg)
    model.load_state_dict(W.make_dit_params(cfg, 0))
    vae = wan.modules.WanVAE(state_dict=W.make_vae_params(8, 1), device=dev)
    conf = Config(num_train_timesteps=1000, param_dtype=torch.bfloat16, vae_stride=(4, 8, 8), patch_size=(1, 2, 2),
                  sample_neg_prompt='', vae_checkpoint='', text_len=cfg['text_len'])
    pipe = wan.WanT2V(conf, '', device_id=0, model=model, vae=vae)
    lats = []
    video = pipe.generate(T(g['ctx']), size=(96, 64), frame_num=5, shift=5.0, sample_solver=solver, sampling_steps=50,
                          guide_scale=5.0, n_prompt=T(g['ctx_null']), seed=0, offload_model=False,
                          noise=T(g['noise']), callback=lambda i, l: lats.append(l.clone()))
    assert len(lats) == 50
    keep = list(g['keep'])
    ref_bf16_drift = [rel_l2(T(g[f'lat_{solver}_bf16'][j]), g[f'lat_{solver}_fp32'][j]) for j in range(len(keep))]
    for j, step in enumerate(keep):
        e32 = rel_l2(lats[step - 1], g[f'lat_{solver}_fp32'][j])
        ebf = rel_l2(lats[step - 1], g[f'lat_{solver}_bf16'][j])
        print(f'{solver} step {step}: engine vs ref fp32 {e32:.2e}, vs ref bf16 {ebf:.2e}, ref bf16 vs fp32 '
              f'{ref_bf16_drift[j]:.2e}')
        assert e32 < DRIFT_BOUND_50[step], (solver, step, e32)
        assert ebf < ref_bf16_drift[j] + 1e-4, (solver, step, ebf)
    assert tuple(video.shape) == (3, 5, 64, 96) and video.dtype == torch.float32
    if solver == 'unipc':
        ev = rel_l2(video, g['video_unipc_fp32'])
        print(f'video rel-L2 {ev:.2e}')
        assert ev < 1.2e-2


# ------------------------------------------------------------------------------------------------
# size-independent properties at BASELINE.json configs[1] sizes (L = 75 600, 40 heads, d = 5120)
# ------------------------------------------------------------------------------------------------
def _attn_rows_check(q, k, v, o, rows, heads_to_check, sc, tol=2e-2):
    """sampled rows of o against fp32 softmax attention of the same bf16 operands, RELATIVE to the largest reference value
    (the outputs of near-uniform rows over 10^5 keys are ~0.02: an absolute bound would see nothing)."""
    for h in heads_to_check:
        qs = q[rows, h * 128:(h + 1) * 128].float()
        s_ = (qs @ k[:, h * 128:(h + 1) * 128].float().T) * sc
        ref = torch.softmax(s_, -1) @ v[:, h * 128:(h + 1) * 128].float()
        err = ((o[rows, h * 128:(h + 1) * 128].float() - ref).abs().max() / ref.abs().max()).item()
        assert err < tol, (h, err, ref.abs().max().item())


@pytest.mark.parametrize('variant', [0, 3], ids=['m16', 'w64'])
def test_fullsize_attention_properties(dev, variant):
    """both attention kernels at the full 720p size: near-uniform rows (N(0,1) operands) and peaky rows (q x 6: single
    keys dominate, logit sigma ~6)."""
    from wan.backend import lib, ops
    L, N = 75600, 40
    gen = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(L, N * 128, device=dev, generator=gen).bfloat16()
    k = torch.randn(L, N * 128, device=dev, generator=gen).bfloat16()
    v = torch.randn(L, N * 128, device=dev, generator=gen).bfloat16()
    n_pk = ops.packed_kv_numel(L, N)
    kpk = torch.empty(n_pk, dtype=torch.bfloat16, device=dev)
    vpk = torch.empty(n_pk, dtype=torch.bfloat16, device=dev)
    o = torch.empty(L, N * 128, dtype=torch.bfloat16, device=dev)
    sc = 1 / math.sqrt(128)
    import contextlib
    with (lib.ab_library() if variant else contextlib.nullcontext()):
        if variant:
            lib.load().mg_attn_set_variant(variant)
        # (1) rows of softmax sum to one: V = const  =>  O = const, for EVERY query and head
        ops.pack_kv(k, torch.full_like(v, 0.5), N, kpk, vpk)
        ops.attention_hd128(q, kpk, vpk, o, L, N, sc)
        assert (o.float() - 0.5).abs().max().item() < 4e-3
        # (2) permuting the keys (and values with them) does not change the output
        ops.pack_kv(k, v, N, kpk, vpk)
        ops.attention_hd128(q, kpk, vpk, o, L, N, sc)
        o1 = o.clone()
        perm = torch.randperm(L, device=dev, generator=gen)
        kp, vp = k[perm].contiguous(), v[perm].contiguous()
        ops.pack_kv(kp, vp, N, kpk, vpk)
        ops.attention_hd128(q, kpk, vpk, o, L, N, sc)
        assert ((o.float() - o1.float()).abs().max() / o1.float().abs().max()).item() < 5e-2
        # (3) sampled rows against fp32 attention of the GPU-resident data, relative tolerance
        rows = torch.tensor([0, 1, 255, 256, 40000, 75599], device=dev)
        _attn_rows_check(q, kp, vp, o, rows, (0, 17, 39), sc)
        # (4) peaky rows
        q6 = (q.float() * 6).bfloat16()
        ops.attention_hd128(q6, kpk, vpk, o, L, N, sc)
        _attn_rows_check(q6, kp, vp, o, rows, (0, 17, 39), sc)


def test_fullsize_gemm_properties(dev):
    from wan.backend import ops
    L, d, f = 75600, 5120, 13824
    gen = torch.Generator(device=dev).manual_seed(1)
    a = torch.randn(L, d, device=dev, generator=gen).bfloat16()
    w = (torch.randn(f, d, device=dev, generator=gen) * 0.02).bfloat16()
    out = torch.empty(L, f, dtype=torch.bfloat16, device=dev)
    ops.gemm(a, w, None, ops.BIAS_BF16, out)
    # sampled rows vs an fp32 matmul of the same bf16 operands
    rows = torch.tensor([0, 127, 128, 37777, 75599], device=dev)
    ref = a[rows].float() @ w.float().T
    assert ((out[rows].float() - ref).abs().max() / ref.abs().max()).item() < 1e-2
    # residual epilogue is an exact accumulate: x += y twice == x + 2y (fp32 adds of identical bf16 y)
    x = torch.zeros(L, d, dtype=torch.float32, device=dev)
    w2 = (torch.randn(d, d, device=dev, generator=gen) * 0.02).bfloat16()
    ops.gemm(a, w2, None, ops.GATE_RESID_F32, x)
    x1 = x.clone()
    ops.gemm(a, w2, None, ops.GATE_RESID_F32, x)
    assert torch.equal(x, 2 * x1)


# ------------------------------------------------------------------------------------------------
# BASELINE.json configs[2], [3], [4] at their sizes: per-rank attention / GEMM shapes of the Ulysses layouts
# (cfg3 in SURVEY numbering = 1920x832x81f, L = 131 040, SP=8: Ulysses ranks attend L x L x 5 heads, ring ranks 16 380 x L;
#  cfg4 = 1920x1056x81f, L = 166 320, SP=4: L x L x 10 heads / 41 580 x L), the single-GPU L = 131 040 launch
# of the metric's configuration, and the 1920x832x81f VAE decode.
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Lq,Lk,heads', [(131040, 131040, 1), (131040, 131040, 5), (166320, 166320, 2), (16380, 131040, 5), (41580, 166320, 10),
                                         (131040, 131040, 40)],
                         ids=['cfg1920x832_ulysses8_one_head_group', 'cfg1920x832_ulysses8_rank', 'cfg1920x1056_ulysses4_head_group', 'cfg1920x832_ring8_rank',
                              'cfg1920x1056_ring4_rank', 'cfg1920x832_single_gpu'])
def test_fullsize_attention_big_configs(dev, Lq, Lk, heads):
    """per-rank launch shapes at full size.  ULYSSES: after the seq->head exchange a rank attends ALL L queries against ALL
    L keys for its heads/P heads (xdit_context_parallel.py:185-190) — configs[2]: L = 131 040, 5 heads per rank, launched
    one head per pipeline group (wan/distributed/ulysses.py) and as one 5-head launch (MOVIIGEN_SP_GROUPS=1); configs[3]
    (CFG halves x Ulysses 4): L = 166 320, 10 heads per rank in 5 groups of 2.  RING (wan/distributed/ring.py): a rank
    keeps its L/P queries and all heads against a hop's keys — the (16 380 | 41 580) x L shapes.  Plus the single-GPU launch."""
    from wan.backend import ops
    gen = torch.Generator(device=dev).manual_seed(Lq % 97)
    q = torch.randn(Lq, heads * 128, device=dev, generator=gen).bfloat16()
    k = torch.randn(Lk, heads * 128, device=dev, generator=gen).bfloat16()
    v = torch.randn(Lk, heads * 128, device=dev, generator=gen).bfloat16()
    n_pk = ops.packed_kv_numel(Lk, heads)
    kpk = torch.empty(n_pk, dtype=torch.bfloat16, device=dev)
    vpk = torch.empty(n_pk, dtype=torch.bfloat16, device=dev)
    o = torch.empty(Lq, heads * 128, dtype=torch.bfloat16, device=dev)
    sc = 1 / math.sqrt(128)
    # (1) softmax rows sum to one for EVERY query row and head: V = const => O = const
    ops.pack_kv(k, torch.full_like(v, 0.5), heads, kpk, vpk)
    ops.attention_hd128(q, kpk, vpk, o, Lk, heads, sc)
    assert (o.float() - 0.5).abs().max().item() < 4e-3
    # (2) sampled rows (first / last / tile edges / middle) vs fp32 softmax attention of the same bf16 data, RELATIVE
    # to the largest reference value (near-uniform rows over 10^5 keys: |o| ~ 0.02)
    ops.pack_kv(k, v, heads, kpk, vpk)
    ops.attention_hd128(q, kpk, vpk, o, Lk, heads, sc)
    rows = torch.tensor([0, 1, 63, 64, 255, 256, Lq // 2, Lq - 257, Lq - 2, Lq - 1], device=dev)
    hs = sorted({0, heads // 2, heads - 1})
    _attn_rows_check(q, k, v, o, rows, hs, sc)
    # (3) peaky rows (q x 6: logit sigma ~6, single keys dominate), the pre-scaled entry on the same operands too
    q6 = (q.float() * 6).bfloat16()
    ops.attention_hd128(q6, kpk, vpk, o, Lk, heads, sc)
    _attn_rows_check(q6, k, v, o, rows, hs, sc)
    q6s = (q.float() * (6 * sc * ops.ATTN_LOG2E)).bfloat16()
    ops.attention_hd128(q6s, kpk, vpk, o, Lk, heads, sc, prescaled=True)
    _attn_rows_check(q6, k, v, o, rows, hs, sc, tol=3e-2)         # q6s is a second rounding of q6: one more bf16 error
    # (4) a ragged key count (last 64-key tile partly filled) at this size: the masked keys must not contribute
    lk2 = Lk - 4097
    ops.pack_kv(k[:lk2], v[:lk2], heads, kpk, vpk)
    ops.attention_hd128(q6, kpk, vpk, o, lk2, heads, sc)
    _attn_rows_check(q6, k[:lk2], v[:lk2], o, rows, hs, sc)


@pytest.mark.parametrize('M', [16380, 32760, 41580, 75600, 131040, 166320])
def test_fullsize_gemm_big_configs(dev, M):
    """the four GEMM shapes of a block at the per-rank / single-GPU token counts of configs[1], [2], [3]: 16 380 = L/8 (Ulysses 8),
    32 760 = L/4 (what `bench.py --gpus 8` runs: CFG halves x Ulysses 4), 41 580 = configs[3]'s L/4, 75 600 = 720p on one GPU,
    131 040 = 1080p on one GPU, 166 320 = `bench.py --workload 1056p --gpus 1` (N = 13 824 / 15 360: output element index past 2^31)."""
    from wan.backend import ops
    d, f = 5120, 13824
    gen = torch.Generator(device=dev).manual_seed(M % 89)
    rows = torch.tensor([0, 127, 128, 255, 256, M // 2, M - 129, M - 1], device=dev)
    for (N, K, epi) in ((3 * d, d, ops.BIAS_BF16), (f, d, ops.BIAS_GELU_BF16), (d, f, ops.GATE_RESID_F32), (d, d, ops.GATE_RESID_F32)):
        a = torch.randn(M, K, device=dev, generator=gen).bfloat16()
        w = (torch.randn(N, K, device=dev, generator=gen) * 0.02).bfloat16()
        bias = torch.randn(N, device=dev, generator=gen) * 0.1
        acc = a[rows].float() @ w.float().T + bias
        if epi == ops.GATE_RESID_F32:
            gate = torch.randn(N, device=dev, generator=gen)
            x0 = torch.randn(M, N, device=dev, generator=gen)
            x = x0.clone()
            ops.gemm(a, w, bias, epi, x, gate=gate)
            ref = x0[rows] + acc.bfloat16().float() * gate
            assert ((x[rows] - ref).abs().max() / ref.abs().max()).item() < 1e-2
            untouched = torch.tensor([1, M // 3, M - 2], device=dev)
            assert not torch.equal(x[untouched], x0[untouched])           # every row got its update
        else:
            out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
            ops.gemm(a, w, bias, epi, out)
            ref = torch.nn.functional.gelu(acc, approximate='tanh') if epi == ops.BIAS_GELU_BF16 else acc
            assert ((out[rows].float() - ref).abs().max() / ref.abs().max()).item() < 1e-2
        del a, w


def _rope_dev(x, grid, hd, pos0=0):
    """oracle.dit.rope (reference model.py:39-67) restated for DEVICE tensors: x [rows, N, hd] fp32, token index = pos0 + row, angles from
    oracle.dit.rope_table in fp64.  (The oracle's own function builds its index tensors on the host; this is the same arithmetic.)"""
    from oracle import dit
    f, h, w = grid
    ta, th, tw = [t.to(x.device) for t in dit.rope_table(hd)]
    idx = torch.arange(x.shape[0], device=x.device) + pos0
    fi, hi, wi = idx // (h * w), (idx // w) % h, idx % w
    ang = torch.cat([ta[fi], th[hi], tw[wi]], dim=-1)                      # [rows, hd/2] fp64
    xd = x.to(torch.float64).reshape(x.shape[0], x.shape[1], -1, 2)
    c, s_ = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
    a, b = xd[..., 0], xd[..., 1]
    return torch.stack([a * c - b * s_, a * s_ + b * c], dim=-1).flatten(2).to(torch.float32)


@pytest.mark.parametrize('grid', [(21, 52, 120), (21, 66, 120)], ids=['1080p', '1056p'])
def test_rmsnorm_rope_real_grids(dev, grid):
    """RoPE at the grids the bench runs: the (f, h, w) decomposition of token indices up to L - 1 and table rows up
    to w = 119 / h = 65 / f = 20, against oracle.dit.rope itself — slices of 64 rows at the start, across a frame boundary, across a row
    boundary and at the very end (pos0 = L - 64), and the device restatement used by the block test below against the oracle too."""
    from oracle import dit
    from wan.backend import ops
    from wan.modules.model import rope_cos_sin
    dim, hd = 5120, 128
    f, h, w = grid
    L = f * h * w
    tab = rope_cos_sin(hd, grid).to(dev)
    wt = 1 + 0.1 * W.randn((dim,), 5)
    for pos0 in (0, h * w - 32, 7 * h * w + 3 * w - 32, L // 2 + 17, L - 64):
        x = (W.randn((64, dim), 4 + pos0 % 7) * 2).bfloat16()
        ref = dit.rope(dit.rmsnorm(x.float(), wt, 1e-6, True).view(64, dim // hd, hd), grid, dit.rope_table(hd, max_len=1024), pos0)
        out = torch.empty(64, dim, dtype=torch.bfloat16, device=dev)
        ops.rmsnorm_rope(x.to(dev), wt.to(dev), 1e-6, hd, out, tab, grid, pos0)
        assert scale_err(out.float(), ref.reshape(64, dim).bfloat16().float()) < 1e-2, pos0
        mine = _rope_dev(dit.rmsnorm(x.float(), wt, 1e-6, True).view(64, dim // hd, hd).to(dev), grid, hd, pos0).cpu()
        assert (mine - ref).abs().max().item() < 1e-5, pos0


def test_fullsize_rowwise_kernels_past_2gib(dev):
    """mg_ln_modulate / mg_gate_residual_f32 / mg_rmsnorm_rope_bf16 on a buffer of L = 166 320 rows (the fp32 residual stream is 3.4 GB:
    byte offsets pass 2^31 at row 104 857 and 2^32 would be row 209 715): rows at the start, around the 2^31-byte boundary and the last
    64 against the oracle (the largest row count tested was 300)."""
    from oracle import dit
    from wan.backend import ops
    from wan.modules.model import rope_cos_sin
    L, d, hd, grid = 166320, 5120, 128, (21, 66, 120)
    gen = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(L, d, device=dev, generator=gen) * 2
    sc, sh = torch.randn(d, device=dev, generator=gen), torch.randn(d, device=dev, generator=gen)
    rows = torch.cat([torch.arange(0, 4), torch.arange(104855, 104861), torch.arange(L - 64, L)]).to(dev)
    hb = torch.empty(L, d, dtype=torch.bfloat16, device=dev)
    ops.ln_modulate(x, sc, sh, True, 1e-6, hb)
    ref = (dit.layernorm(x[rows].cpu(), 1e-6) * (1 + sc.cpu()) + sh.cpu()).bfloat16().float()
    assert scale_err(hb[rows].float(), ref) < 1e-2
    hf = torch.empty(L, d, dtype=torch.float32, device=dev)
    ops.ln_modulate(x, sc, sh, False, 1e-6, hf)
    assert scale_err(hf[rows], dit.layernorm(x[rows].cpu(), 1e-6, sc.cpu(), sh.cpu())) < 1e-5
    del hf
    # x += y * gate on every row, exact (one product, one sum per element, as torch's two kernels)
    y = torch.randn(L, d, device=dev, generator=gen).bfloat16()
    x0 = x[rows].clone()
    ops.gate_residual(x, y, sc)
    assert torch.equal(x[rows], x0 + y[rows].float() * sc)
    # RMS-norm + RoPE in place of q at the last rows of the 1056p grid
    wq = 1 + 0.1 * torch.randn(d, device=dev, generator=gen)
    out = torch.empty(L, d, dtype=torch.bfloat16, device=dev)
    ops.rmsnorm_rope(y, wq, 1e-6, hd, out, rope_cos_sin(hd, grid).to(dev), grid, 0)
    for r0 in (104855, L - 64):
        ref = dit.rope(dit.rmsnorm(y[r0:r0 + 6].float().cpu(), wq.cpu(), 1e-6, True).view(6, d // hd, hd), grid, dit.rope_table(hd), r0)
        assert scale_err(out[r0:r0 + 6].float(), ref.reshape(6, d).bfloat16().float()) < 1e-2, r0


def test_fullsize_block_composition_vs_fp32(dev):
    """ONE WanAttentionBlock at the metric's shape through the engine — L = 131 040 tokens of the (21, 52, 120) grid, d = 5120, 40 heads,
    ffn 13 824, 512 text keys: LN-modulate -> q|k|v GEMM -> RMS-norm + RoPE -> pack -> attention -> o-proj + gate -> cross-attention -> FFN —
    and, for 16 sampled token rows (first / last, 256-row tile edges, frame and grid-row boundaries), an fp32 torch evaluation IN THIS TEST
    of the same block from the block's own input (reference model.py:274-313; K / V of all tokens by torch matmuls on the GPU).  The pieces
    are checked at this size elsewhere; this is their composition.  Tolerance: the stated 2e-2 of the largest
    reference value, on the block's UPDATE (x_out - x_in: the residual stream itself would hide an error 30 times larger)."""
    import wan
    from oracle import dit
    from wan.backend import ops
    cfg = dict(model_type='t2v', patch_size=(1, 2, 2), text_len=512, in_dim=16, dim=5120, ffn_dim=13824, freq_dim=256, text_dim=4096,
               out_dim=16, num_heads=40, num_layers=1, eps=1e-6)
    grid, d, N, hd = (21, 52, 120), 5120, 40, 128
    L = grid[0] * grid[1] * grid[2]
    model = wan.modules.WanModel(**cfg, device=dev)
    model.init_weights(seed=3)
    model.eval().requires_grad_(False)
    gen = torch.Generator(device=dev).manual_seed(11)
    lat = torch.randn(16, 21, 104, 240, device=dev, generator=gen)
    ctx = torch.randn(512, 4096, device=dev, generator=gen).bfloat16()
    captured = {}
    orig = ops.ln_modulate

    def spy(x, *a, **k):
        if 'x_in' not in captured:
            captured['x_in'] = x.clone()                 # the block's input, exactly as the engine sees it
        return orig(x, *a, **k)
    ops.ln_modulate = spy
    try:
        model([lat], t=torch.tensor([500], device=dev), context=[ctx], seq_len=L)
    finally:
        ops.ln_modulate = orig
    ws = next(iter(model._ws.values()))
    x_in, x_out = captured['x_in'], ws['x']              # (the head reads x, it does not write it)
    assert x_in.shape == (L, d) and torch.isfinite(x_out).all().item()
    e = ws['mod'][:6].float()                            # blocks.0.modulation + e0, as the engine applied it
    ctx_emb = model._context(ctx)[1].float()             # the text embedding the engine's cross-attention used
    P = {k: v.float() for k, v in model.state_dict().items() if k.startswith('blocks.0.')}
    pre, sa, ca = 'blocks.0.', 'blocks.0.self_attn.', 'blocks.0.cross_attn.'
    rows = torch.tensor([0, 1, 119, 120, 255, 256, 6239, 6240, 6240 * 7 + 120 * 31 + 5, 65535, 65536, L // 2, L - 257, L - 256, L - 2, L - 1],
                        device=dev)
    lin = lambda x, n: dit.linear(x, P[n + '.weight'], P[n + '.bias'], False)
    # self-attention: K / V for ALL tokens (fp32 matmuls on the device), q and everything behind it for the sampled rows
    h = dit.layernorm(x_in, 1e-6) * (1 + e[1]) + e[0]
    k = _rope_dev(dit.rmsnorm(lin(h, sa + 'k'), P[sa + 'norm_k.weight'], 1e-6, False).view(L, N, hd), grid, hd)
    v = lin(h, sa + 'v').view(L, N, hd)
    qs = dit.rmsnorm(lin(h[rows], sa + 'q'), P[sa + 'norm_q.weight'], 1e-6, False).view(-1, N, hd)
    qs = torch.cat([_rope_dev(qs[i:i + 1], grid, hd, int(rows[i])) for i in range(rows.numel())])
    del h
    a = dit.attention(qs, k, v, L, False)                # [16, N, hd]: 16 x 131 040 scores per head
    del k, v
    x = x_in[rows] + lin(a.reshape(-1, d), sa + 'o') * e[2]
    # cross-attention over the 512 text keys
    hq = dit.layernorm(x, 1e-6, P[pre + 'norm3.weight'], P[pre + 'norm3.bias'])
    q = dit.rmsnorm(lin(hq, ca + 'q'), P[ca + 'norm_q.weight'], 1e-6, False)
    kc = dit.rmsnorm(lin(ctx_emb, ca + 'k'), P[ca + 'norm_k.weight'], 1e-6, False)
    vc = lin(ctx_emb, ca + 'v')
    a = dit.attention(q.view(-1, N, hd), kc.view(-1, N, hd), vc.view(-1, N, hd), kc.shape[0], False)
    x = x + lin(a.reshape(-1, d), ca + 'o')
    # ffn
    hf = dit.layernorm(x, 1e-6) * (1 + e[4]) + e[3]
    u = torch.nn.functional.gelu(lin(hf, pre + 'ffn.0'), approximate='tanh')
    ref = x + lin(u, pre + 'ffn.2') * e[5]
    upd_ref, upd = ref - x_in[rows], x_out[rows] - x_in[rows]
    err = ((upd - upd_ref).abs().max() / upd_ref.abs().max()).item()
    assert err < 2e-2, err
    # and no row of the 131 040 was skipped: the update is non-zero everywhere
    assert ((x_out - x_in).abs().amax(dim=1) > 0).all().item()


def _conv_ref_f64(x, cache, w, bias, pts, up2=False):
    """direct fp64 evaluation of the causal 3x3x3 / 3x3 convolution (reference vae.py:17-36; nearest-2x first when
    up2, vae.py:57-63) at sampled output voxels.  x [T,H,W,Ci], cache [Tc,H,W,Ci] or None, w [Co,kt,kh,kw,Ci]."""
    Co, kt, kh, kw, Ci = w.shape
    T, H, W, _ = x.shape
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    tc = 0 if cache is None else cache.shape[0]
    wd = w.double().cpu()
    out = []
    for (t, y, xx) in pts:
        acc = bias.double().cpu().clone()
        for a in range(kt):
            ts = t - (kt - 1) + a                       # causal: taps reach back in time only
            if ts < -tc:
                continue                                # zero left padding
            src = x[ts] if ts >= 0 else cache[tc + ts]
            for b in range(kh):
                for c in range(kw):
                    yy, xc = y + b - kh // 2, xx + c - kw // 2
                    if yy < 0 or yy >= Ho or xc < 0 or xc >= Wo:
                        continue
                    vec = src[yy // 2, xc // 2] if up2 else src[yy, xc]
                    acc += wd[:, a, b, c, :] @ vec.double().cpu()
        out.append(acc)
    return torch.stack(out)


@pytest.mark.parametrize('cin,cout,H,W,up2,kt', [(96, 96, 832, 1920, False, 3), (192, 192, 416, 960, False, 3),
                                                 (192, 96, 416, 960, True, 1), (96, 3, 832, 1920, False, 3)],
                         ids=['res96_832x1920', 'res192_416x960', 'up192to96_2x', 'head96to3'])
def test_fullsize_vae_conv_config5(dev, cin, cout, H, W, up2, kt):
    """the last decoder stages of the 1920x832 decode (BASELINE configs[4]) at their real spatial size: one frame
    with a 2-frame causal cache, sampled output voxels (corners, edges, interior) vs a direct fp64 evaluation."""
    from wan.backend import ops
    gen = torch.Generator(device=dev).manual_seed(cin + cout)
    x = torch.randn(1, H, W, cin, device=dev, generator=gen)
    cache = torch.randn(2, H, W, cin, device=dev, generator=gen) if kt == 3 else None
    w = torch.randn(cout, kt, 3, 3, cin, device=dev, generator=gen) / math.sqrt(kt * 9 * cin)
    b = torch.randn(cout, device=dev, generator=gen)
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    out = torch.empty(1, Ho, Wo, cout, device=dev)
    ops.vae_conv(x, w, b, out, kt, 3, 3, cache=cache, up2=up2)
    pts = [(0, 0, 0), (0, 0, Wo - 1), (0, Ho - 1, 0), (0, Ho - 1, Wo - 1), (0, 1, 1), (0, Ho // 2, Wo // 2),
           (0, Ho // 2 + 1, Wo - 1), (0, 255, 256), (0, Ho - 2, 63), (0, 17, Wo - 2)]
    ref = _conv_ref_f64(x, cache, w, b, pts, up2)
    got = torch.stack([out[t, y, xx] for (t, y, xx) in pts]).double().cpu()
    assert ((got - ref).abs().max() / ref.abs().max()).item() < 1e-5
    assert torch.isfinite(out).all().item()


@pytest.mark.parametrize('cin,cout,T,H,W,tc,up2', [(96, 96, 2, 40, 72, 2, False), (32, 192, 1, 33, 47, 0, False), (64, 128, 3, 24, 40, 1, False),
                                                  (192, 96, 2, 20, 36, 0, True), (16, 384, 1, 40, 64, 0, False), (40, 3, 2, 9, 11, 2, False)])
def test_vae_conv_shapes(dev, cin, cout, T, H, W, tc, up2):
    """the implicit-GEMM convolution with per-tap row pointers and the zero page for padding taps, on sampled voxels vs
    an fp64 evaluation: ragged M, Cin < 32 and Cin % 32 != 0 (zero-weight tail of a chunk), cache of 0 / 1 / 2 frames,
    the folded nearest-2x, Cout = 3 (head), bias + residual epilogue."""
    from wan.backend import ops
    gen = torch.Generator(device=dev).manual_seed(cin * 7 + cout)
    kt = 1 if up2 else 3
    x = torch.randn(T, H, W, cin, device=dev, generator=gen)
    cache = torch.randn(tc, H, W, cin, device=dev, generator=gen) if tc else None
    w = torch.randn(cout, kt, 3, 3, cin, device=dev, generator=gen) / math.sqrt(kt * 9 * cin)
    b = torch.randn(cout, device=dev, generator=gen)
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    res = torch.randn(T, Ho, Wo, cout, device=dev, generator=gen)
    out = torch.full((T, Ho, Wo, cout), float('nan'), device=dev)
    ops.vae_conv(x, w, b, out, kt, 3, 3, cache=cache, up2=up2, residual=res)
    assert torch.isfinite(out).all().item()                       # every output element written, nothing read from a NaN
    pts = [(0, 0, 0), (T - 1, Ho - 1, Wo - 1), (0, Ho - 1, 0), (T - 1, 0, Wo - 1), (T // 2, Ho // 2, Wo // 2), (0, 1, Wo - 2)]
    ref = _conv_ref_f64(x, cache, w, b, pts, up2) + torch.stack([res[t, y, xx] for (t, y, xx) in pts]).double().cpu()
    got = torch.stack([out[t, y, xx] for (t, y, xx) in pts]).double().cpu()
    assert ((got - ref).abs().max() / ref.abs().max()).item() < 1e-5


@pytest.mark.parametrize('cin,cout,T,H,W', [(8, 12, 2, 5, 7), (64, 96, 1, 16, 24), (192, 96, 3, 9, 11), (384, 192, 2, 13, 6), (20, 3, 1, 4, 4)])
def test_vae_upconv_phases(dev, cin, cout, T, H, W):
    """conv3x3(nearest-2x(x)) as four 2x2 phase convs with pre-summed taps (mg_vae_upconv_phases_f32, what WanVAE.decode
    runs) against the 3x3 conv that reads through the upsample (mg_vae_conv_f32 up2 = 1) — the whole output — and against
    an fp64 evaluation on sampled voxels incl. the four corners (zero padding of the UPSAMPLED image); the folded weights
    against their definition."""
    from wan.backend import ops
    gen = torch.Generator(device=dev).manual_seed(cin * 5 + cout)
    x = torch.randn(T, H, W, cin, device=dev, generator=gen)
    w = torch.randn(cout, 1, 3, 3, cin, device=dev, generator=gen) / math.sqrt(9 * cin)
    b = torch.randn(cout, device=dev, generator=gen)
    wp = ops.vae_upconv_fold_weights(w)
    w64 = w.double().cpu()[:, 0]                                    # [cout, 3, 3, cin]
    rows = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}                   # parity -> 3x3 taps behind each of the two image taps
    for py in (0, 1):
        for px in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    ref = sum(w64[:, yy, xx] for yy in rows[py][dy] for xx in rows[px][dx])
                    assert (wp[2 * py + px, :, dy, dx].double().cpu() - ref).abs().max().item() < 1e-6
    got = torch.full((T, 2 * H, 2 * W, cout), float('nan'), device=dev)
    ops.vae_upconv_phases(x, wp, b, got)
    assert torch.isfinite(got).all().item()                         # every output voxel of every phase written
    old = torch.empty(T, 2 * H, 2 * W, cout, device=dev)
    ops.vae_conv(x, w, b, old, 1, 3, 3, up2=True)
    assert ((got - old).abs().max() / old.abs().max()).item() < 1e-5
    Ho, Wo = 2 * H, 2 * W
    pts = [(0, 0, 0), (T - 1, Ho - 1, Wo - 1), (0, Ho - 1, 0), (T - 1, 0, Wo - 1), (T // 2, Ho // 2, Wo // 2), (0, 1, Wo - 2),
           (0, Ho - 2, 1)]
    ref = _conv_ref_f64(x, None, w, b, pts, True)
    sel = torch.stack([got[t, y, xx] for (t, y, xx) in pts]).double().cpu()
    assert ((sel - ref).abs().max() / ref.abs().max()).item() < 1e-5


@pytest.mark.parametrize('cin,cout,T,H,Wd,tc,phases', [(96, 96, 3, 37, 53, 2, False), (192, 192, 2, 30, 41, 1, False), (64, 384, 1, 19, 23, 0, False),
                                                        (192, 96, 2, 21, 33, 0, True)])
def test_vae_conv_voxel_tiles_agree(dev, cin, cout, T, H, Wd, tc, phases):
    """the 256-voxel workgroup tile of the wide exact convolutions (two 128-voxel sub-tiles sharing the staged weights;
    what the library picks for large launches) against the 128-voxel one: the same accumulation order per voxel, so
    the SAME BITS — with a ragged last tile (M not a multiple of 256), cache frames, residual, cout tails, and the four
    phase convolutions of an up-conv."""
    from wan.backend import ops
    gen = torch.Generator(device=dev).manual_seed(cin + cout)
    x = torch.randn(T, H, Wd, cin, device=dev, generator=gen)
    b = torch.randn(cout, device=dev, generator=gen)
    outs = []
    for flag in (1 << 8, 2 << 8, 0):
        if phases:
            wp = ops.vae_upconv_fold_weights(torch.randn(cout, 1, 3, 3, cin, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) / math.sqrt(9 * cin))
            outs.append(ops.vae_upconv_phases(x, wp, b, torch.full((T, 2 * H, 2 * Wd, cout), float('nan'), device=dev), mode=ops.VAE_EXACT | flag))
        else:
            w = torch.randn(cout, 3, 3, 3, cin, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) / math.sqrt(27 * cin)
            cache = torch.randn(tc, H, Wd, cin, device=dev, generator=torch.Generator(device=dev).manual_seed(4)) if tc else None
            res = torch.randn(T, H, Wd, cout, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
            o = torch.full((T, H, Wd, cout), float('nan'), device=dev)
            outs.append(ops.vae_conv(x, w, b, o, 3, 3, 3, cache=cache, residual=res, mode=ops.VAE_EXACT | flag))
    assert torch.isfinite(outs[0]).all().item()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_vae_fast_mode(dev, golden):
    """the opt-in split-bf16 x 3 mode of the VAE convolutions (mode = MG_VAE_BF16X3 of a conv call; WanVAE(mode='bf16x3'))
    against the exact mode: single convolutions (3x3x3 with cache and residual, channel tails, Cout = 3, the phase up-conv)
    to 1e-4 of the largest output, a whole small decode to 2e-3 absolute on [-1, 1] video values; the mode is an argument of
    each call (ABI 7), so decoders of both modes coexist; an unknown mode is refused."""
    import wan
    from wan.backend import lib, ops
    gen = torch.Generator(device=dev).manual_seed(11)
    for (cin, cout, Tn, H, Wd, tc) in [(96, 96, 3, 12, 20, 2), (384, 192, 2, 9, 7, 1), (20, 3, 2, 6, 6, 0), (192, 384, 1, 8, 8, 0)]:
        x = torch.randn(Tn, H, Wd, cin, device=dev, generator=gen)
        cache = torch.randn(tc, H, Wd, cin, device=dev, generator=gen) if tc else None
        w = torch.randn(cout, 3, 3, 3, cin, device=dev, generator=gen) / math.sqrt(27 * cin)
        b = torch.randn(cout, device=dev, generator=gen)
        res = torch.randn(Tn, H, Wd, cout, device=dev, generator=gen)
        outs = []
        for mode in (ops.VAE_EXACT, ops.VAE_BF16X3):
            o = torch.full((Tn, H, Wd, cout), float('nan'), device=dev)
            ops.vae_conv(x, w, b, o, 3, 3, 3, cache=cache, residual=res, mode=mode)
            outs.append(o)
        assert torch.isfinite(outs[1]).all().item()
        assert torch.equal(outs[0], outs[1]) == (cout <= 4)         # the fast kernel really ran (Cout <= 4 — the head — is exact in either mode)
        assert ((outs[0] - outs[1]).abs().max() / outs[0].abs().max()).item() < 1e-4
    x = torch.randn(2, 10, 14, 192, device=dev, generator=gen)
    wp = ops.vae_upconv_fold_weights(torch.randn(96, 1, 3, 3, 192, device=dev, generator=gen) / math.sqrt(9 * 192))
    b = torch.randn(96, device=dev, generator=gen)
    outs = []
    for mode in (ops.VAE_EXACT, ops.VAE_BF16X3):
        outs.append(ops.vae_upconv_phases(x, wp, b, torch.empty(2, 20, 28, 96, device=dev), mode=mode))
    assert ((outs[0] - outs[1]).abs().max() / outs[0].abs().max()).item() < 1e-4
    with pytest.raises(lib.MoviigenHipError):
        ops.vae_upconv_phases(x, wp, b, torch.empty(2, 20, 28, 96, device=dev), mode=2)
    P = W.make_vae_params(8, 1)
    z = torch.randn(16, 3, 8, 8, generator=torch.Generator().manual_seed(3)).to(dev)
    v_exact, v_fast = wan.modules.WanVAE(state_dict=P, device=dev), wan.modules.WanVAE(state_dict=P, device=dev, mode='bf16x3')
    exact = v_exact.model.decode(z)
    fast = v_fast.model.decode(z)
    again = v_exact.model.decode(z)
    assert torch.equal(exact, again) and torch.equal(fast, v_fast.model.decode(z))     # each decoder keeps its own arithmetic
    assert not torch.equal(exact, fast) and (exact - fast).abs().max().item() < 2e-3
    # against the reference's own outputs (the goldens of test_vae_decode_vs_reference), at the mode's stated tolerance
    for dim, t in ((8, 3), (32, 2)):
        g = golden(f'g5_vae_d{dim}_t{t}')
        out = wan.modules.WanVAE(state_dict=W.make_vae_params(dim, 1), device=dev, mode='bf16x3').decode([T(g['z']).to(dev)])[0]
        err = scale_err(out, g['video'])
        print(f'bf16x3 decode vs reference golden d{dim} t{t}: scale_err {err:.3e}')
        assert err < 1e-4          # measured 7.1e-5 (d8) / 4.3e-5 (d32): the same bound the exact mode is held to


def test_vae_conv_rejects_large_kernel_extents(dev):
    """the tile gather's per-tap validity masks hold extents up to 3: a 5x5 (or 5-frame) kernel is refused, not mis-computed."""
    from wan.backend import lib, ops
    x = torch.zeros(2, 8, 8, 32, device=dev)
    out = torch.empty(2, 8, 8, 32, device=dev)
    for (kt, kh, kw) in ((1, 5, 5), (5, 3, 3), (3, 3, 5)):
        w = torch.zeros(32, kt, kh, kw, 32, device=dev)
        with pytest.raises(lib.MoviigenHipError):
            ops.vae_conv(x, w, None, out, kt, kh, kw)


def test_fullsize_vae_decode_config5(dev):
    """BASELINE configs[4]: the 1920x832x81f decode (latent [16,21,104,240], seed 7) through WanVAE.decode:
    shape / finite / range, and two size-independent properties of the causal decoder — the first 17 output frames
    depend on the first 5 latent frames only (causality, vae.py:17-36), and the chunking of the latent frames is
    free — checked at the full spatial size."""
    import wan
    vae = wan.modules.WanVAE(state_dict=W.make_vae_params(96, 1), device=dev)
    z = torch.randn(16, 21, 104, 240, generator=torch.Generator().manual_seed(7)).to(dev)
    video = vae.decode([z])[0]
    assert video.shape == (3, 81, 832, 1920) and video.dtype == torch.float32
    assert torch.isfinite(video).all().item() and video.abs().max().item() <= 1.0
    assert video.std().item() > 1e-3
    head = vae.model.decode(z[:, :5].contiguous())
    assert torch.equal(head, video[:, :17])                       # causal, and the same launches -> bit-equal
    del video
    rechunk = vae.model.decode(z[:, :5].contiguous(), chunks=[1, 2, 2])
    assert (rechunk - head).abs().max().item() < 1e-5
    # the opt-in split-bf16 mode at a BASELINE size (its error was only bounded at dim 96 / 256 x 256): the first 17 frames
    # at 832 x 1920 against the exact decode of the same latent — 33 convolutions deep, every activation at full spatial size
    del rechunk
    fast = wan.modules.WanVAE(state_dict=W.make_vae_params(96, 1), device=dev, mode='bf16x3').model.decode(z[:, :5].contiguous())
    err = ((fast - head).abs().max() / head.abs().max()).item()
    rel = ((fast - head).norm() / head.norm()).item()
    print(f'bf16x3 vs exact at 832x1920x17f: max-abs / max {err:.3e}, rel-L2 {rel:.3e}')
    assert not torch.equal(fast, head) and err < 2e-4 and rel < 5e-5


def test_dit_depth40_vs_oracle(dev):
    """error growth over the real DEPTH: 40 layers (dim 1024, 8 heads x 128, ffn 2048, 512 tokens) against the
    bf16-emulating oracle and against the fp32 algorithm — the stated bf16 tolerance (rel-L2 <= 2e-2) must hold at
    40 layers, not only at 2 (the bf16 rounding model itself sits 4.7e-3 from fp32 here)."""
    import wan
    from oracle import dit
    cfg = dict(model_type='t2v', patch_size=(1, 2, 2), text_len=64, in_dim=16, dim=1024, ffn_dim=2048, freq_dim=256,
               text_dim=128, out_dim=16, num_heads=8, num_layers=40, eps=1e-6)
    P = W.make_dit_params(cfg, 5)
    m = wan.modules.WanModel(**cfg)
    m.load_state_dict(P)
    m.to(dev)
    lat = W.randn((16, 2, 32, 32), 21)
    ctx = W.randn((40, 128), 22)
    t = torch.tensor([417.0])
    out = m([lat.to(dev)], t=t.to(dev), context=[ctx.to(dev)], seq_len=512)[0]
    orc = dit.dit_forward(P, cfg, lat, t, ctx, 512, emulate_bf16=True)
    ref32 = dit.dit_forward(P, cfg, lat, t, ctx, 512, emulate_bf16=False)
    e_bf, e_32 = rel_l2(out, orc), rel_l2(out, ref32)
    print(f'depth-40 rel-L2: vs bf16 oracle {e_bf:.3e}, vs fp32 {e_32:.3e}')
    assert e_bf < 1.2e-2 and e_32 < 2e-2


def test_dit_real_width_and_depth_vs_oracle(dev):
    """the model's REAL width and REAL depth together (reference model.py:486-579 at the 14B configuration): dim 5120,
    40 heads x 128, ffn 13824, text 4096 -> 512 keys, 40 LAYERS, 1024 video tokens, against the oracle in both modes —
    the only check of the stated bf16 tolerance (rel-L2 <= 2e-2 vs the fp32 algorithm, <= 1.2e-2 vs the bf16 rounding
    model) at the shape whose rounding behaviour the bench number stands for.  The 40 blocks share ONE set of weights
    (same arithmetic and error growth per layer; 1.6 instead of 57 GB of fp32 host tensors): the engine gets the same
    tensors under all 40 block prefixes, the oracle reads them through a dict that maps blocks.i.* to blocks.0.*."""
    import wan
    from oracle import dit
    cfg1 = dict(model_type='t2v', patch_size=(1, 2, 2), text_len=512, in_dim=16, dim=5120, ffn_dim=13824, freq_dim=256,
                text_dim=4096, out_dim=16, num_heads=40, num_layers=1, eps=1e-6)
    cfg = dict(cfg1, num_layers=40)
    P1 = W.make_dit_params(cfg1, 7)

    class Shared(dict):
        def __missing__(self, key):
            if key.startswith('blocks.'):
                return self['blocks.0.' + key.split('.', 2)[2]]
            raise KeyError(key)
    full = {k: v for k, v in P1.items() if not k.startswith('blocks.')}
    for i in range(40):
        full.update({f'blocks.{i}.' + k[len('blocks.0.'):]: v for k, v in P1.items() if k.startswith('blocks.0.')})
    m = wan.modules.WanModel(**cfg, device=dev)         # parameters are born on the device: no 57 GB host copy
    m.load_state_dict(full)
    del full
    lat = W.randn((16, 4, 32, 32), 21)                  # grid (4, 16, 16) = 1024 tokens
    ctx = W.randn((100, 4096), 22)
    t = torch.tensor([417.0])
    out = m([lat.to(dev)], t=t.to(dev), context=[ctx.to(dev)], seq_len=1024)[0].cpu()
    del m
    torch.cuda.empty_cache()
    P40 = Shared(P1)
    orc = dit.dit_forward(P40, cfg, lat, t, ctx, 1024, emulate_bf16=True)
    ref32 = dit.dit_forward(P40, cfg, lat, t, ctx, 1024, emulate_bf16=False)
    e_bf, e_32, e_model = rel_l2(out, orc), rel_l2(out, ref32), rel_l2(orc, ref32)
    print(f'5120 x 40 layers, L=1024 rel-L2: vs bf16 oracle {e_bf:.3e}, vs fp32 {e_32:.3e} (the rounding model itself: {e_model:.3e})')
    assert torch.isfinite(out).all().item()
    assert e_bf < 1.2e-2 and e_32 < 2e-2


@pytest.mark.parametrize('mode', ['exact', 'bf16x3'])
def test_vae_decode_real_width_vs_oracle(dev, mode):
    """the REAL decoder width (dim 96: 384 / 192 / 96 channels, reference vae.py:544-568 with the shipped config
    :597-605): whole decode of z[16,3,32,32] -> [3,9,256,256] against oracle.vae.vae_decode, <= 1e-4 of the tensor scale
    in the exact mode AND in the opt-in split-bf16 mode (its stated bound is the same 1e-4)."""
    import wan
    from oracle import vae as ovae
    P = W.make_vae_params(96, 1)
    z = W.randn((16, 3, 32, 32), 61)
    kw = {} if mode == 'exact' else {'mode': mode}
    out = wan.modules.WanVAE(state_dict=P, device=dev, **kw).decode([z.to(dev)])[0].cpu()
    ref = ovae.vae_decode(P, z)
    assert tuple(out.shape) == (3, 9, 256, 256) and tuple(ref.shape) == (3, 9, 256, 256)
    err = scale_err(out, ref)
    print(f'dim-96 WanVAE decode [{mode}] vs oracle: scale_err {err:.3e}')
    assert err < 1e-4


def test_sequence_parallel_two_ranks_one_gpu():
    """Ulysses path end to end with world_size 2 (both ranks on cuda:0, gloo transport):
    sharded forward == unsharded forward, bit for bit."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                        '--master-addr', '127.0.0.1', '--master-port', '29551',
                        os.path.join(root, 'tests', 'dist_sp_worker.py')], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'SP_OK rank0' in r.stdout and 'SP_OK rank1' in r.stdout
    assert 'SP_ATTN_OP_OK rank0' in r.stdout and 'SP_ATTN_OP_OK rank1' in r.stdout
    assert 'SP_FSDP_OK rank0' in r.stdout and 'SP_FSDP_OK rank1' in r.stdout


@pytest.mark.parametrize('world', [2, 4])
def test_cfg_parallel_one_gpu(world):
    """cond / uncond halves (x Ulysses when world == 4): every rank gets the plain pair, bit for bit."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={world}',
                        '--master-addr', '127.0.0.1', '--master-port', str(29560 + world),
                        os.path.join(root, 'tests', 'dist_cfg_worker.py')], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for k in range(world):
        assert f'CFGP_OK rank{k}/{world}' in r.stdout


def _run_hybrid(world, backend, layout, port, transport='torch', model=None):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MOVIIGEN_TEST_BACKEND=backend, MOVIIGEN_TEST_LAYOUT=layout, HSA_ENABLE_IPC_MODE_LEGACY='0')
    if model:
        env['MOVIIGEN_TEST_MODEL'] = model
    env['MOVIIGEN_SP_TRANSPORT'] = 'torch'
    if transport != 'torch':            # rccl_direct: the C-ABI collectives on the library's own communicator
        env['MOVIIGEN_SP_TRANSPORT'] = transport        # (mg_sp_all_to_all, ...); peer_copy: one-sided copies into IPC-mapped buffers
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={world}',
                        '--master-addr', '127.0.0.1', '--master-port', str(port),
                        os.path.join(root, 'tests', 'dist_hybrid_worker.py')], capture_output=True, text=True, timeout=1500,
                       env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for k in range(world):
        assert f'HYBRID_OK {layout} {backend} rank{k}/{world}' in r.stdout, r.stdout[-2000:]
        if transport == 'peer_copy' and layout == 'sp_fsdp':      # the injected refused copy: every rank fell back and still got the right bits
            assert f'PEER_FALLBACK_OK rank{k}/{world}' in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize('world,layout', [(4, 'cfg_sp_fsdp'), (2, 'sp_fsdp'), (4, 'sp_fsdp')])
def test_config3_composition_one_gpu(world, layout):
    """BASELINE configs[3] composition: CFG-parallel halves x Ulysses x block shards over all ranks (4 gloo ranks on
    cuda:0 = 2 x Ulysses 2 x 4-way shards), and Ulysses over all ranks + shards; pipelined packed exchange at
    depth 1, 2 and default; bit-identical to the unsharded forwards."""
    _run_hybrid(world, 'gloo', layout, 29600 + world + (0 if layout == 'cfg_sp_fsdp' else 10))


@pytest.mark.parametrize('layout', ['sp_fsdp', 'cfg_sp_fsdp'], ids=['ulysses_sp8_fsdp8', 'cfg2_ulysses_sp4_fsdp8'])
def test_eight_rank_layouts_real_heads_one_gpu(layout):
    """the 8-rank layouts of BASELINE configs[2] / configs[3] instantiated with the model's REAL width and head count
    (dim 5120, 40 heads, ffn 13824; 2 layers, 256 tokens; 8 gloo ranks sharing cuda:0): `ulysses_sp8` = 5 heads per rank
    = five one-head pipeline groups (reference scripts/inference/generate.py:216-229, 40 % 8 == 0), and
    `cfg2 x ulysses_sp4 x fsdp8` = cond / uncond halves x Ulysses 4 (ten heads per rank in five 2-head groups) x block
    shards over all eight ranks (reference text2video.py:97-108) — both bit-identical to the unsharded forwards at
    pipeline depth 1, 2 and default."""
    _run_hybrid(8, 'gloo', layout, 29640 + (0 if layout == 'sp_fsdp' else 1), model='width40')


def test_peer_copy_transport_one_gpu():
    """MOVIIGEN_SP_TRANSPORT=peer_copy: the exchange as one-sided device copies into the peers' receive buffers (IPC
    handles exchanged once, hipMemcpyAsync D2D on the comm stream between two rendezvous).  Here: 2 ranks sharing
    cuda:0 (the handles cross a process boundary; the rendezvous is gloo's host barrier), Ulysses over both ranks +
    block shards, bit-identical to the unsharded forward at every pipeline depth."""
    _run_hybrid(2, 'gloo', 'sp_fsdp', 29671, 'peer_copy')


def test_peer_copy_transport_eight_ranks_real_heads_one_gpu():
    """the copy-engine transport at the REAL rank count: 8 processes sharing cuda:0 map each other's 10 receive
    buffers (IPC handles among 8 ranks, the pattern self-check, the ring order of the copies), 40 heads on 8 ranks = five one-head
    pipeline groups, Ulysses 8 + block shards — bit-identical to the unsharded forward at every pipeline depth."""
    _run_hybrid(8, 'gloo', 'sp_fsdp', 29673, 'peer_copy', model='width40')


@pytest.mark.parametrize('transport', ['auto', 'torch', 'rccl_direct', 'peer_copy'])
@pytest.mark.parametrize('layout', ['cfg_sp_fsdp', 'sp_fsdp'])
def test_rccl_multi_gpu(layout, transport):
    """the production transport with MORE than one rank: backend nccl (= RCCL over xGMI), one rank per visible GPU
    (2, 4 or 8), exchange on the communication stream overlapped with attention.  Skipped on a 1-GPU box."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip('needs >= 2 GPUs (RCCL refuses two ranks on one device)')
    world = 8 if n >= 8 else 4 if n >= 4 else 2
    _run_hybrid(world, 'nccl', layout, 29630 + world + {'torch': 0, 'rccl_direct': 20, 'peer_copy': 40, 'auto': 60}[transport], transport)


def test_emulation_tools_run():
    """the two one-GPU emulations DESIGN 4 quotes — `tools/emulate_rank.py` (one rank of a P-GPU DiT step on loop-back groups) and
    `tools/bench_vae.py --bands` (one rank of the W-band VAE decode) — still run against the engine as it is (small sizes: 2 layers, 720p;
    a 256 x 256 x 9f decode) and mark their lines as emulation."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'emulate_rank.py'), '--workload', '720p', '--layers', '2', '--ranks', '2', '8',
                        '--fsdp-at'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    em = [ln for ln in lines if 'invalid' in ln]
    assert {(ln['ranks'], ln['layout']) for ln in em} == {(2, 'ulysses_sp2'), (2, 'cfg2 x ulysses_sp1'), (8, 'ulysses_sp8'), (8, 'cfg2 x ulysses_sp4')}
    assert all(ln['compute_s_per_step'] > 0 and 'emulation' in ln['invalid'] for ln in em)
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'bench_vae.py'), '--size', '256x256', '--frames', '9', '--chunk', '4', '--bands', '2', '4'],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    bands = [ln for ln in lines if ln.get('metric') == 'vae_decode_band_rank_sec']
    assert [ln['ranks'] for ln in bands] == [2, 4] and all('emulation' in ln['invalid'] and ln['rank_seconds_measured'] > 0 for ln in bands)
    assert bands[1]['band_columns_latent'] == 8 and bands[1]['link_bytes_per_link']['kv_all_gather'] > 0


def test_train_side_sp_forward_one_gpu():
    """SURVEY 8(f) rank 4, second half: the training-side sequence-parallel DiT forward (reference
    scripts/train/model/model_seq.py) on the engine, 2 gloo ranks on cuda:0, vs the reference-generated golden g8
    (with and without padded rows) and bit-identical to the single-rank forward."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
                        '--master-addr', '127.0.0.1', '--master-port', '29655',
                        os.path.join(root, 'tests', 'dist_train_seq_worker.py')], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'TRAIN_SEQ_OK rank0/2' in r.stdout and 'TRAIN_SEQ_OK rank1/2' in r.stdout


def test_launcher_end_to_end(dev, tmp_path):
    """scripts/inference/generate.py on a tiny synthetic checkpoint directory (config.json + safetensors
    DiT + VAE .pth, prompt embeddings from a file): same video as driving WanT2V by hand."""
    import importlib.util
    import json
    import os
    from safetensors.torch import save_file
    import wan
    from wan.configs import SIZE_CONFIGS, SUPPORTED_SIZES, WAN_CONFIGS, Config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('mg_generate', os.path.join(root, 'scripts', 'inference', 'generate.py'))
    gen = importlib.util.module_from_spec(spec)
    ck = tmp_path / 'ckpt'
    ck.mkdir()
    cfg = W.TINY_DIT
    json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, open(ck / 'config.json', 'w'))
    save_file({k: (v.bfloat16() if v.dim() >= 2 and 'modulation' not in k else v).contiguous()
               for k, v in W.make_dit_params(cfg, 0).items()}, str(ck / 'diffusion_pytorch_model.safetensors'))
    torch.save(W.make_vae_params(8, 1), ck / 'Wan2.1_VAE.pth')
    torch.save({'prompt': W.randn((9, cfg['text_dim']), 50), 'negative': W.randn((5, cfg['text_dim']), 51)}, ck / 'emb.pt')
    tiny = Config(WAN_CONFIGS['t2v-14B'])
    tiny.update(text_len=cfg['text_len'], num_heads=cfg['num_heads'], sample_fps=16)
    WAN_CONFIGS['t2v-tiny'], SIZE_CONFIGS['64*64'], SUPPORTED_SIZES['t2v-tiny'] = tiny, (64, 64), ('64*64',)
    try:
        spec.loader.exec_module(gen)
        gen.EXAMPLE_PROMPT['t2v-tiny'] = {'prompt': 'x'}
        out = tmp_path / 'clip.mp4'
        args = gen.generate(gen._parse_args(['--task', 't2v-tiny', '--size', '64*64', '--frame_num', '5', '--ckpt_dir', str(ck),
                                             '--sample_steps', '2', '--base_seed', '3', '--prompt_embeds', str(ck / 'emb.pt'),
                                             '--save_file', str(out), '--offload_model', 'False']))
        assert args.saved_as is not None and os.path.exists(args.saved_as)
        pipe = wan.WanT2V(tiny, str(ck), device_id=0)
        emb = torch.load(ck / 'emb.pt')
        video = pipe.generate(emb['prompt'], size=(64, 64), frame_num=5, shift=5.0, sampling_steps=2, guide_scale=5.0,
                              n_prompt=emb['negative'], seed=3, offload_model=False)
        assert tuple(video.shape) == (3, 5, 64, 64)
        from wan.utils.utils import video_frames_uint8
        want = video_frames_uint8(video[None]).cpu().numpy()
        if args.saved_as.endswith('.npy'):
            assert np.array_equal(np.load(args.saved_as), want)
        else:                               # imageio absent: the hand-written container with one JPEG per frame (wan/utils/mp4_mjpeg.py)
            from wan.utils.mp4_mjpeg import read_mp4_mjpeg
            back = read_mp4_mjpeg(args.saved_as)
            assert back['frames'].shape == want.shape and back['fps'] == 16
            assert np.abs(back['frames'].astype(np.int32) - want.astype(np.int32)).mean() < 4.0
    finally:
        for d, k in ((WAN_CONFIGS, 't2v-tiny'), (SIZE_CONFIGS, '64*64'), (SUPPORTED_SIZES, 't2v-tiny')):
            d.pop(k, None)


def test_video_write_out(dev, tmp_path):
    """uint8 frames == the reference's cache_video arithmetic (utils.py:39-47), byte for byte."""
    import os
    from wan.utils.utils import cache_video, video_frames_uint8
    v = (W.randn((3, 5, 18, 34), 77) * 0.8)
    v[0, 0, 0, :4] = torch.tensor([1.0, -1.0, 1.7, -3.0])
    x = v.clamp(-1, 1)
    x = (x - (-1)) / max(1 - (-1), 1e-5)                       # torchvision make_grid(normalize=True, value_range)
    ref = (x.permute(1, 2, 3, 0) * 255).type(torch.uint8)
    got = video_frames_uint8(v.to(dev)[None])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, 18, 34, 3)
    assert torch.equal(got.cpu(), ref)
    path = cache_video(v.to(dev)[None], save_file=str(tmp_path / 'out.mp4'), fps=16)
    assert path is not None and os.path.exists(path)
    if path.endswith('.npy'):
        assert np.array_equal(np.load(path), ref.numpy())
    else:
        try:
            import imageio  # noqa: F401
        except ModuleNotFoundError:         # the fallback container: the frames come back (JPEG, quality 95) and the rate is the one asked for
            from wan.utils.mp4_mjpeg import read_mp4_mjpeg
            back = read_mp4_mjpeg(path)
            assert back['frames'].shape == tuple(ref.shape) and back['fps'] == 16 and back['object_type'] == 0x6C
            assert np.abs(back['frames'].astype(np.int32) - ref.numpy().astype(np.int32)).mean() < 6.0      # white noise: the worst case for JPEG
    other = cache_video(v.to(dev)[None], save_file=str(tmp_path / 'out.avi'))
    assert other is not None and os.path.exists(other)


def test_image_write_out(dev, tmp_path):
    """t2i result -> PNG: the reference's cache_image (utils.py:64-91 = torchvision save_image: x255, +0.5, clamp,
    uint8), byte for byte, and the file really holds those pixels."""
    from PIL import Image
    from wan.utils.utils import cache_image
    img = (W.randn((3, 1, 20, 36), 78) * 0.8)                    # generate() returns [3, 1, H, W] for t2i
    img[0, 0, 0, :4] = torch.tensor([1.0, -1.0, 1.7, -3.0])
    x = img.squeeze(1).clamp(-1, 1)
    x = (x - (-1)) / max(1 - (-1), 1e-5)
    ref = x.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)
    path = cache_image(tensor=img.to(dev).squeeze(1)[None], save_file=str(tmp_path / 'out.png'), nrow=1,
                       normalize=True, value_range=(-1, 1))
    assert path is not None and path.endswith('.png')
    assert np.array_equal(np.asarray(Image.open(path)), ref.numpy())


@pytest.mark.parametrize('world', [2, 3])
def test_vae_pipelined_one_gpu(world):
    """layer-pipelined multi-rank VAE decode == single-GPU decode, bit for bit (video on rank 0)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={world}',
                        '--master-addr', '127.0.0.1', '--master-port', str(29570 + world),
                        os.path.join(root, 'tests', 'dist_vae_worker.py')], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, MOVIIGEN_VAE_TEST='pipeline'))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for k in range(world):
        assert f'VAEPIPE_OK rank{k}/{world}' in r.stdout


@pytest.mark.parametrize('world', [2, 4, 8])
def test_vae_spatial_one_gpu(world):
    """W-band multi-rank VAE decode (WanVAE.decode_spatial; SURVEY 8(e): spatial bands with one halo pixel per convolution, reference decode
    vae.py:544-568 on rank 0 alone) == single-GPU decode, bit for bit, video on rank 0: 10 latent columns over 2 / 4 / 8 gloo ranks sharing
    cuda:0 = bands of 5+5, 3+3+2+2 (W not divisible), 2+2+1+1+1+1+1+1 (one-column bands), the default and the one-frame chunk lists, and a
    second geometry with 9 columns.  Halo exchange in front of every 3x3 convolution (caches keep their halos), k|v all-gather in the
    per-frame attention block, rank 0 assembles."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={world}',
                        '--master-addr', '127.0.0.1', '--master-port', str(29580 + world),
                        os.path.join(root, 'tests', 'dist_vae_worker.py')], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, MOVIIGEN_VAE_TEST='spatial'))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for k in range(world):
        assert f'VAESPATIAL_OK rank{k}/{world}' in r.stdout


@pytest.mark.parametrize('world', [2, 3, 4])
def test_ring_attention_one_gpu(world):
    """ring attention (operator and whole forward) vs one long softmax, head counts not divisible by the ring size."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={world}',
                        '--master-addr', '127.0.0.1', '--master-port', str(29580 + world),
                        os.path.join(root, 'tests', 'dist_ring_worker.py')], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for k in range(world):
        assert f'RING_OP_OK rank{k}/{world}' in r.stdout and f'RING_MODEL_OK rank{k}/{world}' in r.stdout
        assert world != 4 or f'HYBRID_OK rank{k}/{world}' in r.stdout
        # back on SpLayout.single() after each leg, the forward is the first one's again, bit for bit
        assert f'RING_RESET_OK rank{k}/{world}' in r.stdout and (world != 4 or f'HYBRID_RESET_OK rank{k}/{world}' in r.stdout)


def test_attention_lse_and_merge(dev):
    """mg_attn_fwd_bf16_hd128_lse (both kernels) and mg_attn_merge_f32 against fp32 math on one GPU."""
    from wan.backend import lib, ops
    heads, Lq = 2, 300
    for Lk in (200, 2300):                                   # two-level kernel / w64 kernel (Lk >= 2048)
        q = (W.randn((Lq, heads * 128), 71) * 1.2).bfloat16().to(dev)
        k = (W.randn((Lk, heads * 128), 72) * 1.2).bfloat16().to(dev)
        v = W.randn((Lk, heads * 128), 73).bfloat16().to(dev)
        n = ops.packed_kv_numel(Lk, heads)
        kp, vp = torch.empty(n, dtype=torch.bfloat16, device=dev), torch.empty(n, dtype=torch.bfloat16, device=dev)
        ops.pack_kv(k, v, heads, kp, vp)
        out = torch.empty(Lq, heads * 128, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(heads, Lq, dtype=torch.float32, device=dev)
        ops.attention_hd128_lse(q, kp, vp, out, lse, Lk, heads, 128 ** -0.5)
        s = (q.float().view(Lq, heads, 128).permute(1, 0, 2) @ k.float().view(Lk, heads, 128).permute(1, 2, 0)) * 128 ** -0.5
        assert (lse - torch.logsumexp(s, -1)).abs().max().item() < 2e-3, Lk
        ref = (torch.softmax(s, -1) @ v.float().view(Lk, heads, 128).permute(1, 0, 2)).permute(1, 0, 2).reshape(Lq, -1)
        assert scale_err(out.float(), ref) < 2e-2
    # merge of two halves == the whole
    h = Lk // 2 // 64 * 64
    parts = []
    for a, b in ((0, h), (h, Lk)):
        n = ops.packed_kv_numel(b - a, heads)
        kp, vp = torch.empty(n, dtype=torch.bfloat16, device=dev), torch.empty(n, dtype=torch.bfloat16, device=dev)
        ops.pack_kv(k[a:b], v[a:b], heads, kp, vp)
        o = torch.empty(Lq, heads * 128, dtype=torch.bfloat16, device=dev)
        l = torch.empty(heads, Lq, dtype=torch.float32, device=dev)
        ops.attention_hd128_lse(q, kp, vp, o, l, b - a, heads, 128 ** -0.5)
        parts.append((o, l))
    acc = torch.empty(Lq, heads * 128, dtype=torch.float32, device=dev)
    lacc = torch.empty(heads, Lq, dtype=torch.float32, device=dev)
    fin = torch.empty(Lq, heads * 128, dtype=torch.bfloat16, device=dev)
    ops.attention_merge(acc, lacc, parts[0][0], parts[0][1], heads, True)
    ops.attention_merge(acc, lacc, parts[1][0], parts[1][1], heads, False, out=fin)
    assert scale_err(fin.float(), ref) < 2e-2 and (lacc - torch.logsumexp(s, -1)).abs().max().item() < 2e-3
    with pytest.raises(lib.MoviigenHipError):
        ops.attention_hd128_lse(q, kp, vp, out, torch.empty(3, dtype=torch.float32, device=dev), Lk, heads, 1.0)


@pytest.mark.parametrize('world,extra,plain', [(2, ['--cfg-parallel'], False), (4, [], True), (2, ['--no-cfg-parallel', '--single-layout'], True),
                                               (4, ['--dit-fsdp', '--vae-parallel', '--transport', 'peer_copy', '--layers', '3'], False)],
                         ids=['cfg2_primary_torchrun', 'sp4_and_cfg2_sp2_plain', 'sp2_single_layout_plain', 'configs3_form_cfg2_sp2_fsdp4_vaepipe_peercopy'])
def test_bench_multirank_code_path(world, extra, plain):
    """bench.py's N > 1 branches (CFG-parallel halves x Ulysses, or Ulysses over all ranks; block-sharded weights,
    pipelined VAE tail, exchange transport) on one GPU through gloo, tiny workload: must print ONE JSON line with the
    contract keys.  plain: `python bench.py --gpus N` WITHOUT torch.distributed.run — bench.py launches its own ranks;
    else the driver's torchrun form.  The last case is the command form of BASELINE configs[3] (`--gpus 8 --dit-fsdp` prints
    `cfg2 x ulysses_sp4 x fsdp8`) at 4 ranks, with 3 layers so that the two gather buffers really rotate."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MOVIIGEN_BENCH_BACKEND='gloo')
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    tail = [os.path.join(root, 'bench.py'), '--gpus', str(world), '--steps', '1', '--warmup', '1', '--workload', 'tiny', '--full'] + extra
    head = [sys.executable] if plain else [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={world}',
                                           '--master-addr', '127.0.0.1', '--master-port', str(29590 + world + len(extra))]
    r = subprocess.run(head + tail, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'sec_per_video', 'vae_decode'):
        assert k in d, k
    assert d['n_gpus'] == world and d['scaling'] == 'strong' and d['value'] > 0
    # primary layout: Ulysses over all ranks (BASELINE configs[2], the reference's layout) unless --cfg-parallel / --dit-fsdp (configs[3]);
    # the other layout of an even world is measured in the same run and reported beside it
    fsdp = '--dit-fsdp' in extra
    cfg_first = '--cfg-parallel' in extra or fsdp
    want = f'cfg2 x ulysses_sp{world // 2}' if cfg_first else f'ulysses_sp{world}'
    assert d['config']['parallelism'] == want + (f' x fsdp{world}' if fsdp else ''), d['config']
    if fsdp or '--single-layout' in extra:
        assert 'other_layout' not in d
    else:
        o = d['other_layout']
        assert o['parallelism'] == (f'ulysses_sp{world}' if cfg_first else f'cfg2 x ulysses_sp{world // 2}') and o['value'] > 0
        assert o['latent_max_abs_diff_vs_primary'] == 0.0          # both layouts computed the same K + W steps of the same video
    # the preflight leg: backend / ranks / peer access / the 64 MiB all-to-all probe; the IPC probe only with the copy-engine transport
    pf = d['preflight']
    assert pf['rccl_ranks'] == 0 and pf['link_gbps_measured']['all_to_all'] > 0 and not pf['preflight_errors'], pf
    assert pf['transport_recommended'] in ('torch', 'peer_copy') and len(pf['peer_access']) == world
    assert (pf['ipc_open'] is True and pf['link_gbps_measured']['peer_copy'] > 0) == ('peer_copy' in extra), pf
    # what the line says about the ranks: gloo plumbing here (rccl_ranks 0), one entry per rank, overlap measured
    # whenever the layout has a per-layer exchange (cfg2 on 2 ranks has none)
    assert d['rccl_ranks'] == 0 and 'gloo' in d['transport']['used'] and len(d['rank_devices']) == world
    assert d['transport']['requested'] == ('peer_copy' if 'peer_copy' in extra else 'torch')     # the collective is the default
    if fsdp:
        f = d['fsdp']
        assert f['ranks'] == world and f['gathers_per_step'] >= 2 and f['gather_ms_per_step'] > 0 and 0 <= f['exposed_ms_per_step']
        assert f['gathered_bytes_per_block'] >= 2 * (4 * 5120 * 5120 * 2 + 2 * 5120 * 13824)     # bf16 GEMM weights of one 14B-width block
    assert ('W bands over' in d['vae_decode_layout']) == ('--vae-parallel' in extra)      # the flag alone = the W-band decode
    assert sorted(e['rank'] for e in d['rank_devices']) == list(range(world))
    if want != 'cfg2 x ulysses_sp1':
        ov = d['overlap']
        assert ov['exchange_ms_per_step'] > 0 and ov['exposed_ms_per_step'] >= 0 and ov['hidden_frac'] <= 1.0
        assert sum(ov['groups']['heads_per_group']) * (world if '--no-cfg-parallel' in extra else world // 2) == 12 or ov['groups']['heads_per_group']
    else:
        assert d['overlap'] is None


def test_fullsize_generate_call(dev):
    """ONE call through the drop-in surface at the metric's size (reference wan/text2video.py:158-271): WanT2V.generate
    on the 14B architecture (random weights), 1920x832x81f, 2 UniPC steps, dim-96 WanVAE decode — shape / range /
    finite, the per-step latents equal to a hand-driven loop over the same WanModel (what bench.py times), the same
    video again under offload_model=True (a no-op on 288 GB: the DiT must stay on the device), and the wall time of
    the call against steps x step + decode."""
    import time
    import wan
    from wan.backend import ops
    from wan.configs import WAN_CONFIGS
    from wan.utils import FlowUniPCMultistepScheduler
    cfg = WAN_CONFIGS['t2v-14B']
    model = wan.modules.WanModel(dim=cfg.dim, ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, num_heads=cfg.num_heads,
                                 num_layers=cfg.num_layers, text_len=cfg.text_len, eps=cfg.eps, device=dev)
    model.init_weights(seed=0)
    vae = wan.modules.WanVAE(state_dict=W.make_vae_params(96, 1), device=dev)
    g = torch.Generator(device=dev).manual_seed(5)
    ctx = torch.randn(512, 4096, device=dev, generator=g).bfloat16()
    ctx_null = torch.randn(130, 4096, device=dev, generator=g).bfloat16()
    pipe = wan.WanT2V(cfg, checkpoint_dir=None, model=model, vae=vae)
    lats = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    video = pipe.generate(ctx, size=(1920, 832), frame_num=81, sampling_steps=2, n_prompt=ctx_null, seed=11,
                          offload_model=False, callback=lambda i, lat: lats.append(lat.clone()))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    assert tuple(video.shape) == (3, 81, 832, 1920) and video.dtype == torch.float32
    assert torch.isfinite(video).all().item() and video.abs().max().item() <= 1.0
    assert len(lats) == 2 and tuple(lats[0].shape) == (16, 21, 104, 240)
    # the same two steps driven by hand (bench.py's loop): identical latents
    noise = torch.randn(16, 21, 104, 240, dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(11))
    sch = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1, use_dynamic_shifting=False)
    sch.set_timesteps(2, device=dev, shift=5.0)
    lat, pred = noise, torch.empty_like(noise)
    L = 21 * 52 * 120
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for i, th in enumerate(sch.timesteps.tolist()):
        t = sch.timesteps[i:i + 1]
        c = model([lat], t=t, context=[ctx], seq_len=L)[0]
        u = model([lat], t=t, context=[ctx_null], seq_len=L)[0]
        ops.cfg_combine(pred, u, c, 5.0)
        lat = sch.step(pred.unsqueeze(0), th, lat.unsqueeze(0), return_dict=False)[0].squeeze(0)
        assert torch.equal(lat, lats[i]), i
    torch.cuda.synchronize()
    loop_s = time.perf_counter() - t1
    t2 = time.perf_counter()
    video2 = vae.decode([lat])[0]
    torch.cuda.synchronize()
    dec_s = time.perf_counter() - t2
    assert torch.equal(video2, video)
    # no hidden cost in the call: its wall time is the loop + the decode (+ scheduler set-up, noise, < 3 %)
    assert wall < 1.03 * (loop_s + dec_s) + 0.5, (wall, loop_s, dec_s)
    print(f'generate(1920x832x81f, 2 steps): {wall:.2f} s = loop {loop_s:.2f} s + decode {dec_s:.2f} s')
    # offload_model=True (the reference default): nothing has to move on this device, same bits
    del video2
    video3 = pipe.generate(ctx, size=(1920, 832), frame_num=81, sampling_steps=2, n_prompt=ctx_null, seed=11, offload_model=True)
    assert pipe.last_offloaded is False and next(model.parameters()).is_cuda
    assert torch.equal(video3, video)


def test_bench_live_traffic_measurement():
    """bench.py's roofline.traffic leg: the two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; --kernel-trace only) over
    `mg_selftest attnpmc` at a small launch shape — the passes run, the kernel's dispatches are found in the counter CSV,
    and the bytes are at least the algorithmic ones (q + k + v read once, o written once)."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('mg_bench', os.path.join(root, 'bench.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    L, heads = 16384, 4
    got, why = b.measure_attention_traffic(L, heads, timeout=300)
    assert got is not None, why
    alg = 4 * L * heads * 128 * 2
    assert got['dispatches'] == [2, 2]
    assert alg * 0.9 <= got['traffic_bytes_per_launch'] <= 40 * alg, (got, alg)


def test_bench_refuses_more_ranks_than_gpus():
    """`python bench.py --gpus 2` on a 1-GPU box with the production backend: fails with ITS OWN message about
    visible GPUs (RCCL cannot place two ranks on one device) — not with a WORLD_SIZE assertion."""
    import os
    import subprocess
    import sys
    if torch.cuda.device_count() >= 2:
        pytest.skip('needs a box with fewer than 2 GPUs')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MOVIIGEN_BENCH_BACKEND')}
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0',
                        '--workload', 'tiny'], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0
    assert 'needs 2 visible GPUs' in (r.stdout + r.stderr), (r.stdout + r.stderr)[-2000:]


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` times K steps and reports nothing that needs a leg of its own (those run with
    --full), and --dump-outputs writes what the last timed step computed: float32, the same bits with --full as without
    (the extra legs leave the timed path alone; the inputs are seeded)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MOVIIGEN_BENCH_BACKEND')}
    lines, dumps = [], []
    for i, extra in enumerate(([], ['--full', '--no-cpu-baseline'])):
        out = tmp_path / f'out{i}'
        r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--workload', 'tiny',
                            '--dump-outputs', str(out)] + extra, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        js = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert len(js) == 1, r.stdout[-2000:]
        lines.append(json.loads(js[0]))
        dumps.append({n: np.load(out / f'{n}.npy') for n in ('latent', 'noise_pred')})
        assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64e6
    plain, full = lines
    assert plain['steps'] == 2 and plain['warmup'] == 1 and plain['ms_per_step'] > 0 and abs(plain['value'] * plain['ms_per_step'] - 1e3) < 1e-6
    assert plain['metric'] == full['metric'] == 'denoise-steps/sec' and plain['dtype'] == 'bf16' and plain['higher_is_better'] is True
    for k in ('roofline', 'sec_per_video', 'telemetry', 'vae_decode', 'cpu_baseline'):
        assert k not in plain, k
    assert 'roofline' in full and 'vae_decode' in full
    lat = dumps[0]['latent']
    assert lat.dtype == np.float32 and lat.shape == tuple(plain['config']['latent']) and np.isfinite(lat).all()
    assert dumps[0]['noise_pred'].dtype == np.float32 and dumps[0]['noise_pred'].size == lat.size
    for n in dumps[0]:
        assert np.array_equal(dumps[0][n], dumps[1][n]), n


def test_rccl_backend_single_rank():
    """the production transport: backend "nccl" (RCCL) with device tensors, world_size 1 — the same
    collective calls and the Ulysses / sharded-weights branches of the forward, equal to the plain one."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tests', 'dist_rccl_worker.py')], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for tag in ('RCCL_COLLECTIVES_OK', 'RCCL_SP_BRANCH_OK', 'RCCL_DIRECT_OK', 'PEER_COPY_OK', 'RCCL_CONTROL_PREFLIGHT_OK', 'RCCL_FSDP_OK'):
        assert tag in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------
# umT5 encoder
# ------------------------------------------------------------------------------------------------
def _t5_model(dev, cfg=W.TINY_T5, seed=2):
    from wan.modules.t5 import T5Encoder
    m = T5Encoder(**{('vocab' if k == 'vocab_size' else k): v for k, v in cfg.items()})
    m.load_state_dict(W.make_t5_params(cfg, seed))
    return m.to(dev)


def test_t5_kernels_vs_oracle(dev):
    from oracle import t5 as ot5
    from wan.backend import ops
    from wan.modules.t5 import relative_buckets
    bf = torch.bfloat16
    # embedding gather + elementwise
    tab = W.randn((50, 128), 1).to(bf)
    ids = torch.tensor([3, 49, 0, 7, 7], dtype=torch.int64)
    out = torch.empty(5, 128, dtype=bf, device=dev)
    ops.embed_rows(tab.to(dev), ids.to(dev), out)
    assert torch.equal(out.cpu(), tab[ids])
    a, b = W.randn((33, 264), 2).to(bf), (W.randn((33, 264), 3) * 2).to(bf)
    o = torch.empty(33, 264, dtype=bf, device=dev)
    ops.ew_bf16(a.to(dev), b.to(dev), o, 0)
    assert torch.equal(o.cpu(), (a.float() + b.float()).to(bf))
    ops.ew_bf16(a.to(dev), b.to(dev), o, 1)
    g = b.float()
    ref = a.float() * (0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3))))
    assert scale_err(o.float(), ref.to(bf).float()) < 1e-2
    # attention with relative-position bias, no scaling
    for L, heads, hd in ((17, 4, 32), (24, 4, 32), (200, 2, 64), (1, 2, 64)):
        qkv = (W.randn((L, 3 * heads * hd), 4) * 0.5).to(bf)
        emb = (W.randn((32, heads), 5) * 0.5).to(bf)
        da = heads * hd
        q, k, v = (qkv[:, i * da:(i + 1) * da].float().view(L, heads, hd).permute(1, 0, 2) for i in range(3))
        s = (q @ k.transpose(1, 2)).to(bf).float() + ot5.pos_bias(emb.float(), L, L, 32)
        p = torch.softmax(s.to(bf).float(), -1)
        ref = (p @ v).permute(1, 0, 2).reshape(L, da)
        qd = qkv.to(dev)
        o = torch.empty(L, da, dtype=bf, device=dev)
        ops.t5_attention(qd[:, :da], qd[:, da:2 * da], qd[:, 2 * da:], emb.to(dev), relative_buckets(L).to(dev), o,
                         L, heads, hd)
        assert scale_err(o.float(), ref) < 1.5e-2, (L, heads, hd)


def test_t5_encoder_vs_reference(dev, golden):
    """HIP encoder vs the imported reference (g7): as close to the fp32 truth as the reference's own
    bf16 run, and within the bf16 tolerance of the bf16-emulating oracle."""
    from oracle import t5 as ot5
    g = golden('g7_t5')
    m = _t5_model(dev)
    ids, mask = T(g['ids']), T(g['mask'])
    out = m(ids.to(dev), mask.to(dev)).float().cpu()
    P = W.make_t5_params(W.TINY_T5, 2)
    for b in range(ids.shape[0]):
        kl = int(mask[b].sum())
        truth, ref_bf = g['out_fp32'][b, :kl], g['out_bf16'][b, :kl].astype(np.float32)
        got = out[b, :kl]
        assert rel_l2(got, truth) < 1.25 * rel_l2(T(ref_bf), truth) + 1e-3
        assert rel_l2(got, ot5.t5_encode(P, W.TINY_T5, ids[b], kl, True)) < 2e-2
        assert (out[b, kl:] == 0).all()
    # batch-of-one / no mask, determinism
    one = m(ids[1:2].to(dev)).float().cpu()
    assert torch.equal(one[0], out[1])


def test_t5_encoder_model_contract(dev):
    """T5EncoderModel.__call__ contract (reference t5.py:504-518) with an injected tokenizer, at the
    real width (dim 4096, 64 heads, ffn 10240; 2 layers, small vocab) against the oracle."""
    from oracle import t5 as ot5
    from wan.modules.t5 import T5EncoderModel
    cfg = dict(vocab_size=512, dim=4096, dim_attn=4096, dim_ffn=10240, num_heads=64, num_layers=2, num_buckets=32)
    m = _t5_model('cpu', cfg, seed=5)
    text_len = 64
    rs = np.random.RandomState(7)

    class Tok:
        def __call__(self, texts, return_mask=False, add_special_tokens=True):
            ids = torch.zeros(len(texts), text_len, dtype=torch.long)
            mask = torch.zeros(len(texts), text_len, dtype=torch.long)
            for i, t in enumerate(texts):
                n = min(len(t.split()) + 1, text_len)
                ids[i, :n] = T(rs.randint(1, 512, n))
                mask[i, :n] = 1
            self.last = ids, mask
            return ids, mask

    tok = Tok()
    enc = T5EncoderModel(text_len, device=dev, model=m, tokenizer=tok)
    outs = enc(['a b c d e f g h i j k', ' '.join(['w'] * 80)], dev)
    ids, mask = tok.last
    assert [tuple(o.shape) for o in outs] == [(12, 4096), (64, 4096)]
    assert all(o.dtype == torch.bfloat16 and o.device.type == 'cuda' for o in outs)
    P = W.make_t5_params(cfg, 5)
    ref = ot5.t5_encode(P, cfg, ids[0], 12, True)
    assert rel_l2(outs[0].float(), ref) < 2e-2
