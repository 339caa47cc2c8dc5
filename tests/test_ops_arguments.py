"""The argument checks of the hot-path wrappers in wan.backend.ops (-m gpu): ln_modulate, ln_modulate_mxfp8, rmsnorm_rope, pack_kv, gemm, gemm_mxfp8,
gemm_mxfp8_gelu_q, attention_hd128, attention_generic, attention_merge, t5_attention, ew_bf16, gate_residual.

ops.py checks what the C ABI cannot see: device, dtype, None against required, and that a tensor's memory holds the extent its pointer, stride and
counts claim.  One test per wrapper, at the smallest shape its C entry accepts: the operands are views into larger sentinel-filled parents
(tests/sentinels.py); the valid call comes first and has to write its output and leave the parents' margins alone, so that the rejections
behind it prove something; then every misuse has to raise before anything is launched — the parents still hold their fill."""
import pytest
import torch

from sentinels import FILL, FILL16, holds16, host, rejects, sentinel16

pytestmark = pytest.mark.gpu
BF16, I16, I32 = torch.bfloat16, torch.int16, torch.int32


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def f32(shape, dev):
    return torch.full(tuple(shape), FILL, device=dev)


def u8(shape, dev):
    return torch.full(tuple(shape), int(FILL), dtype=torch.uint8, device=dev)


def holds(t):
    return holds16(t) if t.dtype == BF16 else bool((t == FILL).all())


def margins_hold(parent, rows, cols):
    """everything of the 2-D parent outside its [rows, cols] corner still holds the fill"""
    return holds(parent[rows:]) and holds(parent[:rows, cols:])


def refill(*parents):
    for p in parents:
        p.view(I16).fill_(FILL16) if p.dtype == BF16 else p.fill_(FILL)


def rnd(shape, seed, dev, dtype=BF16):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


def rnd_parent(rows, cols, pad, seed, dev):
    """a bf16 parent [rows + 1, cols + pad] whose [rows, cols] corner holds random values -> (parent, corner)"""
    parent = sentinel16((rows + 1, cols + pad), dev)
    parent[:rows, :cols] = rnd((rows, cols), seed, dev)
    return parent, parent[:rows, :cols]


def test_rejects_ln_modulate(dev):
    from wan.backend import ops
    rows, dim = 3, 8
    xb, sb = f32((rows + 1, dim + 4), dev), f32((2, 2 * dim + 4), dev)
    xb[:rows, :dim] = rnd((rows, dim), 1, dev, torch.float32)
    x, scale, shift = xb[:rows, :dim], sb[0, :dim], sb[1, :dim]
    ob, fb = sentinel16((rows + 1, dim + 8), dev), f32((rows + 1, dim + 4), dev)
    out, outf = ob[:rows, :dim], fb[:rows, :dim]
    ops.ln_modulate(x, scale, shift, True, 1e-6, out)                                   # the valid calls: bf16 and fp32 out
    ops.ln_modulate(x, None, None, False, 1e-6, outf)
    torch.cuda.synchronize()
    assert not holds(out) and not holds(outf) and margins_hold(ob, rows, dim) and margins_hold(fb, rows, dim)
    refill(ob, fb)
    call = lambda x=x, scale=scale, shift=shift, out=out: ops.ln_modulate(x, scale, shift, True, 1e-6, out)      # noqa: E731
    rejects(lambda: call(out=out.view(torch.float16)), ob)                              # an fp16 out would be written as bf16
    rejects(lambda: call(out=out.view(I16)), ob)
    rejects(lambda: call(out=host(out)))                                                # on the host
    rejects(lambda: call(out=ob[:rows - 1, :dim]), ob)                                  # one row short
    rejects(lambda: call(out=ob[:rows, :dim - 1]), ob)                                  # one column short
    rejects(lambda: call(out=ob.view(-1)[:rows * dim]), ob)                             # not [rows, dim]
    rejects(lambda: call(out=None), ob)
    rejects(lambda: call(x=None), ob)
    rejects(lambda: call(x=host(x)), ob)
    rejects(lambda: call(x=x.view(I32)), ob)
    rejects(lambda: call(x=xb.view(-1)[:dim]), ob)                                      # x is not 2-D
    rejects(lambda: call(scale=sb[0, :dim - 1]), ob)                                    # one element short
    rejects(lambda: call(shift=sb[1, :dim + 1]), ob)                                    # one too many
    rejects(lambda: call(scale=sb[0, :2 * dim:2]), ob)                                  # strided
    rejects(lambda: call(shift=shift.view(I32)), ob)
    rejects(lambda: call(scale=host(scale)), ob)


def test_rejects_ln_modulate_mxfp8(dev):
    from wan.backend import ops
    rows, dim = 3, 128
    xb, sb = f32((rows + 1, dim + 4), dev), f32((2, 2 * dim + 4), dev)
    xb[:rows, :dim] = rnd((rows, dim), 2, dev, torch.float32)
    x, scale, shift = xb[:rows, :dim], sb[0, :dim], sb[1, :dim]
    qb, cb, ob = u8((rows + 1, dim + 16), dev), u8((rows + 1, 8), dev), sentinel16((rows + 1, dim + 8), dev)
    q, sc, out = qb[:rows, :dim], cb[:rows, :dim // 32], ob[:rows, :dim]
    ops.ln_modulate_mxfp8(x, scale, shift, True, 1e-6, q, sc, out=out)                  # the valid call
    torch.cuda.synchronize()
    assert not holds(q) and not holds(sc) and not holds(out)
    assert margins_hold(qb, rows, dim) and margins_hold(cb, rows, dim // 32) and margins_hold(ob, rows, dim)
    refill(qb, cb, ob)
    ops.ln_modulate_mxfp8(x, None, None, False, 1e-6, q, sc)                            # ... and without the bf16 copy
    torch.cuda.synchronize()
    assert not holds(q) and holds(ob)
    refill(qb, cb)
    call = lambda x=x, scale=scale, shift=shift, q=q, sc=sc, out=out: ops.ln_modulate_mxfp8(x, scale, shift, True, 1e-6, q, sc, out=out)      # noqa: E731
    for bad in (dict(x=None), dict(x=host(x)), dict(x=x.view(I32)), dict(x=xb.view(-1)[:dim]),
                dict(q=None), dict(q=q.view(torch.int8)), dict(q=qb[:rows - 1, :dim]), dict(q=qb[:rows, :dim - 1]),
                dict(sc=None), dict(sc=cb[:rows, :dim // 32 - 1]), dict(sc=cb[:rows - 1, :dim // 32]),
                dict(out=out.view(I16)), dict(out=out.view(torch.float16)), dict(out=ob[:rows - 1, :dim]), dict(out=ob[:rows, :dim - 1]),
                dict(scale=sb[0, :dim - 1]), dict(shift=sb[1, :dim + 1]), dict(scale=sb[0, :2 * dim:2]), dict(shift=host(shift))):
        rejects(lambda: call(**bad), qb, cb, ob)


def test_rejects_rmsnorm_rope(dev):
    from wan.backend import ops
    from wan.modules.model import rope_cos_sin
    rows, dim, hd, grid = 4, 128, 128, (1, 2, 2)
    xb, x = rnd_parent(rows, dim, 8, 3, dev)
    ob = sentinel16((rows + 1, dim + 8), dev)
    out = ob[:rows, :dim]
    wb = f32((dim + 4,), dev)
    weight = wb[:dim]
    tab, small = rope_cos_sin(hd, grid), rope_cos_sin(hd, (1, 2, 1))                    # 2 * 106 and 2 * 85 floats
    n = tab.numel()
    assert n == 212 and small.numel() == 170
    rb, rb2 = f32((2 * n + 8,), dev), f32((n + 8,), dev)
    rb[:n] = tab.view(-1).to(dev)
    rb2[:small.numel()] = small.view(-1).to(dev)
    rope = rb[:n].view(-1, 2)
    ops.rmsnorm_rope(x, weight, 1e-6, hd, out, rope, grid, 0)                           # the valid calls: with the table, and without
    torch.cuda.synchronize()
    assert not holds(out) and margins_hold(ob, rows, dim)
    refill(ob)
    ops.rmsnorm_rope(x, weight, 1e-6, hd, out)
    torch.cuda.synchronize()
    assert not holds(out) and margins_hold(ob, rows, dim)
    refill(ob)
    call = lambda x=x, weight=weight, out=out, rope=rope, grid=grid: ops.rmsnorm_rope(x, weight, 1e-6, hd, out, rope, grid, 0)      # noqa: E731
    for bad in (dict(rope=rb2[:small.numel()].view(-1, 2)),                             # the table of grid (1, 2, 1): the kernel would index it by (1, 2, 2)
                dict(rope=rb[:n - 1]), dict(rope=rb[:n + 1]),                           # one float short, one too many
                dict(rope=rb[:2 * n:2]), dict(rope=host(rope)), dict(rope=rope.view(I32)), dict(rope=rb[:n].double()),
                dict(grid=(1, 2, 3)),                                                   # the same table under a larger grid
                dict(weight=None), dict(weight=wb[:dim - 1]), dict(weight=wb[:dim + 1]), dict(weight=weight.view(I32)), dict(weight=host(weight)),
                dict(out=None), dict(out=ob[:rows - 1, :dim]), dict(out=ob[:rows, :dim - 8]), dict(out=out.view(I16)), dict(out=ob.view(-1)[:rows * dim]),
                dict(x=None), dict(x=host(x)), dict(x=x.view(I16)), dict(x=xb.view(-1)[:dim])):
        rejects(lambda: call(**bad), ob)


def test_rejects_pack_kv(dev):
    from wan.backend import ops
    L, heads = 64, 1
    n = ops.packed_kv_numel(L, heads)
    (kb, k), (vb, v) = rnd_parent(L, 128, 8, 4, dev), rnd_parent(L, 128, 8, 5, dev)
    kpb, vpb = sentinel16((2 * n,), dev), sentinel16((2 * n,), dev)
    kp, vp = kpb[:n], vpb[:n]
    ops.pack_kv(k, v, heads, kp, vp)                                                    # the valid calls: both, and V alone
    torch.cuda.synchronize()
    assert not holds(kp) and not holds(vp) and holds(kpb[n:]) and holds(vpb[n:])
    refill(kpb, vpb)
    ops.pack_kv(None, v, heads, None, vp)
    torch.cuda.synchronize()
    assert not holds(vp) and holds(kpb) and holds(vpb[n:])
    refill(vpb)
    call = lambda k=k, v=v, heads=heads, kp=kp, vp=vp: ops.pack_kv(k, v, heads, kp, vp)      # noqa: E731
    for bad in (dict(k=kb[:L - 1, :128]), dict(v=vb[:L + 1, :128]),                     # k and v differ in rows
                dict(k=kb[:L, :120]), dict(v=vb[:L, :120]),                             # fewer than heads * 128 columns
                dict(heads=2, kp=kpb, vp=vpb),                                          # room for two heads in kp, vp, but not in k, v
                dict(kp=kpb[:n - 1]), dict(vp=vpb[:n - 1]), dict(kp=kpb[::2]), dict(kp=None), dict(vp=None),
                dict(k=None, v=None), dict(k=host(k)), dict(v=v.view(I16)), dict(kp=kp.view(I16)), dict(k=kb.view(-1)[:128])):
        rejects(lambda: call(**bad), kpb, vpb)


def test_rejects_gemm(dev):
    from wan.backend import ops
    M, N, K = 8, 8, 64
    (ab, a), (wb, w) = rnd_parent(M, K, 64, 6, dev), rnd_parent(N, K, 64, 7, dev)
    bb, gb = f32((2 * N + 4,), dev), f32((2 * N + 4,), dev)
    bias, gate = bb[:N], gb[:N]
    ob, fb = sentinel16((M + 1, N + 8), dev), f32((M + 1, N + 4), dev)
    out, outf = ob[:M, :N], fb[:M, :N]
    ops.gemm(a, w, bias, ops.BIAS_BF16, out)                                            # the valid calls: a bf16 and an fp32 epilogue
    ops.gemm(a, w, bias, ops.GATE_RESID_F32, outf, gate=gate)
    torch.cuda.synchronize()
    assert not holds(out) and not holds(outf) and margins_hold(ob, M, N) and margins_hold(fb, M, N)
    refill(ob, fb)
    call = lambda a=a, w=w, bias=bias, out=out: ops.gemm(a, w, bias, ops.BIAS_BF16, out)      # noqa: E731
    for bad in (dict(bias=bb[:N - 1]), dict(bias=bb[:N + 1]), dict(bias=bb[:2 * N:2]), dict(bias=bias.view(I32)), dict(bias=host(bias)),
                dict(out=ob[:M - 1, :N]), dict(out=ob[:M, :N - 1]), dict(out=outf), dict(out=out.view(I16)), dict(out=None),
                dict(a=None), dict(a=ab.view(-1)[:K]), dict(a=ab[:M, :K].view(2, 4, K)), dict(a=host(a)), dict(a=a.view(I16)),
                dict(w=None), dict(w=wb[:N, :2 * K]), dict(w=wb.view(-1)[:K])):
        rejects(lambda: call(**bad), ob, fb)
    for bad in (gb[:N - 1], gb[:N + 1], gb[:2 * N:2], gate.view(I32), host(gate)):      # the gate of the gated-residual epilogue
        rejects(lambda: ops.gemm(a, w, bias, ops.GATE_RESID_F32, outf, gate=bad), ob, fb)


def _mx_operands(dev, M, N, K, seed):
    """e4m3 bytes below 0x78 (finite, |v| < 256) and scale bytes 127 (= 1.0) in the corners of FILL parents"""
    g = torch.Generator().manual_seed(seed)
    aqb, wqb, asb, wsb = u8((M + 1, K + 16), dev), u8((N + 1, K + 16), dev), u8((M + 1, K // 32 + 4), dev), u8((N + 1, K // 32 + 4), dev)
    aqb[:M, :K] = torch.randint(0, 0x78, (M, K), generator=g).to(torch.uint8).to(dev)
    wqb[:N, :K] = torch.randint(0, 0x78, (N, K), generator=g).to(torch.uint8).to(dev)
    asb[:M, :K // 32] = 127
    wsb[:N, :K // 32] = 127
    return (aqb, wqb, asb, wsb), (aqb[:M, :K], asb[:M, :K // 32], wqb[:N, :K], wsb[:N, :K // 32])


def test_rejects_gemm_mxfp8(dev):
    from wan.backend import ops
    M, N, K = 4, 16, 128
    (aqb, wqb, asb, wsb), (aq, a_s, wq, w_s) = _mx_operands(dev, M, N, K, 8)
    bb, gb = f32((2 * N + 4,), dev), f32((2 * N + 4,), dev)
    bias, gate = bb[:N], gb[:N]
    ob, fb = sentinel16((M + 1, N + 8), dev), f32((M + 1, N + 4), dev)
    out, outf = ob[:M, :N], fb[:M, :N]
    ops.gemm_mxfp8(aq, a_s, wq, w_s, bias, ops.BIAS_BF16, out)                          # the valid calls
    ops.gemm_mxfp8(aq, a_s, wq, w_s, bias, ops.GATE_RESID_F32, outf, gate=gate)
    torch.cuda.synchronize()
    assert not holds(out) and not holds(outf) and margins_hold(ob, M, N) and margins_hold(fb, M, N)
    refill(ob, fb)
    call = lambda aq=aq, a_s=a_s, wq=wq, w_s=w_s, bias=bias, out=out: ops.gemm_mxfp8(aq, a_s, wq, w_s, bias, ops.BIAS_BF16, out)      # noqa: E731
    for bad in (dict(bias=bb[:N - 1]), dict(bias=bb[:N + 1]), dict(bias=bb[:2 * N:2]), dict(bias=bias.view(I32)), dict(bias=host(bias)),
                dict(out=ob[:M - 1, :N]), dict(out=ob[:M, :N - 1]), dict(out=outf), dict(out=None),
                dict(aq=None), dict(aq=aq.view(torch.int8)), dict(aq=aqb.view(-1)[:K]), dict(aq=host(aq)),
                dict(a_s=None), dict(a_s=asb[:M, :K // 32 - 1]), dict(a_s=asb[:M - 1, :K // 32]),
                dict(w_s=None), dict(w_s=wsb[:N - 1, :K // 32]), dict(wq=wqb[:N, :K - 1])):
        rejects(lambda: call(**bad), ob, fb)
    for bad in (gb[:N - 1], gb[:N + 1], gate.view(I32)):
        rejects(lambda: ops.gemm_mxfp8(aq, a_s, wq, w_s, bias, ops.GATE_RESID_F32, outf, gate=bad), ob, fb)


def test_rejects_gemm_mxfp8_gelu_q(dev):
    from wan.backend import ops
    M, N, K = 4, 32, 128
    (aqb, wqb, asb, wsb), (aq, a_s, wq, w_s) = _mx_operands(dev, M, N, K, 9)
    bb = f32((2 * N + 4,), dev)
    bias = bb[:N]
    qb, cb = u8((M + 1, N + 16), dev), u8((M + 1, N // 32 + 3), dev)
    oq, o_s = qb[:M, :N], cb[:M, :N // 32]
    ops.gemm_mxfp8_gelu_q(aq, a_s, wq, w_s, bias, oq, o_s)                              # the valid call
    torch.cuda.synchronize()
    assert not holds(oq) and margins_hold(qb, M, N) and margins_hold(cb, M, N // 32)
    refill(qb, cb)
    call = lambda aq=aq, a_s=a_s, wq=wq, w_s=w_s, bias=bias, oq=oq, o_s=o_s: ops.gemm_mxfp8_gelu_q(aq, a_s, wq, w_s, bias, oq, o_s)      # noqa: E731
    for bad in (dict(bias=bb[:N - 1]), dict(bias=bb[:N + 1]), dict(bias=bb[:2 * N:2]), dict(bias=bias.view(I32)), dict(bias=host(bias)),
                dict(oq=None), dict(oq=qb[:M - 1, :N]), dict(oq=qb[:M, :N - 1]), dict(oq=oq.view(torch.int8)), dict(oq=host(oq)),
                dict(o_s=None), dict(o_s=cb[:M - 1, :N // 32]), dict(o_s=cb[:M, :N // 32 + 1]),
                dict(aq=None), dict(aq=aqb.view(-1)[:K]), dict(a_s=asb[:M, :K // 32 - 1]), dict(w_s=wsb[:N - 1, :K // 32])):
        rejects(lambda: call(**bad), qb, cb)


def _packed(dev, L, heads, seed):
    """K and V of L keys packed for attention_hd128, each at the start of a sentinel parent twice the size"""
    from wan.backend import ops
    n = ops.packed_kv_numel(L, heads)
    kpb, vpb = sentinel16((2 * n,), dev), sentinel16((2 * n,), dev)
    ops.pack_kv(rnd((L, heads * 128), seed, dev), rnd((L, heads * 128), seed + 1, dev), heads, kpb[:n], vpb[:n])
    return kpb, vpb, n


def test_rejects_attention_hd128(dev):
    from wan.backend import lib, ops
    Lq, Lk, heads = 16, 64, 1
    kpb, vpb, n = _packed(dev, Lk, heads, 10)
    kp, vp = kpb[:n], vpb[:n]
    qb, q = rnd_parent(Lq, 128, 8, 12, dev)
    ob, lb = sentinel16((Lq + 1, 128 + 8), dev), f32((2 * Lq + 4,), dev)
    out, lse = ob[:Lq, :128], lb[:Lq]
    nbytes = int(lib.load().mg_attn_workspace_bytes())
    wsb = torch.zeros(2 * nbytes + 8, dtype=torch.uint8, device=dev)
    ws = wsb[:nbytes]
    for kw in (dict(), dict(workspace=None), dict(workspace=ws), dict(workspace=ws, lse=lse), dict(workspace=ws, lse=lse, prescaled=True)):      # the valid calls
        ops.attention_hd128(q, kp, vp, out, Lk, heads, 128 ** -0.5, **kw)
        torch.cuda.synchronize()
        assert not holds(out) and margins_hold(ob, Lq, 128) and ('lse' in kw) != holds(lse) and holds(lb[Lq:]) and not wsb.any().item()
        refill(ob, lb)
    call = lambda q=q, kp=kp, vp=vp, out=out, heads=heads, **kw: ops.attention_hd128(q, kp, vp, out, Lk, heads, 128 ** -0.5, **kw)      # noqa: E731
    for bad in (dict(q=qb[:Lq, :120]), dict(out=ob[:Lq, :120]), dict(out=ob[:Lq - 1, :128]),      # columns below heads * 128, out shorter than q
                dict(heads=2, kp=kpb, vp=vpb),                                          # tiles for two heads, q and out for one
                dict(kp=kpb[:n - 1]), dict(vp=vpb[:n - 1]), dict(kp=kpb[::2]), dict(kp=None), dict(vp=vp.view(I16)),
                dict(q=None), dict(out=None), dict(q=host(q)), dict(q=q.view(I16)), dict(out=out.view(torch.float16)), dict(q=qb.view(-1)[:128]),
                dict(workspace=wsb[:nbytes - 1]), dict(workspace=wsb[:2 * nbytes:2]), dict(workspace=ws.view(torch.int8)),
                dict(workspace=ws.view(torch.float32)), dict(workspace=host(ws)),
                dict(lse=lb[:Lq - 1]), dict(lse=lb[:2 * Lq:2]), dict(lse=lse.view(I32)), dict(lse=host(lse))):
        rejects(lambda: call(**bad), ob, lb)
    assert not wsb.any().item()


def test_rejects_attention_generic(dev):
    from wan.backend import ops
    L, heads, hd = 16, 1, 32
    (qb, q), (kb, k), (vb, v) = (rnd_parent(L, hd, 8, s, dev) for s in (13, 14, 15))
    ob = sentinel16((L + 1, hd + 8), dev)
    out = ob[:L, :hd]
    ops.attention_generic(q, k, v, out, L, heads, hd, hd ** -0.5)                       # the valid call
    torch.cuda.synchronize()
    assert not holds(out) and margins_hold(ob, L, hd)
    refill(ob)
    call = lambda q=q, k=k, v=v, out=out, heads=heads: ops.attention_generic(q, k, v, out, L, heads, hd, hd ** -0.5)      # noqa: E731
    for bad in (dict(k=kb[:L - 1, :hd]), dict(v=vb[:L - 1, :hd]),                       # fewer than lk rows
                dict(q=qb[:L, :hd - 8]), dict(k=kb[:L, :hd - 8]), dict(v=vb[:L, :hd - 8]), dict(out=ob[:L, :hd - 8]),      # fewer than heads * head_dim columns
                dict(heads=2), dict(out=ob[:L - 1, :hd]),
                dict(q=None), dict(k=None), dict(v=None), dict(out=None), dict(q=host(q)), dict(k=k.view(I16)), dict(out=out.view(torch.float16)),
                dict(v=vb.view(-1)[:hd])):
        rejects(lambda: call(**bad), ob)


def test_rejects_attention_merge(dev):
    from wan.backend import ops
    rows, heads, cols = 4, 1, 128
    ab, lab, lpb = f32((rows + 1, cols + 4), dev), f32((2 * rows + 4,), dev), f32((2 * rows + 4,), dev)
    pb, part = rnd_parent(rows, cols, 8, 16, dev)
    ob = sentinel16((rows + 1, cols + 8), dev)
    acc, lse_acc, lse_part, out = ab[:rows, :cols], lab[:rows], lpb[:rows], ob[:rows, :cols]
    lse_part.copy_(rnd((rows,), 17, dev, torch.float32))
    ops.attention_merge(acc, lse_acc, part, lse_part, heads, True, out=out)             # the valid calls: the first block, a second one
    ops.attention_merge(acc, lse_acc, part, lse_part, heads, False)
    torch.cuda.synchronize()
    assert not holds(acc) and not holds(lse_acc) and not holds(out)
    assert margins_hold(ab, rows, cols) and margins_hold(ob, rows, cols) and holds(lab[rows:])
    refill(ab, lab, ob)
    call = lambda acc=acc, lse_acc=lse_acc, part=part, lse_part=lse_part, heads=heads, out=out: \
        ops.attention_merge(acc, lse_acc, part, lse_part, heads, True, out=out)         # noqa: E731
    for bad in (dict(part=pb[:rows - 1, :cols]), dict(part=pb[:rows, :cols - 8]),       # acc and part differ in shape
                dict(heads=2),                                                          # fewer than heads * 128 columns
                dict(lse_acc=lab[:rows - 1]), dict(lse_part=lpb[:rows - 1]), dict(lse_acc=lab[:2 * rows:2]), dict(lse_part=lpb[:2 * rows:2]),
                dict(out=ob[:rows - 1, :cols]), dict(out=ob[:rows, :cols - 8]), dict(out=out.view(I16)), dict(out=host(out)),
                dict(acc=None), dict(acc=acc.view(I32)), dict(acc=host(acc)), dict(acc=ab.view(-1)[:cols]),
                dict(part=None), dict(part=part.view(I16)), dict(lse_acc=None), dict(lse_part=lse_part.view(I32))):
        rejects(lambda: call(**bad), ab, lab, ob)


def test_rejects_t5_attention(dev):
    from wan.backend import ops
    L, heads, hd, buckets = 8, 1, 32, 32
    fb, _ = rnd_parent(L, 3 * hd, 8, 18, dev)
    q, k, v = (fb[:L, i * hd:(i + 1) * hd] for i in range(3))
    emb = torch.zeros(buckets, heads, dtype=BF16, device=dev)
    rb = torch.zeros(2 * L + 4, dtype=I32, device=dev)
    bucket = rb[:2 * L - 1]
    ob = sentinel16((L + 1, hd + 8), dev)
    out = ob[:L, :hd]
    ops.t5_attention(q, k, v, emb, bucket, out, L, heads, hd)                           # the valid call
    torch.cuda.synchronize()
    assert not holds(out) and margins_hold(ob, L, hd)
    refill(ob)
    call = lambda q=q, k=k, v=v, emb=emb, bucket=bucket, out=out: ops.t5_attention(q, k, v, emb, bucket, out, L, heads, hd)      # noqa: E731
    for bad in (dict(out=ob[:L - 1, :hd]), dict(out=ob[:L, :hd - 8]),                   # out below [Lq, heads * head_dim]
                dict(k=fb[:L - 1, hd:2 * hd]), dict(v=fb[:L - 1, 2 * hd:3 * hd]),       # fewer than lk rows
                dict(out=None), dict(out=out.view(I16)), dict(out=host(out)), dict(out=ob.view(-1)[:L * hd]),
                dict(q=None), dict(k=None), dict(v=None), dict(q=host(q)), dict(k=k.view(I16)),
                dict(emb=None), dict(emb=emb.view(I16)), dict(bucket=None), dict(bucket=rb[:2 * L - 2]), dict(bucket=bucket.view(torch.float32))):
        rejects(lambda: call(**bad), ob)


def test_rejects_ew_bf16(dev):
    from wan.backend import ops
    n = 16
    ab, bb, ob = sentinel16((2 * n + 8,), dev), sentinel16((2 * n + 8,), dev), sentinel16((2 * n + 8,), dev)
    ab[:n], bb[:n] = rnd((n,), 19, dev), rnd((n,), 20, dev)
    a, b, out = ab[:n], bb[:n], ob[:n]
    for mode in (0, 1):                                                                 # the valid calls
        ops.ew_bf16(a, b, out, mode)
        torch.cuda.synchronize()
        assert not holds(out) and holds(ob[n:])
        refill(ob)
    call = lambda a=a, b=b, out=out, mode=0: ops.ew_bf16(a, b, out, mode)               # noqa: E731
    for bad in (dict(a=ab[:n - 8]), dict(a=ab[:n + 8]), dict(b=bb[:n - 8]), dict(b=bb[:n - 1]), dict(out=ob[:n - 8]), dict(out=ob[:n + 8]),      # one element count
                dict(a=ab[:2 * n:2]), dict(b=bb[:2 * n:2]), dict(out=ob[:2 * n:2]), dict(mode=2), dict(mode=-1),
                dict(a=None), dict(b=None), dict(out=None), dict(a=host(a)), dict(out=host(out)), dict(b=b.view(I16)), dict(out=out.view(torch.float16))):
        rejects(lambda: call(**bad), ob)


def test_rejects_gate_residual(dev):
    from wan.backend import ops
    rows, dim = 3, 8
    xb, gb = f32((rows + 1, dim + 4), dev), f32((2 * dim + 4,), dev)
    yb, y = rnd_parent(rows, dim, 8, 21, dev)
    x, gate = xb[:rows, :dim], gb[:dim]
    ops.gate_residual(x, y, gate)                                                       # the valid calls: x += y * gate, x += y
    torch.cuda.synchronize()
    assert not (x == FILL).any().item() and margins_hold(xb, rows, dim)
    refill(xb)
    ops.gate_residual(x, y)
    torch.cuda.synchronize()
    assert not (x == FILL).any().item() and margins_hold(xb, rows, dim)
    refill(xb)
    call = lambda x=x, y=y, gate=gate: ops.gate_residual(x, y, gate)                    # noqa: E731
    for bad in (dict(gate=gb[:dim - 1]), dict(gate=gb[:dim + 1]), dict(gate=gb[:2 * dim:2]), dict(gate=gate.view(I32)), dict(gate=host(gate)),
                dict(y=yb[:rows - 1, :dim]), dict(y=yb[:rows, :dim - 4]), dict(y=None), dict(y=y.view(I16)), dict(y=host(y)), dict(y=yb.view(-1)[:dim]),
                dict(x=None), dict(x=x.view(I32)), dict(x=xb.view(-1)[:dim])):
        rejects(lambda: call(**bad), xb)
    rejects(lambda: call(x=host(x)))
