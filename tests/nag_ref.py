"""References for normalized attention guidance — test infrastructure, NOT product code.

nag_rows: the row arithmetic of mg_nag_combine_bf16 in fp64, taken from bf16 inputs, with what the error bound of tests/test_nag.py needs.
dit_forward_nag: a restatement of the DiT forward with NAG in every cross-attention, built from oracle.dit's helpers with its own block
routine; without NAG it equals oracle.dit.dit_forward bit for bit (a CPU test asserts it, so it cannot drift from the oracle).
"""
import torch
import torch.nn.functional as F

from oracle import dit as O


def nag_rows(p, n, scale, tau, alpha):
    """p, n: [rows, dim] bf16 (or anything holding bf16 values) -> dict of fp64 tensors:
        out [rows, dim]   alpha c g + (1 - alpha) p, NOT rounded to bf16
        c [rows], clipped [rows] (bool: Ng > tau Np)
        M [rows, dim]     alpha c (s |p| + (s - 1) |n|) + (1 - alpha) |p|: the magnitude the fp32 error of an element scales with
        kappa [rows]      sum_j (s |p_j| + (s - 1) |n_j|) / sum_j |g_j| >= 1 (1 where both are 0): how much the rounding of g weighs in Ng
        margin [rows]     |Ng - tau Np| / (tau Np), inf where Np = 0: the distance of the row from the clip threshold"""
    p, n = p.to(torch.float64), n.to(torch.float64)
    s = float(scale)
    g = s * p - (s - 1.0) * n
    G = s * p.abs() + (s - 1.0) * n.abs()
    Np, Ng = p.abs().sum(1), g.abs().sum(1)
    clipped = Ng > tau * Np
    c = torch.where(clipped, tau * Np / (Ng + 1e-7), torch.ones_like(Np))
    out = alpha * c[:, None] * g + (1.0 - alpha) * p
    M = alpha * c[:, None] * G + (1.0 - alpha) * p.abs()
    kappa = torch.where(Ng > 0, G.sum(1) / Ng.clamp_min(1e-300), torch.ones_like(Ng))
    margin = torch.where(Np > 0, (Ng - tau * Np).abs() / (tau * Np).clamp_min(1e-300), torch.full_like(Np, float('inf')))
    return dict(out=out, c=c, clipped=clipped, M=M, kappa=kappa, margin=margin)


def nag_mix(p, n, nag, bf):
    """the mix of two attention outputs [L, dim] as the forward applies it: fp64 arithmetic, ONE rounding to bf16 in bf16 mode (the engine's
    fp32 value differs from this by far less than that rounding); fp32 otherwise"""
    r = nag_rows(p, n, *nag)
    return O._bf(r['out'].to(torch.float32), bf), r['clipped']


def block(P, pre, x, e0, seq_len_valid, grid, tables, ctx, num_heads, eps, bf, first_block, neg=None, nag=None, clip_log=None):
    """oracle.dit.block (model.py:274-313) with NAG in the cross-attention: neg [Lc, dim] the embedded negative prompt, nag = (scale, tau,
    alpha); neg None: the oracle's block, operation for operation."""
    L, dim = x.shape
    hd = dim // num_heads
    e = (P[pre + 'modulation'][0] + e0).to(torch.float32)

    def norm_mod(xx, shift, scale):
        y = O.layernorm(xx, eps)
        if first_block and bf:
            y = O._bf(y, True)
        return y * (1 + scale) + shift

    h = norm_mod(x, e[0], e[1])
    sa = pre + 'self_attn.'
    q = O.rmsnorm(O.linear(h, P[sa + 'q.weight'], P[sa + 'q.bias'], bf), P[sa + 'norm_q.weight'], eps, bf)
    k = O.rmsnorm(O.linear(h, P[sa + 'k.weight'], P[sa + 'k.bias'], bf), P[sa + 'norm_k.weight'], eps, bf)
    v = O.linear(h, P[sa + 'v.weight'], P[sa + 'v.bias'], bf)
    q = O.rope(q.view(L, num_heads, hd), grid, tables, 0)
    k = O.rope(k.view(L, num_heads, hd), grid, tables, 0)
    a = O.attention(q, k, v.view(L, num_heads, hd), seq_len_valid, bf)
    y = O.linear(a.reshape(L, dim), P[sa + 'o.weight'], P[sa + 'o.bias'], bf)
    x = x.to(torch.float32) + y * e[2]

    ca = pre + 'cross_attn.'
    h = O.layernorm(x, eps, P[pre + 'norm3.weight'], P[pre + 'norm3.bias'])
    q = O.rmsnorm(O.linear(h, P[ca + 'q.weight'], P[ca + 'q.bias'], bf), P[ca + 'norm_q.weight'], eps, bf)

    def cross(c):
        kc = O.rmsnorm(O.linear(c, P[ca + 'k.weight'], P[ca + 'k.bias'], bf), P[ca + 'norm_k.weight'], eps, bf)
        vc = O.linear(c, P[ca + 'v.weight'], P[ca + 'v.bias'], bf)
        Lc = c.shape[0]
        return O.attention(q.view(L, num_heads, hd), kc.view(Lc, num_heads, hd), vc.view(Lc, num_heads, hd), Lc, bf).reshape(L, dim)
    a = cross(ctx)
    if neg is not None:
        a, clipped = nag_mix(a, cross(neg), nag, bf)
        if clip_log is not None:
            clip_log.append(clipped)
    x = x + O.linear(a, P[ca + 'o.weight'], P[ca + 'o.bias'], bf)

    h = O.layernorm(x, eps) * (1 + e[4]) + e[3]
    u = O.linear(h, P[pre + 'ffn.0.weight'], P[pre + 'ffn.0.bias'], bf)
    u = O._bf(F.gelu(u, approximate='tanh'), bf)
    y = O.linear(u, P[pre + 'ffn.2.weight'], P[pre + 'ffn.2.bias'], bf)
    return x + y * e[5]


def dit_forward_nag(P, cfg, lat, t, ctx, seq_len, neg_ctx=None, nag=None, emulate_bf16=False, clip_log=None):
    """oracle.dit.dit_forward with nag = (scale, tau, alpha) and the negative prompt neg_ctx [Ln, text_dim]; neg_ctx None: the plain forward.
    clip_log: a list that receives, per block, the bool [L] of the rows the clip acted on."""
    bf = emulate_bf16
    x, grid = O.patch_embed(P, lat.to(torch.float32), cfg['patch_size'], bf)
    L = x.shape[0]
    assert L <= seq_len
    x = torch.cat([x, torch.zeros(seq_len - L, x.shape[1])])
    e, e0 = O.time_embed(P, t.reshape(1), cfg['freq_dim'])
    c = O.text_embed(P, ctx, cfg['text_len'], bf)
    neg = None if neg_ctx is None else O.text_embed(P, neg_ctx, cfg['text_len'], bf)
    tables = O.rope_table(cfg['dim'] // cfg['num_heads'])
    for i in range(cfg['num_layers']):
        x = block(P, f'blocks.{i}.', x, e0[0], L, grid, tables, c, cfg['num_heads'], cfg['eps'], bf, i == 0, neg, nag, clip_log)
    y = O.head(P, x, e[0], cfg['eps'])
    return O.unpatchify(y, grid, cfg['patch_size'], cfg['out_dim']).to(torch.float32)
