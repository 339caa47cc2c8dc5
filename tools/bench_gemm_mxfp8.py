"""mg_gemm_bf16 against activation quantisation + mg_gemm_mxfp8 at the four step shapes of a DiT block (M tokens), same process,
alternating rounds, DiT-like operands (N(0,1) activations with one x50 channel, N(0, 0.02^2) weights; the weights are quantised
once, outside the timed window, as WanModel.set_gemm_precision('mxfp8') does).
    python tools/bench_gemm_mxfp8.py [M] [rounds] [iters] [sites|fused|all]  > profiles/<name>.log
One JSON line per shape and a last line with the per-site decision for MXFP8_SITES in wan/modules/model.py: a site uses fp8 only
if quantise + GEMM is faster than the bf16 kernel here.  Times are device events around `iters` back-to-back calls after a
warm-up call of each kernel; the spread over the rounds is printed so that a difference can be judged against it.

`fused` (part of `all`, the default): the producers that write an fp8 site's operand themselves against the unfused pair of the SAME
tree in the SAME run, alternating rounds —
  (a) ln_modulate (bf16 out) + quant_mxfp8 against ln_modulate_mxfp8 at dim 5120,
  (b) gemm_mxfp8 GELU + quant_mxfp8 against gemm_mxfp8_gelu_q at N = 13824, K = 5120,
  (c) the sites again as CHAINS from the fp32 residual stream to the site's output, so that a producer's own gain or loss is inside the
      figure: LayerNorm -> GEMM for wqkv and cross_attn.q, LayerNorm -> ffn.0 -> ffn.2 for the ffn; each as bf16, as fp8 with the
      stand-alone quantiser ('unfused') and as fp8 with the fused producers ('fused').
A fused producer is wired in (MXFP8_FUSED_PRODUCERS in wan/modules/model.py) only if it is not slower than its unfused pair in every
round; cross_attn.q goes to fp8 only if its fused chain beats the bf16 chain in every round."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'moviigen1.1_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402
from wan.backend import ops  # noqa: E402

M = int(sys.argv[1]) if len(sys.argv) > 1 else 131040
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
ITERS = int(sys.argv[3]) if len(sys.argv) > 3 else 20
PARTS = sys.argv[4] if len(sys.argv) > 4 else 'all'
if PARTS not in ('sites', 'fused', 'all'):
    raise SystemExit(f'unknown part {PARTS!r}: sites, fused or all')
if not torch.cuda.is_available():
    raise SystemExit('bench_gemm_mxfp8 needs the GPU: a CPU run gives no time')
dev = torch.device('cuda:0')
g = torch.Generator(device=dev).manual_seed(0)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


# (N, K, epilogue, the call sites of the layer loop with this shape)
SHAPES = ((15360, 5120, ops.BIAS_BF16, ('wqkv',)),
          (5120, 5120, ops.GATE_RESID_F32, ('self_attn.o', 'cross_attn.q', 'cross_attn.o')),
          (13824, 5120, ops.BIAS_GELU_BF16, ('ffn.0',)),
          (5120, 13824, ops.GATE_RESID_F32, ('ffn.2',)))
EPI = {ops.BIAS_BF16: 'bias', ops.BIAS_GELU_BF16: 'GELU', ops.GATE_RESID_F32: 'gate-resid'}
decision = {}
for (N, K, epi, sites) in (SHAPES if PARTS in ('sites', 'all') else ()):
    A = torch.randn(M, K, device=dev, generator=g)
    A[:, 7] *= 50.0
    A = A.bfloat16()
    Wt = (torch.randn(N, K, device=dev, generator=g) * 0.02).bfloat16()
    bias = torch.randn(N, device=dev, generator=g) * 0.02
    gate = torch.randn(N, device=dev, generator=g) if epi == ops.GATE_RESID_F32 else None
    odt = torch.float32 if epi == ops.GATE_RESID_F32 else torch.bfloat16
    out_b, out_q = torch.zeros(M, N, dtype=odt, device=dev), torch.zeros(M, N, dtype=odt, device=dev)
    wq, w_s = ops.quant_mxfp8(Wt)
    aq, a_s = torch.empty(M, K, dtype=torch.uint8, device=dev), torch.empty(M, K // 32, dtype=torch.uint8, device=dev)

    def bf16():
        ops.gemm(A, Wt, bias, epi, out_b, gate=gate)

    def quant():
        ops.quant_mxfp8(A, aq, a_s)

    def fp8_gemm():
        ops.gemm_mxfp8(aq, a_s, wq, w_s, bias, epi, out_q, gate=gate)

    def fp8():
        quant()
        fp8_gemm()
    for fn in (bf16, fp8):        # warm-up: code objects, first touch of every buffer
        fn()
    torch.cuda.synchronize()
    rel = ((out_q.float() - out_b.float())[:512].norm() / out_b.float()[:512].norm()).item()      # after ONE call each
    fl = 2.0 * M * N * K
    t = {'bf16': [], 'quant': [], 'fp8_gemm': [], 'fp8': []}
    for r in range(ROUNDS):
        t['bf16'].append(timed(bf16, ITERS))
        t['fp8'].append(timed(fp8, ITERS))
        t['quant'].append(timed(quant, ITERS))
        t['fp8_gemm'].append(timed(fp8_gemm, ITERS))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    res = {'M': M, 'N': N, 'K': K, 'epilogue': EPI[epi], 'sites': list(sites),
           'ms_per_round': {k: [round(x, 3) for x in v] for k, v in t.items()},
           'ms_median': {k: round(v, 3) for k, v in med.items()},
           'tflops': {'mg_gemm_bf16': round(fl / med['bf16'] / 1e9, 1), 'mg_gemm_mxfp8_alone': round(fl / med['fp8_gemm'] / 1e9, 1),
                      'quant_plus_mxfp8': round(fl / med['fp8'] / 1e9, 1)},
           'quant_gbytes_per_s': round(3.03125 * M * K / med['quant'] / 1e6, 1),       # 2 B read + 1 B + 1/32 B written per element
           'speedup_quant_plus_mxfp8_over_bf16': round(med['bf16'] / med['fp8'], 3),
           'fp8_wins_every_round': all(f < b for f, b in zip(t['fp8'], t['bf16'])),
           'rel_l2_mxfp8_vs_bf16_first_512_rows': rel}
    print(json.dumps(res), flush=True)
    for s in sites:
        decision[s] = bool(res['fp8_wins_every_round'])
    del A, Wt, out_b, out_q, aq, a_s, wq, w_s
    torch.cuda.empty_cache()
if decision:
    print(json.dumps({'MXFP8_SITES': decision}), flush=True)


def rounds(fns):
    """{name: [ms per round]} of the callables, one after the other inside a round, ROUNDS rounds; one warm-up call each first"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(timed(fn, ITERS))
    return t


def report(what, t, pairs, **extra):
    """pairs: (new, old) names; 'not slower / faster in every round' is judged round by round, as the acceptance rule asks"""
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    res = {'measure': what, 'M': M, **extra, 'ms_per_round': {k: [round(x, 3) for x in v] for k, v in t.items()},
           'ms_median': {k: round(v, 3) for k, v in med.items()}}
    for new, old in pairs:
        res[f'{new}_over_{old}_median_ms'] = round(med[new] - med[old], 3)
        res[f'{new}_not_slower_than_{old}_every_round'] = all(a <= b for a, b in zip(t[new], t[old]))
    print(json.dumps(res), flush=True)
    return res


if PARTS in ('fused', 'all'):
    D, F, eps = 5120, 13824, 1e-6
    u8, bf = torch.uint8, torch.bfloat16
    x = torch.randn(M, D, device=dev, generator=g)
    x[:, 7] *= 50.0
    sc, sh = torch.randn(D, device=dev, generator=g) * 0.5, torch.randn(D, device=dev, generator=g)
    h = torch.empty(M, D, dtype=bf, device=dev)
    hq, hs = torch.empty(M, D, dtype=u8, device=dev), torch.empty(M, D // 32, dtype=u8, device=dev)
    hq2, hs2 = torch.empty_like(hq), torch.empty_like(hs)
    u = torch.empty(M, F, dtype=bf, device=dev)
    uq, us = torch.empty(M, F, dtype=u8, device=dev), torch.empty(M, F // 32, dtype=u8, device=dev)
    uq2, us2 = torch.empty_like(uq), torch.empty_like(us)
    mk = lambda n, k: (torch.randn(n, k, device=dev, generator=g) * 0.02).bfloat16()  # noqa: E731
    w_qkv, w_q, w_0, w_2 = mk(3 * D, D), mk(D, D), mk(F, D), mk(D, F)
    m_qkv, m_q, m_0, m_2 = (ops.quant_mxfp8(w) for w in (w_qkv, w_q, w_0, w_2))
    b_qkv, b_d, b_f = (torch.randn(n, device=dev, generator=g) * 0.02 for n in (3 * D, D, F))
    gate = torch.randn(D, device=dev, generator=g)
    qkv, q_out = torch.empty(M, 3 * D, dtype=bf, device=dev), torch.empty(M, D, dtype=bf, device=dev)
    resid = torch.zeros(M, D, device=dev)

    def ln_bf16(add_one=True):
        ops.ln_modulate(x, sc, sh, add_one, eps, h)

    def ln_fp8(add_one=True):
        ops.ln_modulate_mxfp8(x, sc, sh, add_one, eps, hq2, hs2)

    def ln_unfused(add_one=True):
        ln_bf16(add_one)
        ops.quant_mxfp8(h, hq, hs)

    # (a)
    ta = rounds({'ln_modulate': ln_bf16, 'quant': lambda: ops.quant_mxfp8(h, hq, hs), 'unfused': ln_unfused, 'fused': ln_fp8})
    same = bool(torch.equal(hq, hq2) and torch.equal(hs, hs2))
    ra = report('(a) ln_modulate + quant_mxfp8 | ln_modulate_mxfp8', ta, (('fused', 'unfused'),), dim=D, same_bytes=same)

    # (b)
    def gelu_unfused():
        ops.gemm_mxfp8(hq, hs, m_0[0], m_0[1], b_f, ops.BIAS_GELU_BF16, u)
        ops.quant_mxfp8(u, uq, us)

    def gelu_fused():
        ops.gemm_mxfp8_gelu_q(hq, hs, m_0[0], m_0[1], b_f, uq2, us2)
    tb = rounds({'gemm_gelu': lambda: ops.gemm_mxfp8(hq, hs, m_0[0], m_0[1], b_f, ops.BIAS_GELU_BF16, u),
                 'quant': lambda: ops.quant_mxfp8(u, uq, us), 'unfused': gelu_unfused, 'fused': gelu_fused})
    same = bool(torch.equal(uq, uq2) and torch.equal(us, us2))
    rb = report('(b) gemm_mxfp8 GELU + quant_mxfp8 | gemm_mxfp8_gelu_q', tb, (('fused', 'unfused'),), N=F, K=D, same_bytes=same)

    # (c)
    def chain(site, w, m, bias, out, add_one):
        def bf16():
            ln_bf16(add_one)
            ops.gemm(h, w, bias, ops.BIAS_BF16, out)

        def unfused():
            ln_unfused(add_one)
            ops.gemm_mxfp8(hq, hs, m[0], m[1], bias, ops.BIAS_BF16, out)

        def fused():
            ln_fp8(add_one)
            ops.gemm_mxfp8(hq2, hs2, m[0], m[1], bias, ops.BIAS_BF16, out)
        t = rounds({'bf16': bf16, 'unfused': unfused, 'fused': fused})
        return report(f'(c) chain LayerNorm -> {site}', t, (('fused', 'unfused'), ('fused', 'bf16'), ('unfused', 'bf16')),
                      N=w.shape[0], K=D)
    rc_qkv = chain('wqkv', w_qkv, m_qkv, b_qkv, qkv, True)
    rc_q = chain('cross_attn.q', w_q, m_q, b_d, q_out, False)

    def ffn_bf16():
        ln_bf16()
        ops.gemm(h, w_0, b_f, ops.BIAS_GELU_BF16, u)
        ops.gemm(u, w_2, b_d, ops.GATE_RESID_F32, resid, gate=gate)

    def ffn_unfused():
        ln_unfused()
        gelu_unfused()
        ops.gemm_mxfp8(uq, us, m_2[0], m_2[1], b_d, ops.GATE_RESID_F32, resid, gate=gate)

    def ffn_fused():
        ln_fp8()
        ops.gemm_mxfp8_gelu_q(hq2, hs2, m_0[0], m_0[1], b_f, uq2, us2)
        ops.gemm_mxfp8(uq2, us2, m_2[0], m_2[1], b_d, ops.GATE_RESID_F32, resid, gate=gate)
    tf = rounds({'bf16': ffn_bf16, 'unfused': ffn_unfused, 'fused': ffn_fused})
    rc_ffn = report('(c) chain LayerNorm -> ffn.0 -> ffn.2', tf, (('fused', 'unfused'), ('fused', 'bf16'), ('unfused', 'bf16')))
    print(json.dumps({'MXFP8_FUSED_PRODUCERS': {'ln_modulate': ra['fused_not_slower_than_unfused_every_round'],
                                                'gelu': rb['fused_not_slower_than_unfused_every_round']},
                      "MXFP8_SITES['cross_attn.q']": bool(rc_q['fused_not_slower_than_bf16_every_round']
                                                          and all(a < b for a, b in zip(rc_q['ms_per_round']['fused'],
                                                                                        rc_q['ms_per_round']['bf16']))),
                      'ms_saved_per_block_fused_vs_unfused_median': round(
                          -(rc_qkv['fused_over_unfused_median_ms'] + rc_ffn['fused_over_unfused_median_ms']), 3)}), flush=True)
