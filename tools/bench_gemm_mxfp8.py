"""mg_gemm_bf16 against activation quantisation + mg_gemm_mxfp8 at the four step shapes of a DiT block (M tokens), same process,
alternating rounds, DiT-like operands (N(0,1) activations with one x50 channel, N(0, 0.02^2) weights; the weights are quantised
once, outside the timed window, as WanModel.set_gemm_precision('mxfp8') does).
    python tools/bench_gemm_mxfp8.py [M] [rounds] [iters]  > profiles/<name>.log
One JSON line per shape and a last line with the per-site decision for MXFP8_SITES in wan/modules/model.py: a site uses fp8 only
if quantise + GEMM is faster than the bf16 kernel here.  Times are device events around `iters` back-to-back calls after a
warm-up call of each kernel; the spread over the rounds is printed so that a difference can be judged against it."""
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
for (N, K, epi, sites) in SHAPES:
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
print(json.dumps({'MXFP8_SITES': decision}), flush=True)
