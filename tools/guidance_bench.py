"""The guided mix of WanT2V.generate(guidance=) at the metric's latent size, 16 x 21 x 104 x 240 = 8 386 560 fp32 elements (1920x832x81f): the three
launches of the CFG-Zero* / rescale path — mg_cfg_stats_f32 (with its one-lane finish), mg_cfg_coef_f32, mg_cfg_combine_coef_f32 — next to the plain
path's mg_cfg_combine_f32 on the same tensors, in one process and one run, alternating.  One JSON line per figure.
    python tools/guidance_bench.py [elements]

Device events around `rounds` passes over a ring of distinct (uncond, cond, out) triples larger than the 256 MB last-level cache, so every launch
reads its inputs from HBM; bytes = what the algorithm has to move (stats: read u, c; combine: read u, c, write out), next to the 6.29 TB/s a copy
reaches on this part.  The event window holds the launches back to back as the sampling loop issues them, through the Python
wrappers: where a kernel is shorter than its launch the figure is the launch rate — the kernels' own times come from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats, a run of its own)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'moviigen1.1_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402
from wan.backend import ops  # noqa: E402

COPY_TBS = 6.29
RING, ROUNDS, REPEATS = 6, 50, 3


def main(n):
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(0)
    ring = []
    for _ in range(RING):               # 6 x 3 x 33.5 MB = 604 MB of distinct tensors
        u = torch.randn(n, device=dev, generator=gen) + 0.5
        ring.append((u, u + 0.3 * torch.randn(n, device=dev, generator=gen), torch.empty(n, device=dev)))
    stats, partials = torch.empty(5, dtype=torch.float64, device=dev), ops.cfg_stats_partials(dev)
    coef = torch.empty(2, device=dev)

    def three(u, c, out):
        ops.cfg_stats(u, c, stats, partials)
        ops.cfg_coefficients(stats, n, 5.0, True, 0.7, coef)
        ops.cfg_combine_coef(out, u, c, coef)
    cases = [('mg_cfg_combine_f32 (the plain path)', lambda u, c, out: ops.cfg_combine(out, u, c, 5.0), 3 * n * 4),
             ('stats + coef + combine_coef (zero_star, rescale 0.7)', three, 5 * n * 4),
             ('mg_cfg_stats_f32 alone (two launches)', lambda u, c, out: ops.cfg_stats(u, c, stats, partials), 2 * n * 4),
             ('mg_cfg_coef_f32 alone', lambda u, c, out: ops.cfg_coefficients(stats, n, 5.0, True, 0.7, coef), 0),
             ('mg_cfg_combine_coef_f32 alone', lambda u, c, out: ops.cfg_combine_coef(out, u, c, coef), 3 * n * 4)]
    for _, fn, _ in cases:              # warm up: every kernel launched, every tensor touched
        for t in ring:
            fn(*t)
    torch.cuda.synchronize()
    for rep in range(REPEATS):          # the cases alternate: a drift of the box shows as a spread between the repeats
        for name, fn, nbytes in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ROUNDS):
                for t in ring:
                    fn(*t)
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) / (ROUNDS * RING) * 1e3
            print(json.dumps({'what': name, 'elements': n, 'repeat': rep, 'us': round(us, 2), 'GB_per_s': round(nbytes / us / 1e3, 1),
                              'frac_of_copy_6.29': round(nbytes / us / 1e6 / COPY_TBS, 3), 'launches_timed': ROUNDS * RING,
                              'device': torch.cuda.get_device_name(dev)}), flush=True)
    three(*ring[0])
    print(json.dumps({'coefficients (a_u, a_c) of the last triple': coef.tolist(), 'stats': stats.tolist()}), flush=True)


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 16 * 21 * 104 * 240)
