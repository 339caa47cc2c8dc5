"""What normalized attention guidance (WanModel.forward(nag=)) costs, in one process and one run.  One JSON line per figure.
    python tools/nag_bench.py [--skip-step] [--skip-kernel]

(a) the kernel: mg_nag_combine_bf16 at rows = 131 040 (21 x 52 x 120 tokens, 1920x832x81f), dim = 5120, in place as the model runs it,
    as achieved bytes/s over what the algorithm moves, 3 x rows x dim x 2 bytes (read zp, read zn, write out) — next to its partner
    mg_rmsnorm_rope_bf16 (with RoPE, head_dim 128, as the model runs it on q) on the same rows x dim, 2 x rows x dim x 2 bytes: the
    project's existing wave-per-row pass.  A tensor is 1.34 GB: every launch reads HBM, not the 256 MB last-level cache.  Device events
    around LAUNCHES launches issued back to back through the Python wrappers; the two alternate, REPEATS repeats.
(b) the step: the DiT forwards that make one step's prediction at 1280x720x81f (14B architecture, random-init weights, 75 600 tokens):
    a cond-only step (model(...)), a cond-only step with NAG (model(..., nag=)), and a guided step (forward_pair + cfg_combine).  The
    scheduler update (a few launches on the 16 x 21 x 90 x 160 latent) is the same for all three and is not in the window.  Each kind is
    run once untimed (prompt caches, workspace, first launches), then the kinds alternate, STEP_REPEATS repeats, each timed by device events
    and ended by a synchronise.

Quality is NOT measured: random-init weights say nothing about what a scale, tau or alpha does to a video."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'moviigen1.1_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402
from wan.backend import ops  # noqa: E402

ROWS, DIM, GRID, HEAD_DIM = 131040, 5120, (21, 52, 120), 128
LAUNCHES, REPEATS, STEP_REPEATS = 40, 3, 2
COPY_TBS = 6.29         # what a copy reaches on this part


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def kernel(dev):
    from wan.modules.model import rope_cos_sin
    gen = torch.Generator(device=dev).manual_seed(0)
    zp = torch.randn(ROWS, DIM, device=dev, generator=gen).to(torch.bfloat16)
    zn = torch.randn(ROWS, DIM, device=dev, generator=gen).to(torch.bfloat16)
    keep = zp.clone()
    out = torch.empty_like(zp)
    weight = torch.ones(DIM, device=dev)
    rope = rope_cos_sin(HEAD_DIM, GRID).to(dev)
    n = ROWS * DIM * 2
    cases = [('mg_nag_combine_bf16 (4, 2.5, 0.5), in place', lambda: ops.nag_combine(zp, zn, zp, 4.0, 2.5, 0.5), 3 * n),
             ('mg_nag_combine_bf16 (4, 2.5, 0.5), out of place', lambda: ops.nag_combine(keep, zn, out, 4.0, 2.5, 0.5), 3 * n),
             ('mg_rmsnorm_rope_bf16 (RoPE, head_dim 128): the partner', lambda: ops.rmsnorm_rope(keep, weight, 1e-6, HEAD_DIM, out, rope, GRID), 2 * n)]
    for _, fn, _ in cases:
        fn()
    torch.cuda.synchronize()
    for rep in range(REPEATS):
        for name, fn, nbytes in cases:
            zp.copy_(keep)              # (in place feeds on its own output: start every window from the same rows)
            torch.cuda.synchronize()
            us = _timed(lambda: [fn() for _ in range(LAUNCHES)]) / LAUNCHES * 1e3
            print(json.dumps({'what': name, 'rows': ROWS, 'dim': DIM, 'repeat': rep, 'us': round(us, 1), 'bytes': nbytes,
                              'TB_per_s': round(nbytes / us / 1e6, 3), 'frac_of_copy_6.29': round(nbytes / us / 1e6 / COPY_TBS, 3),
                              'launches_timed': LAUNCHES, 'device': torch.cuda.get_device_name(dev)}), flush=True)


def step(dev):
    import wan
    from wan.configs import WAN_CONFIGS
    from wan.text2video import dit_seq_len
    from wan.utils.nag import NAG
    cfg = WAN_CONFIGS['t2v-14B']
    model = wan.modules.WanModel(dim=cfg.dim, ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, num_heads=cfg.num_heads, num_layers=cfg.num_layers,
                                 text_len=cfg.text_len, eps=cfg.eps, device=dev)
    model.init_weights(seed=0)
    model.eval().requires_grad_(False)
    gen = torch.Generator(device=dev).manual_seed(1)
    shape = (16, 21, 90, 160)           # 1280x720x81f through the VAE's (4, 8, 8) stride
    seq_len = dit_seq_len(*shape[1:], cfg.patch_size, 1)
    lat = torch.randn(*shape, device=dev, generator=gen)
    ctx = [torch.randn(512, 4096, device=dev, generator=gen).to(torch.bfloat16)]
    neg = [torch.randn(130, 4096, device=dev, generator=gen).to(torch.bfloat16)]
    t = torch.tensor([900], device=dev)
    nag = (NAG(4.0, 2.5, 0.5), neg)
    mixed = torch.empty_like(lat)

    def guided():
        cond, uncond = model.forward_pair([lat], t, ctx, neg, seq_len)
        ops.cfg_combine(mixed, uncond[0], cond[0], 5.0)
    kinds = [('cond-only step', lambda: model([lat], t=t, context=ctx, seq_len=seq_len)),
             ('cond-only step with NAG (4, 2.5, 0.5)', lambda: model([lat], t=t, context=ctx, seq_len=seq_len, nag=nag)),
             ('guided step (forward_pair + cfg_combine)', guided)]
    with torch.no_grad():
        for _, fn in kinds:
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _ in kinds}
        for rep in range(STEP_REPEATS):
            for name, fn in kinds:
                ms[name].append(_timed(fn))
                print(json.dumps({'what': name, 'workload': '14B T2V 1280x720x81f', 'tokens': seq_len, 'repeat': rep, 'ms': round(ms[name][-1], 1),
                                  'weights': 'random init (seed 0)', 'device': torch.cuda.get_device_name(dev)}), flush=True)
    base, with_nag, both = (min(ms[name]) for name, _ in kinds)
    print(json.dumps({'what': 'summary (the faster of the repeats)', 'cond_ms': round(base, 1), 'cond_nag_ms': round(with_nag, 1), 'guided_ms': round(both, 1),
                      'nag_over_cond': round(with_nag / base, 4), 'nag_over_guided': round(with_nag / both, 4),
                      'nag_extra_ms_per_block': round((with_nag - base) / cfg.num_layers, 3)}), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--skip-kernel', action='store_true')
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/nag_bench.py measures on the GPU: there is no CPU figure'
    device = torch.device('cuda:0')
    if not args.skip_kernel:
        kernel(device)
    if not args.skip_step:
        step(device)
