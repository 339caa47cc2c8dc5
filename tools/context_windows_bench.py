"""Context windows (WanT2V.generate(windows=)), measured.  One JSON line per figure.
    python tools/context_windows_bench.py kernels       the two passes at the metric's latent plane, C = 16, hw = 104 x 240, Fw = 21, F = 41, beside
                                                        mg_lincomb4_f32 with two terms on the window's element count (the same three accesses per
                                                        element as the blend), in one process, alternating, three repeats
    python tools/context_windows_bench.py steps         14B architecture, random-init weights, 1280x720: one denoising step (both guidance branches,
                                                        the blends, the mix; no scheduler update, no VAE) of an 81-frame clip and of a 161-frame clip
                                                        (latent F = 41) through ContextWindows(81, 16), two timed steps each, and the window passes alone
    python tools/context_windows_bench.py one-pass      the same step of the 161-frame clip in ONE DiT pass (147 600 tokens), a process of its own

kernels: device events around `rounds` passes over a ring of distinct tensors larger than the 256 MB last-level cache, so every launch reads its
inputs from HBM; bytes = what the algorithm has to move (gather: read and write the window; blend: read pred, read and write the window's frames of
acc — or only write them where `first` is set; lincomb: read two, write one).  The launches go back to back through the Python wrappers."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'moviigen1.1_amd'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
import torch  # noqa: E402
from wan.backend import ops  # noqa: E402
from wan.utils.context_windows import ContextWindows  # noqa: E402

COPY_TBS = 6.29
RING, ROUNDS, REPEATS = 6, 50, 3


def _timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def kernels(C=16, F=41, h=104, w=240):
    dev = torch.device('cuda:0')
    plan = ContextWindows(81, 16).plan(F)
    Fw, f0, k = plan.Fw, plan.starts[1], 1
    wk, first = plan.weights[k].to(dev), plan.first[k].to(dev)
    none, every = torch.zeros_like(first), torch.ones_like(first)
    gen = torch.Generator(device=dev).manual_seed(0)
    ring = []
    for _ in range(RING):               # 6 x (2 x 65.5 + 3 x 33.5) MB = 1.4 GB of distinct tensors
        ring.append(dict(x=torch.randn(C, F, h, w, device=dev, generator=gen), acc=torch.randn(C, F, h, w, device=dev, generator=gen),
                         pred=torch.randn(C, Fw, h, w, device=dev, generator=gen), win=torch.randn(C, Fw, h, w, device=dev, generator=gen),
                         out=torch.empty(C, Fw, h, w, device=dev)))
    nw = C * Fw * h * w
    n_first = int(first.sum().item())
    cases = [('mg_lincomb4_f32, two terms (the yardstick)', lambda t: ops.lincomb(t['out'], [(t['pred'], 0.5), (t['win'], 0.5)]), 3 * nw * 4),
             ('mg_window_gather_f32', lambda t: ops.window_gather(t['x'], f0, t['out']), 2 * nw * 4),
             ('mg_window_blend_f32, no frame first (fma: read pred, read and write acc)', lambda t: ops.window_blend(t['acc'], t['pred'], f0, wk, none), 3 * nw * 4),
             ('mg_window_blend_f32, every frame first (select: read pred, write acc)', lambda t: ops.window_blend(t['acc'], t['pred'], f0, wk, every), 2 * nw * 4),
             (f'mg_window_blend_f32, the plan\'s window 1 ({n_first} of {Fw} frames first)', lambda t: ops.window_blend(t['acc'], t['pred'], f0, wk, first),
              (3 * Fw - n_first) * C * h * w * 4)]
    for _, fn, _ in cases:              # warm up: every kernel launched, every tensor touched
        for t in ring:
            fn(t)
    torch.cuda.synchronize()
    for rep in range(REPEATS):          # the cases alternate: a drift of the box shows as a spread between the repeats
        for name, fn, nbytes in cases:
            us = _timed(lambda: [fn(t) for t in ring], ROUNDS) / RING * 1e3
            print(json.dumps({'what': name, 'C': C, 'F': F, 'hw': h * w, 'Fw': Fw, 'f0': f0, 'window_elements': nw, 'repeat': rep, 'us': round(us, 2),
                              'GB_per_s': round(nbytes / us / 1e3, 1), 'frac_of_copy_6.29': round(nbytes / us / 1e6 / COPY_TBS, 3),
                              'launches_timed': ROUNDS * RING, 'device': torch.cuda.get_device_name(dev)}), flush=True)


def _window_passes(plan, latent, run):
    """the passes one guided step adds: per window one gather and two blends (the DiT's outputs stand in as `run.lat`)"""
    for k, f0 in enumerate(plan.starts):
        ops.window_gather(latent, f0, run.lat)
        ops.window_blend(run.uncond, run.lat, f0, run.w[k], run.first[k])
        ops.window_blend(run.cond, run.lat, f0, run.w[k], run.first[k])


def steps(size=(1280, 720), timed=2, one_pass=False):
    import wan
    import weights as Wt
    from wan.configs import WAN_CONFIGS
    from wan.text2video import WindowRun
    dev = torch.device('cuda:0')
    cfg = WAN_CONFIGS['t2v-14B']
    model = wan.modules.WanModel(dim=cfg.dim, ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, num_heads=cfg.num_heads, num_layers=cfg.num_layers,
                                 text_len=cfg.text_len, eps=cfg.eps, device=dev)
    model.init_weights(seed=0)
    pipe = wan.WanT2V(cfg, checkpoint_dir=None, model=model, vae=wan.modules.WanVAE(state_dict=Wt.make_vae_params(8, 1), device=dev))
    gen = torch.Generator(device=dev).manual_seed(0)
    ctx = [torch.randn(512, 4096, device=dev, generator=gen)]
    ctx_null = [torch.randn(130, 4096, device=dev, generator=gen)]
    t = torch.tensor([999], device=dev)
    h, w = size[1] // cfg.vae_stride[1], size[0] // cfg.vae_stride[2]
    windows = ContextWindows(81, 16)
    lat21 = torch.randn(16, 21, h, w, device=dev, generator=gen)
    lat41 = torch.randn(16, 41, h, w, device=dev, generator=gen)
    plan = windows.plan(41)
    run = WindowRun(plan, lat41, True, pipe.patch_size, pipe.sp_size)
    pred = {21: torch.empty_like(lat21), 41: torch.empty_like(lat41)}

    def whole(latent):
        F = latent.shape[1]
        cond, uncond = pipe._guidance_pair(latent, t, ctx, ctx_null, F * (h // 2) * (w // 2))
        ops.cfg_combine(pred[F], uncond, cond, 5.0)

    def windowed():
        cond, uncond = pipe._window_predictions(run, lat41, t, ctx, ctx_null)
        ops.cfg_combine(pred[41], uncond, cond, 5.0)
    with torch.no_grad():
        whole(lat21)                    # warm up: every kernel launched, the prompt caches filled
        torch.cuda.synchronize()
        base = dict(size='%dx%d' % size, weights='random init (DiT seed 0)', timed_steps=timed, device=torch.cuda.get_device_name(dev))
        cases = [('81-frame clip, one pass', lambda: whole(lat21), 21), ('161-frame clip, ContextWindows(81, 16)', windowed, 41)]
        if one_pass:
            cases = [('161-frame clip, one pass', lambda: whole(lat41), 41)]
        for name, fn, F in cases:
            ms = [_timed(fn, 1) for _ in range(timed)]
            print(json.dumps(dict(base, what=name, latent_frames=F, windows=len(plan.starts) if fn is windowed else 1,
                                  window_starts=plan.starts if fn is windowed else [0], step_ms=[round(m, 1) for m in ms])), flush=True)
        if one_pass:
            return
        _window_passes(plan, lat41, run)
        torch.cuda.synchronize()
        us = [_timed(lambda: _window_passes(plan, lat41, run), 20) * 1e3 for _ in range(3)]
        print(json.dumps(dict(base, what='the window passes of one guided step alone: %d x (gather + 2 blends)' % len(plan.starts), latent_frames=41,
                              us=[round(u, 1) for u in us])), flush=True)


if __name__ == '__main__':
    {'kernels': kernels, 'steps': steps, 'one-pass': lambda: steps(one_pass=True)}[sys.argv[1] if len(sys.argv) > 1 else 'kernels']()
