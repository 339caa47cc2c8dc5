"""Calibrate the step cache on a checkpoint: the polynomial that maps a step's time-embedding distance to the change of
the DiT's output residual, for `generate.py --step_cache_coefficients` / `WanT2V.generate(step_cache={'coefficients': ...})`.

ONE full, uncached `generate` runs with the residual statistics on: every step computes (the video is the one step_cache=None gives)
and mg_step_resid_capture_f32 reduces sum |r_i - r_(i-1)| and sum |r_(i-1)| of the residual r = x_after_blocks - x_after_patch_embedding
while it stores r_i.  Step i's pair is

    ( d_i = sum |e_i - e_(i-1)| / sum |e_(i-1)|   of the time embedding (what the plan reads),
      o_i = sum |r_i - r_(i-1)| / sum |r_(i-1)|   summed over both guidance branches and, under sequence parallelism, all ranks )

The first step has no r_(i-1): its pair is left out.  numpy.polyfit(d, o, 4) gives the coefficients; with them the threshold of
`--step_cache` means "accumulated predicted relative change of the output residual since the last computed step".  The fit is only as
good as the weights it ran on: calibrate on the real checkpoint (random-init weights say nothing about quality).

usage: python tools/step_cache_calibrate.py --ckpt_dir ./MoviiGen1.1 [--size 1280*720] [--frame_num 81] [--prompt "..."] [--prompt_embeds FILE]
           [--sample_steps 50] [--sample_shift 5.0] [--sample_solver unipc] [--base_seed 0] [--source e0|e]      -> one JSON line on stdout
       (under torchrun with --ulysses_size N: the sums are added over the ranks; rank 0 prints)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'moviigen1.1_amd'))

import numpy as np  # noqa: E402


def calibrate(pipe, prompt, source='e0', degree=4, callback=None, **generate_kwargs):
    """run pipe.generate(prompt, **generate_kwargs) with every step computed and the residual statistics on ->
    {'coefficients': degree + 1 floats, highest power first; 'pairs': [(d_i, o_i)] and 'sums': [(sum |r_i - r_(i-1)|, sum |r_(i-1)|)] of the
    steps behind the first one that ran; 'steps': their schedule indices; 'source'}.  callback(i, latent) is passed on (it runs behind
    the step's statistics)."""
    import torch.distributed as dist
    from wan.utils.step_cache import step_distances
    model = pipe.model
    steps, sums = [], []

    def collect(i, latent):
        a = sum(v[0] for v in model.step_cache_stats.values())
        b = sum(v[1] for v in model.step_cache_stats.values())
        model.step_cache_stats.clear()
        steps.append(i)
        sums.append((a, b))
        if callback is not None:
            callback(i, latent)

    n = generate_kwargs.get('sampling_steps', 50)
    pipe.generate(prompt, callback=collect, step_cache={'plan': [True] * n, 'stats': True}, **generate_kwargs)
    if dist.is_initialized() and dist.get_world_size() > 1:
        # per-rank sums: token shards under sequence parallelism, one guidance branch each under cfg_parallel
        import torch
        t = torch.tensor(sums, dtype=torch.float64, device=pipe.device)
        dist.all_reduce(t)
        sums = [tuple(v) for v in t.tolist()]
    d = step_distances(model, pipe.last_step_timesteps, source)
    steps, sums = steps[1:], sums[1:]                       # the first step that ran has no previous residual
    if len(steps) < degree + 1:
        raise ValueError(f'a degree-{degree} fit needs {degree + 1} pairs: run at least {degree + 2} steps, got {len(steps) + 1}')
    pairs = [(float(d[i]), a / b) for i, (a, b) in zip(steps, sums)]
    coef = np.polyfit(np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]), degree)
    return {'coefficients': [float(c) for c in coef], 'pairs': pairs, 'sums': sums, 'steps': steps, 'source': source}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--ckpt_dir', required=True)
    ap.add_argument('--task', default='t2v-14B')
    ap.add_argument('--size', default='1280*720')
    ap.add_argument('--frame_num', type=int, default=81)
    ap.add_argument('--prompt', default='A cat walks on the grass, realistic style.')
    ap.add_argument('--prompt_embeds', default=None, help="torch file {'prompt','negative'} of umT5 embeddings, replaces the text encoder")
    ap.add_argument('--sample_steps', type=int, default=50)
    ap.add_argument('--sample_shift', type=float, default=5.0)
    ap.add_argument('--sample_solver', default='unipc', choices=['unipc', 'dpm++'])
    ap.add_argument('--sample_guide_scale', type=float, default=5.0)
    ap.add_argument('--base_seed', type=int, default=0)
    ap.add_argument('--source', default='e0', choices=['e0', 'e'])
    ap.add_argument('--ulysses_size', type=int, default=1)
    args = ap.parse_args()
    import torch
    import torch.distributed as dist
    import wan
    from wan.configs import SIZE_CONFIGS, WAN_CONFIGS
    rank, world, local = int(os.getenv('RANK', 0)), int(os.getenv('WORLD_SIZE', 1)), int(os.getenv('LOCAL_RANK', 0))
    if world > 1:
        torch.cuda.set_device(local)
        dist.init_process_group(backend='nccl', init_method='env://', rank=rank, world_size=world, device_id=torch.device(f'cuda:{local}'))
        assert args.ulysses_size == world, '--ulysses_size must equal the world size'
    pipe = wan.WanT2V(config=WAN_CONFIGS[args.task], checkpoint_dir=args.ckpt_dir, device_id=local, rank=rank, use_usp=args.ulysses_size > 1)
    prompt, n_prompt = args.prompt, ''
    if args.prompt_embeds:
        emb = torch.load(args.prompt_embeds, map_location='cpu', weights_only=True)
        prompt, n_prompt = emb['prompt'], emb['negative']
    out = calibrate(pipe, prompt, source=args.source, size=SIZE_CONFIGS[args.size], frame_num=args.frame_num, shift=args.sample_shift,
                    sample_solver=args.sample_solver, sampling_steps=args.sample_steps, guide_scale=args.sample_guide_scale, n_prompt=n_prompt,
                    seed=args.base_seed, offload_model=False)
    if rank == 0:
        out['step_cache_coefficients'] = ','.join(repr(c) for c in out['coefficients'])       # paste behind --step_cache_coefficients
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
