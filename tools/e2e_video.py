"""One whole video through the drop-in surface, MEASURED end to end: WanT2V.generate(prompt string, size, frame_num = 81, sampling_steps = 50) of the 14B
architecture (reference wan/text2video.py:158-271) — text encoder (umT5-XXL, both prompts), 50 denoising steps (two guidance branches, CFG, UniPC), WanVAE
decode — plus the uint8 frames the writer gets (wan/utils/utils.py video_frames_uint8).  bench.py's `sec_per_video` is 50 x the measured step + the measured
decode; this is the call itself on the wall clock, so that the product of the two can be checked once per round.

Random-init weights of the shipped architectures (no checkpoint / tokenizer files in the image): the tokenizer is replaced by a word hash with the reference's
output contract (ids, mask of text_len 512); everything behind it is the product path.

usage: python tools/e2e_video.py [--workload 1080p|720p] [--steps 50] [--solver unipc] [--step_cache SPEC]      -> one JSON line on stdout
--step_cache (opt-in step cache): a threshold (a number), or an explicit plan of C (compute) / S (skip) letters, repeated to
--steps entries — `CS` = every other step.
--guide_interval LO,HI / --cfg_zero_star / --cfg_zero_init N / --guide_rescale PHI (opt-in guidance options): the launcher's flags; the
line then carries the median wall time of the 'guided', 'cond' and 'zero' steps separately.
--frame_num N / --context_frames N / --context_overlap M / --context_fuse pyramid|flat (opt-in context windows): a clip longer than one DiT
pass through the launcher's flags; the line then carries the window starts.
"""
import argparse
import importlib.util
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'moviigen1.1_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import torch  # noqa: E402

SAMPLING_FLAGS = ('--guide_interval', '--cfg_zero_star', '--cfg_zero_init', '--guide_rescale', '--context_frames', '--context_overlap', '--context_fuse')


def _launcher():
    """scripts/inference/generate.py as a module: the one definition of the sampling flags (FLAGS, _guidance_spec, _windows_spec)"""
    spec = importlib.util.spec_from_file_location('mg_generate_launcher', os.path.join(ROOT, 'scripts', 'inference', 'generate.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


class WordHashTokenizer:
    """the reference tokenizer's contract (wan/modules/tokenizers.py:61-82: ids [B, 512] padded with 0, mask) on a word hash: one id per whitespace word + </s>."""

    def __init__(self, seq_len=512, vocab=256384):
        self.seq_len, self.vocab = seq_len, vocab

    def __call__(self, texts, return_mask=True, add_special_tokens=True):
        ids = torch.zeros(len(texts), self.seq_len, dtype=torch.long)
        mask = torch.zeros(len(texts), self.seq_len, dtype=torch.long)
        for b, text in enumerate(texts):
            words = text.split()[:self.seq_len - 1]
            tok = [2 + zlib.crc32(w.encode()) % (self.vocab - 2) for w in words] + [1]
            ids[b, :len(tok)] = torch.tensor(tok)
            mask[b, :len(tok)] = 1
        return (ids, mask) if return_mask else ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='1080p', choices=['1080p', '720p'])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--solver', default='unipc', choices=['unipc', 'dpm++'])
    ap.add_argument('--prompt-words', type=int, default=511)
    ap.add_argument('--neg-words', type=int, default=129)
    ap.add_argument('--step_cache', default=None, help='threshold, or a plan of C / S letters repeated over the steps (CS = every other step)')
    ap.add_argument('--frame_num', type=int, default=81, help='frames of the clip (4n+1)')
    # the launcher's guidance and context-window (3.9) flags: its definitions, its validation
    launcher = _launcher()
    for flag, kw in launcher.FLAGS:
        if flag in SAMPLING_FLAGS:
            ap.add_argument(flag, **kw)
    args = ap.parse_args()
    guidance, windows = launcher._guidance_spec(args), launcher._windows_spec(args)
    extra = {} if windows is None else {'windows': windows}
    step_cache = None
    if args.step_cache is not None:
        pat = args.step_cache.upper()
        if pat and set(pat) <= {'C', 'S'}:
            step_cache = [pat[i % len(pat)] == 'C' for i in range(args.steps)]
        else:
            step_cache = float(args.step_cache)
    import wan
    import weights as Wt
    from wan.configs import WAN_CONFIGS
    from wan.modules.t5 import T5EncoderModel, umt5_xxl
    from wan.utils.utils import video_frames_uint8
    dev = torch.device('cuda:0')
    cfg = WAN_CONFIGS['t2v-14B']
    size = {'1080p': (1920, 832), '720p': (1280, 720)}[args.workload]
    t_build = time.perf_counter()
    model = wan.modules.WanModel(dim=cfg.dim, ffn_dim=cfg.ffn_dim, freq_dim=cfg.freq_dim, num_heads=cfg.num_heads, num_layers=cfg.num_layers,
                                 text_len=cfg.text_len, eps=cfg.eps, device=dev)
    model.init_weights(seed=0)
    vae = wan.modules.WanVAE(state_dict=Wt.make_vae_params(96, 1), device=dev)
    enc = umt5_xxl(device=dev)
    gt = torch.Generator(device=dev).manual_seed(0)
    for name, p in enc.named_parameters():
        if 'norm' in name:
            p.data.fill_(1.0)
        else:
            p.data.copy_(torch.randn(p.shape, generator=gt, device=dev, dtype=torch.float32).mul_(p.shape[-1] ** -0.5 * 0.5))
    text_encoder = T5EncoderModel(text_len=cfg.text_len, device=dev, model=enc.eval().requires_grad_(False), tokenizer=WordHashTokenizer(cfg.text_len))
    pipe = wan.WanT2V(cfg, checkpoint_dir=None, model=model, vae=vae, text_encoder=text_encoder)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t_build
    prompt = ' '.join(f'w{i}' for i in range(args.prompt_words))
    negative = ' '.join(f'n{i}' for i in range(args.neg_words))
    # one tiny call first: every kernel launched once, the prompt caches of THIS run stay cold (other prompts)
    pipe.generate('warm up', size=(64, 64), frame_num=5, sampling_steps=2, n_prompt='warm', seed=1, offload_model=False)
    torch.cuda.synchronize()
    marks = []

    def callback(i, latent):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append(ev)
    start = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    video = pipe.generate(prompt, size=size, frame_num=args.frame_num, sampling_steps=args.steps, sample_solver=args.solver, n_prompt=negative, seed=42,
                          offload_model=True, callback=callback, step_cache=step_cache, **({} if guidance is None else {'guidance': guidance}), **extra)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    t1 = time.perf_counter()
    frames = video_frames_uint8(video[None])
    torch.cuda.synchronize()
    u8_s = time.perf_counter() - t1
    assert tuple(video.shape) == (3, args.frame_num, size[1], size[0]) and torch.isfinite(video).all().item()
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (args.frame_num, size[1], size[0], 3)
    step_ms = [a.elapsed_time(b) for a, b in zip([start] + marks[:-1], marks)]
    mid = sorted(step_ms[1:])[len(step_ms[1:]) // 2] if len(step_ms) > 1 else step_ms[0]
    plan = pipe.last_step_plan
    med = lambda v: sorted(v)[len(v) // 2] if v else None      # noqa: E731
    by_kind = {} if plan is None else {     # a step as the loop sees it: the forward(s) + CFG + the scheduler update (step 0 left out: prompt caches)
        'median_computed_step_ms': med([m for m, c in list(zip(step_ms, plan))[1:] if c]),
        'median_skipped_step_ms': med([m for m, c in list(zip(step_ms, plan))[1:] if not c])}
    kinds = pipe.last_guidance_plan
    if kinds is not None:       # the wall time of a step by what the guidance plan made of it (step 0 left out as above)
        by_kind.update({f'median_{k}_step_ms': med([m for m, kk in list(zip(step_ms, kinds))[1:] if kk == k]) for k in ('guided', 'cond', 'zero')})
        by_kind.update({'guidance': repr(guidance), 'guidance_plan': ''.join({'zero': 'z', 'cond': 'c', 'guided': 'G'}[k] for k in kinds),
                        'step_ms': [round(m, 1) for m in step_ms]})
    if pipe.last_window_plan is not None:
        by_kind.update({'windows': repr(extra['windows']), 'window_starts': pipe.last_window_plan})
    line = {'what':'WanT2V.generate end to end (tools/e2e_video.py): text encoder x 2 prompts + %d denoising steps (two guidance branches through WanModel.forward_pair, CFG 5.0, %s) '
                    '+ WanVAE.decode, offload_model=True (the reference default), one call on the wall clock' % (args.steps, args.solver),
            'workload': '14B T2V %dx%dx%df' % (size + (args.frame_num,)), 'sampling_steps': args.steps,
            'step_cache': args.step_cache, **by_kind, 'steps_computed': sum(pipe.last_step_plan) if pipe.last_step_plan is not None else args.steps, 'sec_per_video_measured': wall,
            'first_step_ms_incl_text_encoder_and_prompt_caches': step_ms[0], 'median_later_step_ms': mid, 'sum_steps_s': sum(step_ms) / 1e3,
            'after_last_step_s_vae_decode_and_teardown': wall - sum(step_ms) / 1e3, 'uint8_frames_s_not_included': u8_s,
            'prompt_tokens': [args.prompt_words + 1, args.neg_words + 1], 'weights': 'random init (DiT seed 0, dim-96 WanVAE, umT5-XXL)', 'data': 'synthetic',
            'model_build_s_not_included': build_s, 'video_abs_max': video.abs().max().item(), 'device': torch.cuda.get_device_name(dev)}
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
