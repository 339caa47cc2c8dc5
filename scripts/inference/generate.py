"""Launcher with the flag set of the reference CLI (scripts/inference/generate.py:66-179; SURVEY.md
§8(f) rank 4): same names, defaults, validation messages, seed broadcast, offload default and output
file naming (generate.py:300-306), on the MI355X engine.

    python scripts/inference/generate.py --task t2v-14B --size 1280*720 --ckpt_dir ./MoviiGen1.1 \\
        --prompt "A cat walks on the grass, realistic style." --base_seed 42
    torchrun --nproc_per_node 8 --master-addr 127.0.0.1 scripts/inference/generate.py ... \\
        --dit_fsdp --t5_fsdp --ulysses_size 8          (the reference's inference.sh line)

Differences: no xfuser (sequence parallelism is built in; `--ulysses_size U` x `--ring_size R`
must equal the world size as in the reference), `--use_prompt_extend` is not built and says so,
`--t5_fsdp` / `--t5_cpu` are accepted (the 9.4 GB encoder is simply replicated on the GPU).  Extra:
`--cfg_parallel`, `--vae_parallel` (this engine's multi-GPU layouts),
`--init_video FILE` / `--strength F` (a video-to-video start, `WanT2V.generate(init_video=, strength=)`),
`--mask FILE` / `--keep_frames N` (with `--init_video`: masked video-to-video, `WanT2V.inpaint` — keep what the mask leaves out and / or
the first N frames, regenerate the rest),
`--lora PATH[:STRENGTH]` (repeatable: LoRA adapters merged into the DiT weights on the device, `WanModel.load_lora`),
`--step_cache THRESH` / `--step_cache_coefficients a,b,c,d,e` / `--step_cache_keep FIRST,LAST` (opt-in step cache,
`WanT2V.generate(step_cache=)`: steps whose time embedding has barely moved skip the DiT blocks and add the last computed step's
residual again; the coefficients come from `tools/step_cache_calibrate.py` on the real checkpoint — no threshold is recommended
without that calibration),
`--guide_interval LO,HI` / `--cfg_zero_star` / `--cfg_zero_init N` / `--guide_rescale PHI` (opt-in guidance options,
`WanT2V.generate(guidance=)`, DESIGN.md §3.8: both branches only while sigma lies in [LO, HI], CFG-Zero*'s projection and zero-init,
guidance rescale; no values are recommended),
`--context_frames N` / `--context_overlap M` / `--context_fuse pyramid|flat` (opt-in context windows, `WanT2V.generate(windows=)`,
DESIGN.md §3.9: a `--frame_num` longer than one DiT pass is denoised as a whole through overlapping windows of N frames; no values are
recommended),
`--nag_scale S` / `--nag_tau T` / `--nag_alpha A` / `--nag_negative TEXT` (opt-in normalized attention guidance, `WanT2V.generate(nag=)`,
DESIGN.md §3.11: a negative prompt that acts inside every cross-attention, also on steps that run the conditional branch alone — with
`--guide_interval 0,0` a negative prompt at one DiT forward per step; no values are recommended) and
`--prompt_embeds FILE` (a torch file {'prompt': [len,4096], 'negative': [len,4096]} instead of running
umT5 — for boxes without the tokenizer files)."""
import argparse
import logging
import os
import random
import sys
from datetime import datetime

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')   # before HIP initialises: see moviigen1.1_amd/wan/__init__.py

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'moviigen1.1_amd'))

import wan  # noqa: E402
from wan.configs import SIZE_CONFIGS, SUPPORTED_SIZES, WAN_CONFIGS  # noqa: E402
from wan.utils.utils import cache_image, cache_video, load_mask, load_video, str2bool  # noqa: E402

EXAMPLE_PROMPT = {   # one short default per task (the reference ships long showcase prompts here)
    't2v-14B': {'prompt': 'A cat walks on the grass, realistic style.'},
    't2i-14B': {'prompt': 'A snow-capped mountain above a quiet lake at dawn, wide-angle photograph.'},
}

# (flag, kwargs) in the reference's order
FLAGS = [
    ('--task', dict(type=str, default='t2v-14B', choices=list(WAN_CONFIGS.keys()), help='The task to run.')),
    ('--size', dict(type=str, default='1280*720', choices=list(SIZE_CONFIGS.keys()),
                    help='The area (width*height) of the generated video.')),
    ('--frame_num', dict(type=int, default=None, help='How many frames to sample. The number should be 4n+1')),
    ('--ckpt_dir', dict(type=str, default=None, help='The path to the checkpoint directory.')),
    ('--offload_model', dict(type=str2bool, default=None,
                             help='Whether to offload the model to CPU after the denoising loop.')),
    ('--ulysses_size', dict(type=int, default=1, help='The size of the ulysses parallelism in DiT.')),
    ('--ring_size', dict(type=int, default=1, help='The size of the ring attention parallelism in DiT.')),
    ('--t5_fsdp', dict(action='store_true', default=False, help='Whether to use FSDP for T5.')),
    ('--t5_cpu', dict(action='store_true', default=False, help='Whether to place T5 model on CPU.')),
    ('--dit_fsdp', dict(action='store_true', default=False, help='Whether to use FSDP for DiT.')),
    ('--save_file', dict(type=str, default=None, help='The file to save the generated image or video to.')),
    ('--prompt', dict(type=str, default=None, help='The prompt to generate the image or video from.')),
    ('--use_prompt_extend', dict(action='store_true', default=False, help='Whether to use prompt extend.')),
    ('--prompt_extend_model', dict(type=str, default='ZuluVision/MoviiGen1.1_Prompt_Rewriter', help='The prompt extend model to use.')),
    ('--prompt_extend_target_lang', dict(type=str, default='en', help='The target language of prompt extend.')),
    ('--base_seed', dict(type=int, default=-1, help='The seed to use for generating the image or video.')),
    ('--sample_solver', dict(type=str, default='unipc', choices=['unipc', 'dpm++'], help='The solver used to sample.')),
    ('--sample_steps', dict(type=int, default=None, help='The sampling steps.')),
    ('--sample_shift', dict(type=float, default=None, help='Sampling shift factor for flow matching schedulers.')),
    ('--sample_guide_scale', dict(type=float, default=5.0, help='Classifier free guidance scale.')),
    # this engine's additions
    ('--cfg_parallel', dict(action='store_true', default=False,
                            help='cond / uncond forwards on the two halves of an even number of ranks, Ulysses inside each half (not with --ring_size > 1).')),
    ('--vae_parallel', dict(nargs='?', const='spatial', default=False, choices=['spatial', 'pipeline'],
                            help='VAE decode over all ranks instead of rank 0 alone: spatial (default) = every rank decodes a band of image columns, '
                                 'pipeline = the decoder layers cut into one segment per rank.')),
    ('--dit_gemm', dict(type=str, default='bf16', choices=['bf16', 'mxfp8'],
                        help="arithmetic of the six per-block DiT linears: bf16 (the reference's) or mxfp8 (opt-in, block-scaled fp8 MFMA; not with --dit_fsdp).")),
    ('--init_video', dict(type=str, default=None,
                          help='video-to-video: start from this clip instead of pure noise (uint8 frames [T,H,W,3] as .npy, or any file imageio reads when it '
                               'is installed); resized to cover --size and centre-cropped. Not part of the reference CLI.')),
    ('--strength', dict(type=float, default=1.0, help='with --init_video: the fraction of the sampling schedule that runs, in (0, 1]; 1 = from pure noise.')),
    ('--mask', dict(type=str, default=None,
                    help='with --init_video: regenerate only where this mask is >= 128 and keep the rest of the clip (uint8 [T,H,W] or [H,W] as .npy, or any '
                         'file --init_video accepts: the maximum of its channels); it must have the frame size of --init_video.')),
    ('--keep_frames', dict(type=int, default=0, help='with --init_video: keep the first N frames of the clip and regenerate the rest (continuation).')),
    ('--lora', dict(type=str, action='append', default=None, metavar='PATH[:STRENGTH]',
                    help='a LoRA adapter (.safetensors: PEFT / diffusers or kohya / ComfyUI key names) merged into the DiT weights before sampling, '
                         'with an optional strength (default 1.0); may be given several times: all adapters are merged in one step, with one rounding.')),
    ('--step_cache', dict(type=float, default=None, metavar='THRESH',
                          help='opt-in step cache (TeaCache rule on the time embedding): a step is skipped while the accumulated predicted change since the '
                               'last computed step stays below THRESH (0 = every step computed). Not the reference arithmetic; off by default.')),
    ('--step_cache_coefficients', dict(type=str, default=None, metavar='a,b,c,d,e',
                                       help='with --step_cache: polynomial (highest power first, numpy.polyval) mapping the embedding distance to the '
                                            'predicted output change, as tools/step_cache_calibrate.py prints it; default 0,0,0,1,0 (the raw distance).')),
    ('--step_cache_keep', dict(type=str, default=None, metavar='FIRST,LAST',
                               help='with --step_cache: always compute the first FIRST and the last LAST steps (default 1,1).')),
    ('--guide_interval', dict(type=str, default=None, metavar='LO,HI',
                              help='opt-in guidance interval: both guidance branches run only while the noise level sigma of a step lies in [LO, HI] '
                                   '(0 <= LO <= HI <= 1); outside it only the conditional branch runs, one DiT forward instead of two. Not the reference '
                                   'arithmetic; off by default.')),
    ('--cfg_zero_star', dict(action='store_true', default=False,
                             help='opt-in CFG-Zero*: the unconditional prediction is rescaled by its projection <c,u>/|u|^2 before the guidance mix.')),
    ('--cfg_zero_init', dict(type=int, default=0, metavar='N', help='opt-in CFG-Zero* zero-init: the first N steps predict zero and run no DiT forward.')),
    ('--guide_rescale', dict(type=float, default=0.0, metavar='PHI',
                             help='opt-in guidance rescale: the guided prediction is pulled towards the standard deviation of the conditional one by '
                                  'PHI in [0, 1] (0 = off).')),
    ('--context_frames', dict(type=int, default=None, metavar='N',
                              help='opt-in context windows for a --frame_num longer than one DiT pass: the clip is denoised as a whole, the DiT sees '
                                   'it through overlapping windows of N frames (4n+1). Not the reference loop; off by default.')),
    ('--context_overlap', dict(type=int, default=16, metavar='M',
                               help='with --context_frames: the frames two neighbouring windows share (a multiple of 4, below N).')),
    ('--context_fuse', dict(type=str, default='pyramid', choices=['pyramid', 'flat'],
                            help='with --context_frames: the weight of a frame inside its window when overlapping predictions are blended.')),
    ('--nag_scale', dict(type=float, default=None, metavar='S',
                         help='opt-in normalized attention guidance: every cross-attention is pushed away from the negative prompt by S in [1, 64] '
                              '(one more short-key attention and one row-wise pass per block, no second DiT forward). Not the reference '
                              'arithmetic; off by default.')),
    ('--nag_tau', dict(type=float, default=None, metavar='T', help='with --nag_scale: the L1 norm of a pushed row is held at most T >= 1 times the '
                                                                   "positive row's (default 2.5, the paper's).")),
    ('--nag_alpha', dict(type=float, default=None, metavar='A', help='with --nag_scale: the weight A in [0, 1] of the pushed row in the blend with the '
                                                                     "positive one (default 0.25, the paper's).")),
    ('--nag_negative', dict(type=str, default=None, metavar='TEXT', help='with --nag_scale: the negative prompt of the attention guidance (default: the '
                                                                         "call's negative prompt).")),
    ('--prompt_embeds', dict(type=str, default=None, help="torch file {'prompt','negative'} of umT5 embeddings, replaces the text encoder.")),
]


def _lora_arg(arg):
    """'PATH' or 'PATH:STRENGTH' -> (path, strength).  Only a suffix that reads as a number is a strength: 'C:\\a.safetensors' and
    'dir:x/a.safetensors' are paths."""
    path, sep, tail = arg.rpartition(':')
    if sep and path:
        try:
            return path, float(tail)
        except ValueError:
            pass
    return arg, 1.0


def _step_cache_spec(args):
    """the three --step_cache* flags -> WanT2V.generate's `step_cache` argument (None without --step_cache)"""
    if args.step_cache is None:
        assert args.step_cache_coefficients is None and args.step_cache_keep is None, \
            '--step_cache_coefficients / --step_cache_keep need --step_cache'
        return None
    assert args.step_cache >= 0.0, f'--step_cache must be >= 0, got {args.step_cache}'      # (also refuses nan)
    spec = dict(thresh=args.step_cache)
    if args.step_cache_coefficients is not None:
        try:
            coef = [float(c) for c in args.step_cache_coefficients.split(',')]
        except ValueError:
            coef = []
        assert coef and all(c == c and abs(c) != float('inf') for c in coef), \
            f'--step_cache_coefficients must be finite numbers a,b,c,... (highest power first), got {args.step_cache_coefficients!r}'
        spec['coefficients'] = coef
    if args.step_cache_keep is not None:
        try:
            keep = [int(k) for k in args.step_cache_keep.split(',')]
        except ValueError:
            keep = []
        assert len(keep) == 2 and min(keep) >= 0, f'--step_cache_keep must be FIRST,LAST (two integers >= 0), got {args.step_cache_keep!r}'
        spec['keep_first'], spec['keep_last'] = keep
    return spec


def _guidance_spec(args):
    """the four guidance flags -> WanT2V.generate's `guidance` argument (None when none of them is given)"""
    if args.guide_interval is None and not args.cfg_zero_star and args.cfg_zero_init == 0 and args.guide_rescale == 0.0:
        return None
    from wan.utils.guidance import Guidance
    interval = (0.0, 1.0)
    if args.guide_interval is not None:
        try:
            interval = tuple(float(v) for v in args.guide_interval.split(','))
        except ValueError:
            interval = ()
        assert len(interval) == 2, f'--guide_interval must be LO,HI (two numbers), got {args.guide_interval!r}'
    try:
        return Guidance(interval=interval, zero_star=args.cfg_zero_star, zero_init_steps=args.cfg_zero_init, rescale=args.guide_rescale)
    except ValueError as e:
        raise AssertionError(f'--guide_interval / --cfg_zero_init / --guide_rescale: {e}') from None


def _nag_spec(args):
    """the four --nag_* flags -> WanT2V.generate's `nag` argument (None without --nag_scale)"""
    if args.nag_scale is None:
        assert args.nag_tau is None and args.nag_alpha is None and args.nag_negative is None, '--nag_tau / --nag_alpha / --nag_negative need --nag_scale'
        return None
    from wan.utils.nag import NAG
    kw = {k: v for k, v in (('tau', args.nag_tau), ('alpha', args.nag_alpha), ('n_prompt', args.nag_negative)) if v is not None}
    try:
        return NAG(args.nag_scale, **kw)
    except ValueError as e:
        raise AssertionError(f'--nag_scale / --nag_tau / --nag_alpha: {e}') from None


def _windows_spec(args):
    """the three --context_* flags -> WanT2V.generate's `windows` argument (None without --context_frames)"""
    if args.context_frames is None:
        return None
    from wan.utils.context_windows import ContextWindows
    try:
        windows = ContextWindows(frames=args.context_frames, overlap=args.context_overlap, fuse=args.context_fuse)
    except ValueError as e:
        raise AssertionError(f'--context_frames / --context_overlap / --context_fuse: {e}') from None
    assert args.step_cache is None, '--context_frames cannot be combined with --step_cache (the cached residuals would be per window)'
    return windows


def _validate_args(args):
    assert args.ckpt_dir is not None, 'Please specify the checkpoint directory.'
    assert args.task in WAN_CONFIGS, f'Unsupport task: {args.task}'
    assert args.task in EXAMPLE_PROMPT, f'Unsupport task: {args.task}'
    if args.sample_steps is None:
        args.sample_steps = 50
    if args.sample_shift is None:
        args.sample_shift = 5.0
    if args.frame_num is None:
        args.frame_num = 1 if 't2i' in args.task else 81
    if 't2i' in args.task:
        assert args.frame_num == 1, f'Unsupport frame_num {args.frame_num} for task {args.task}'
    args.base_seed = args.base_seed if args.base_seed >= 0 else random.randint(0, sys.maxsize)
    assert 0.0 < args.strength <= 1.0, f'--strength must be in (0, 1], got {args.strength}'
    assert args.init_video is not None or args.strength == 1.0, '--strength needs --init_video'
    assert args.init_video is not None or args.mask is None, '--mask needs --init_video'
    assert args.init_video is not None or args.keep_frames == 0, '--keep_frames needs --init_video'
    assert 0 <= args.keep_frames <= args.frame_num, f'--keep_frames must be in [0, {args.frame_num}], got {args.keep_frames}'
    args.lora = [_lora_arg(a) for a in args.lora or []]
    args.step_cache_spec = _step_cache_spec(args)
    args.guidance = _guidance_spec(args)
    args.windows = _windows_spec(args)
    args.nag = _nag_spec(args)
    assert args.size in SUPPORTED_SIZES[args.task], \
        f"Unsupport size {args.size} for task {args.task}, supported sizes are: {', '.join(SUPPORTED_SIZES[args.task])}"


def _parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Generate a image or video from a text prompt using Wan / MoviiGen1.1')
    for flag, kw in FLAGS:
        parser.add_argument(flag, **kw)
    args = parser.parse_args(argv)
    _validate_args(args)
    return args


def default_save_name(args, now=None):
    """reference generate.py:300-306."""
    stamp = (now or datetime.now()).strftime('%Y%m%d_%H%M%S')
    prompt = args.prompt.replace(' ', '_').replace('/', '_')[:50]
    size = args.size.replace('*', 'x') if sys.platform == 'win32' else args.size
    suffix = '.png' if 't2i' in args.task else '.mp4'
    return f'{args.task}_{size}_{args.ulysses_size}_{args.ring_size}_{prompt}_{stamp}' + suffix


def _init_logging(rank):
    if rank == 0:
        logging.basicConfig(level=logging.INFO, format='[%(asctime)s] %(levelname)s: %(message)s',
                            handlers=[logging.StreamHandler(stream=sys.stdout)])
    else:
        logging.basicConfig(level=logging.ERROR)


def generate(args):
    rank, world = int(os.getenv('RANK', 0)), int(os.getenv('WORLD_SIZE', 1))
    local = int(os.getenv('LOCAL_RANK', 0))
    _init_logging(rank)
    if args.offload_model is None:
        args.offload_model = world == 1
        logging.info(f'offload_model is not specified, set to {args.offload_model}.')
    if world > 1:
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        torch.cuda.set_device(local)
        dist.init_process_group(backend='nccl', init_method='env://', rank=rank, world_size=world,
                                device_id=torch.device(f'cuda:{local}'))
    else:
        assert not (args.t5_fsdp or args.dit_fsdp), \
            't5_fsdp and dit_fsdp are not supported in non-distributed environments.'
        assert not (args.ulysses_size > 1 or args.ring_size > 1), \
            'context parallel are not supported in non-distributed environments.'
    if args.ulysses_size > 1 or args.ring_size > 1:
        assert args.ulysses_size * args.ring_size == world, \
            'The number of ulysses_size and ring_size should be equal to the world size.'
    if args.use_prompt_extend:
        raise NotImplementedError('prompt extension (a 7B LLM rewriter) is outside this engine: pass the rewritten prompt')
    cfg = WAN_CONFIGS[args.task]
    if args.ulysses_size > 1:
        assert cfg.num_heads % args.ulysses_size == 0, \
            f'`{cfg.num_heads=}` cannot be divided evenly by `{args.ulysses_size=}`.'
    logging.info(f'Generation job args: {args}')
    logging.info(f'Generation model config: {cfg}')
    if dist.is_initialized():
        seed = [args.base_seed] if rank == 0 else [None]
        dist.broadcast_object_list(seed, src=0)
        args.base_seed = seed[0]
    if args.prompt is None:
        args.prompt = EXAMPLE_PROMPT[args.task]['prompt']
    logging.info(f'Input prompt: {args.prompt}')

    logging.info('Creating WanT2V pipeline.')
    pipe = wan.WanT2V(config=cfg, checkpoint_dir=args.ckpt_dir, device_id=local, rank=rank, t5_fsdp=args.t5_fsdp,
                      dit_fsdp=args.dit_fsdp, use_usp=(args.ulysses_size > 1 or args.ring_size > 1), t5_cpu=args.t5_cpu,
                      cfg_parallel=args.cfg_parallel, vae_parallel=args.vae_parallel, dit_gemm=args.dit_gemm,
                      lora=[p for p, _ in args.lora] or None, lora_strength=[s for _, s in args.lora] or 1.0,
                      sp_degrees=(args.ulysses_size, args.ring_size) if args.ring_size > 1 else None)
    prompt, n_prompt = args.prompt, ''
    if args.prompt_embeds:
        emb = torch.load(args.prompt_embeds, map_location='cpu', weights_only=True)
        prompt, n_prompt = emb['prompt'], emb['negative']
    logging.info(f"Generating {'image' if 't2i' in args.task else 'video'} ...")
    v2v = {}
    if args.init_video:         # every rank reads the file and encodes the clip for itself
        v2v = dict(init_video=load_video(args.init_video), strength=args.strength)
        logging.info(f"video-to-video start from {args.init_video}: {v2v['init_video'].shape[0]} frames, strength {args.strength}")
    if args.guidance is not None:       # (without a guidance flag the call is the one it was)
        v2v['guidance'] = args.guidance
        logging.info(f'guidance options: {args.guidance}')
    if args.windows is not None:        # (likewise)
        v2v['windows'] = args.windows
        logging.info(f'context windows: {args.windows}')
    if args.nag is not None:            # (likewise)
        v2v['nag'] = args.nag
        logging.info(f'normalized attention guidance: {args.nag}')
    run = pipe.generate
    if args.mask or args.keep_frames:       # masked video-to-video: the same call through WanT2V.inpaint
        v2v.update(mask=load_mask(args.mask) if args.mask else None, keep_frames=args.keep_frames)
        run = pipe.inpaint
        logging.info(f'inpaint: mask {args.mask}, the first {args.keep_frames} frames kept')
    video = run(prompt, size=SIZE_CONFIGS[args.size], frame_num=args.frame_num, shift=args.sample_shift,
                sample_solver=args.sample_solver, sampling_steps=args.sample_steps,
                guide_scale=args.sample_guide_scale, n_prompt=n_prompt, seed=args.base_seed,
                offload_model=args.offload_model, step_cache=args.step_cache_spec, **v2v)
    if pipe.last_step_plan is not None:
        logging.info('step cache: computed %d of %d steps: %s' % (sum(pipe.last_step_plan), len(pipe.last_step_plan),
                                                                   ''.join('C' if c else 's' for c in pipe.last_step_plan)))
    if getattr(pipe, 'last_guidance_plan', None) is not None:
        logging.info('guidance plan (z = zero, c = conditional branch only, G = both branches): ' + ''.join(
            {'zero': 'z', 'cond': 'c', 'guided': 'G'}[k] for k in pipe.last_guidance_plan))
    if getattr(pipe, 'last_window_plan', None) is not None:
        logging.info(f'context windows: {len(pipe.last_window_plan)} windows per step, starting at latent frames {pipe.last_window_plan}')
    if rank == 0:
        if args.save_file is None:
            args.save_file = default_save_name(args)
        if 't2i' in args.task:          # reference generate.py:308-315
            logging.info(f'Saving generated image to {args.save_file}')
            args.saved_as = cache_image(tensor=video.squeeze(1)[None], save_file=args.save_file, nrow=1,
                                        normalize=True, value_range=(-1, 1))
        else:
            logging.info(f'Saving generated video to {args.save_file}')
            args.saved_as = cache_video(tensor=video[None], save_file=args.save_file, fps=cfg.sample_fps, nrow=1,
                                        normalize=True, value_range=(-1, 1))
    logging.info('Finished.')
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    return args


if __name__ == '__main__':
    generate(_parse_args())
