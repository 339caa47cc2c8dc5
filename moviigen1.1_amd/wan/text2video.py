"""WanT2V — the drop-in pipeline surface (reference wan/text2video.py:28-271).

Same constructor and `generate()` signature, defaults and return contract
(Tensor[3, frame_num, H, W] fp32 in [-1,1] on rank 0, None elsewhere).  What runs underneath is
the MI355X engine: WanModel (HIP kernels), the fused-update schedulers, WanVAE (HIP kernels),
Ulysses over RCCL when `use_usp`, block-sharded weights when `dit_fsdp`.

The umT5-XXL text encoder (wan/modules/t5.py on the same HIP kernels) is
created from `checkpoint_dir/config.t5_checkpoint` as in the reference when that file exists;
`text_encoder=` injects any callable with T5EncoderModel's contract (prompt list, device) -> list
of `[len<=512, 4096]` tensors, and `input_prompt` / `n_prompt` may also be pre-computed embeddings.
"""
import contextlib
import gc
import inspect
import logging
import math
import os
import random
import sys

import torch
import torch.distributed as dist

from .backend import ops
from .modules.model import WanModel
from .modules.vae import WanVAE
from .utils.fm_solvers import FlowDPMSolverMultistepScheduler, get_sampling_sigmas, retrieve_timesteps
from .utils.fm_solvers_unipc import FlowUniPCMultistepScheduler
from .utils.context_windows import ContextWindows
from .utils.guidance import Guidance
from .utils.nag import NAG
from .utils.sample_plan import refuse_windows_with_step_cache, sample_plan
from .utils.step_cache import resolve_plan


def v2v_steps(sampling_steps, strength):
    """(n_run, i0) of a video-to-video start: the last n_run = min(max(int(sampling_steps * strength), 1), sampling_steps) steps of the
    schedule run, beginning at index i0 = sampling_steps - n_run (the img2img convention); 0 < strength <= 1."""
    if not 0.0 < float(strength) <= 1.0:
        raise ValueError(f'strength must be in (0, 1], got {strength!r}')
    n_run = min(max(int(sampling_steps * float(strength)), 1), sampling_steps)
    return n_run, sampling_steps - n_run


class MaskedEdit:
    """what `WanT2V.inpaint` carries through the sampling loop: the pixel mask pm [T, H, W] and the latent-grid mask lm (uint8, 1 = regenerate,
    0 = keep), and, filled in by `start_latent(keep=)`, the source clip and its encoding z0."""

    def __init__(self, pm, lm):
        self.pm, self.lm, self.clip, self.z0 = pm, lm, None, None


def _checked_guidance(guidance):
    if guidance is not None and not isinstance(guidance, Guidance):
        raise ValueError(f'guidance must be None or a wan.utils.guidance.Guidance, got {guidance!r}')
    return guidance


def _checked_windows(windows):
    if windows is not None and not isinstance(windows, ContextWindows):
        raise ValueError(f'windows must be None or a wan.utils.context_windows.ContextWindows, got {windows!r}')
    return windows


def _checked_nag(nag, model=None):
    """nag must be None or a NAG; given a model, that model's forward must take the `nag` keyword (a user's own `model=` may not)"""
    if nag is not None and not isinstance(nag, NAG):
        raise ValueError(f'nag must be None or a wan.utils.nag.NAG, got {nag!r}')
    if nag is not None and model is not None:
        fwd = getattr(model, 'forward', model)
        try:
            params = inspect.signature(fwd).parameters
        except (TypeError, ValueError):
            params = {}
        if 'nag' not in params:
            raise ValueError(f'nag needs a model whose forward takes the `nag` keyword (wan.modules.WanModel); {type(model).__name__} does not')
    return nag


def dit_seq_len(frames, h, w, patch_size, sp_size):
    """the DiT's seq_len for a latent [C, frames, h, w]: its tokens, rounded up to a multiple of the sequence-parallel degree"""
    return math.ceil((h * w) / (patch_size[1] * patch_size[2]) * frames / sp_size) * sp_size


class WindowRun:
    """what a `generate` call with context windows allocates once and every step reuses: the plan (a WindowPlan), the gather buffer `lat`
    [C, Fw, h, w], the whole-clip predictions `cond` and `uncond` [C, F, h, w] (uncond: None when no step of the call runs both branches),
    the per-window weights `w` [K, Fw] fp32 and first-cover flags `first` [K, Fw] uint8 on the device, and the DiT's seq_len of ONE window."""

    def __init__(self, plan, latent, both, patch_size, sp_size):
        C, _, h, w = latent.shape
        self.plan = plan
        self.lat = latent.new_empty(C, plan.Fw, h, w)
        self.cond = torch.empty_like(latent)
        self.uncond = torch.empty_like(latent) if both else None
        self.w, self.first = plan.weights.to(latent.device), plan.first.to(latent.device)
        self.seq_len = dit_seq_len(plan.Fw, h, w, patch_size, sp_size)


class GuidedMix:
    """the mix of a call's 'guided' steps, built once per call: the effective guide scale (the Guidance's when it has one, else the call's
    `guide_scale`) and, only when the three-launch form will run (CFG-Zero* or rescale on, and some step is 'guided'), its scratch: the five
    fp64 sums `stats`, the per-workgroup `partials` and the two fp32 coefficients `coef`.  mix(out, uncond, cond) -> out, no host read."""

    def __init__(self, guidance, guide_scale, any_guided, device):
        self.scale = guide_scale if guidance is None or guidance.scale is None else guidance.scale
        self.guidance = guidance
        self.stats = self.partials = self.coef = None
        if guidance is not None and not guidance.plain_mix and any_guided:
            self.stats = torch.empty(5, dtype=torch.float64, device=device)
            self.partials = ops.cfg_stats_partials(device)
            self.coef = torch.empty(2, dtype=torch.float32, device=device)

    def __call__(self, out, uncond, cond):
        if self.stats is None:          # the reference's u + g (c - u)
            ops.cfg_combine(out, uncond, cond, self.scale)
        else:                           # CFG-Zero* / rescale: five fp64 sums, two coefficients, the mix
            ops.cfg_stats(uncond, cond, self.stats, self.partials)
            ops.cfg_coefficients(self.stats, out.numel(), self.scale, self.guidance.zero_star, self.guidance.rescale, self.coef)
            ops.cfg_combine_coef(out, uncond, cond, self.coef)
        return out


class WanT2V:

    def __init__(self, config, checkpoint_dir, device_id=0, rank=0, t5_fsdp=False, dit_fsdp=False, use_usp=False,
                 t5_cpu=False, text_encoder=None, model=None, vae=None, cfg_parallel=False, vae_parallel=False, use_ring=False, sp_degrees=None,
                 dit_gemm='bf16', step_cache=None, guidance=None, windows=None, nag=None, lora=None, lora_strength=1.0):
        _checked_guidance(guidance)
        _checked_windows(windows)
        _checked_nag(nag)
        self.device = torch.device(f'cuda:{device_id}')
        self.config = config
        self.rank = rank
        self.t5_cpu = t5_cpu
        self.num_train_timesteps = config.num_train_timesteps
        self.param_dtype = config.param_dtype
        if t5_fsdp or t5_cpu:   # both only trade memory for time in the reference; the outputs are the same
            logging.info('t5_fsdp / t5_cpu: the 9.4 GB bf16 text encoder is kept whole on the GPU (288 GB HBM)')
        t5_path = os.path.join(checkpoint_dir, config.t5_checkpoint) if checkpoint_dir else None
        if text_encoder is None and t5_path and os.path.exists(t5_path):
            from .modules.t5 import T5EncoderModel
            text_encoder = T5EncoderModel(text_len=config.text_len, dtype=config.t5_dtype, device=self.device,
                                          checkpoint_path=t5_path,
                                          tokenizer_path=os.path.join(checkpoint_dir, config.t5_tokenizer))
        self.text_encoder = text_encoder
        self.vae_stride = config.vae_stride
        self.patch_size = config.patch_size
        self.vae = vae if vae is not None else WanVAE(
            vae_pth=os.path.join(checkpoint_dir, config.vae_checkpoint), device=self.device)
        if model is None:
            logging.info(f'Creating WanModel from {checkpoint_dir}')
            model = WanModel.from_pretrained(checkpoint_dir)
        self.model = model
        self.model.eval().requires_grad_(False)
        if dist.is_initialized():
            dist.barrier()
        self.model.to(self.device)
        # LoRA adapters (one `.safetensors` path / dict of tensors or a list, one strength or one per adapter) are merged into the resident
        # weights here: before they are block-sharded and before 'mxfp8' quantises them (WanModel.load_lora).  None touches nothing
        if lora is not None:
            self.model.load_lora(lora, strength=lora_strength)
        self.cfgp = None
        self.vae_parallel = bool(vae_parallel) and dist.is_initialized() and dist.get_world_size() > 1
        # vae_parallel: True / 'spatial' = every rank decodes its band of image columns (WanVAE.decode_spatial); 'pipeline' = the layer pipeline
        self.vae_parallel_kind = vae_parallel if vae_parallel in ('spatial', 'pipeline') else 'spatial'
        # flag combinations are validated BEFORE any process group is created
        U, R = sp_degrees or (1, 1)                                 # the reference CLI's (ulysses_size, ring_size)
        want_ring = bool(use_ring or R > 1)
        if cfg_parallel and want_ring:
            raise NotImplementedError('cfg_parallel is built on plain Ulysses groups (no ring / hybrid layout)')
        if cfg_parallel and not (dist.is_initialized() and dist.get_world_size() % 2 == 0):
            logging.warning('cfg_parallel needs an even number of ranks under torch.distributed: ignored, both CFG '
                            'forwards run on every rank')
            cfg_parallel = False
        if cfg_parallel:
            # cond / uncond halves of the ranks, Ulysses inside each half when it has more than one rank
            # (wan/distributed/cfg_parallel.py) — independent of use_usp: 2 ranks need no sequence parallelism at all
            from .distributed.cfg_parallel import enable_cfg_parallel
            self.cfgp = enable_cfg_parallel(self.model)
        elif use_usp:
            from .distributed.ring import enable_hybrid_sp, enable_ring_attention
            from .distributed.xdit_context_parallel import enable_sequence_parallel
            if U > 1 and R > 1:
                enable_hybrid_sp(self.model, U, R)
            elif want_ring:
                enable_ring_attention(self.model)
            else:
                enable_sequence_parallel(self.model)
        self.sp_size = self.model.sp_size
        if dit_fsdp:
            from .distributed.fsdp import shard_model
            self.model = shard_model(self.model, device_id=device_id)
        # 'mxfp8' = the six per-block linears on the block-scaled fp8 MFMA (WanModel.set_gemm_precision): opt-in, raises with dit_fsdp
        if dit_gemm != 'bf16':      # the default leaves a caller-supplied `model=` object untouched
            self.model.set_gemm_precision(dit_gemm)
        self.sample_neg_prompt = config.sample_neg_prompt
        # the object's default for generate(step_cache=): None = every step runs the blocks (the reference's loop)
        self.step_cache = step_cache
        self.last_step_plan = self.last_step_timesteps = None
        # the object's default for generate(guidance=): None = both branches in every step, mixed as u + g (c - u) (the reference's loop)
        self.guidance = guidance
        self.last_guidance_plan = None
        # the object's default for generate(windows=): None = the whole latent in one DiT pass (the reference's loop)
        self.windows = windows
        self.last_window_plan = None
        # the object's default for generate(nag=): None = the cross-attention as it is (the reference's)
        self.nag = nag
        self.last_nag = None

    def _encode(self, prompt):
        if torch.is_tensor(prompt):
            return [prompt.to(self.device)]
        if isinstance(prompt, (list, tuple)) and prompt and torch.is_tensor(prompt[0]):
            return [p.to(self.device) for p in prompt]
        if self.text_encoder is None:
            raise FileNotFoundError(
                'no text encoder: config.t5_checkpoint not found in the checkpoint dir; pass pre-computed '
                'umT5 embeddings ([len<=512, 4096] tensors) as `input_prompt`/`n_prompt`, or '
                'WanT2V(text_encoder=callable)')
        return [t.to(self.device) for t in self.text_encoder([prompt], self.device)]

    def init_clip(self, init_video, size, frame_num):
        """`generate`'s init_video -> the clip [3, frame_num, size[1], size[0]] fp32 in [-1, 1] on the device."""
        if not torch.is_tensor(init_video):
            init_video = torch.as_tensor(init_video)
        W_, H_ = size
        if init_video.dim() != 4:
            raise ValueError(f'init_video must be uint8 frames [T, H0, W0, 3] or a float clip [3, T, H, W], got {tuple(init_video.shape)}')
        if init_video.dtype == torch.uint8:
            if init_video.shape[3] != 3 or init_video.shape[0] < frame_num:
                raise ValueError(f'init_video: uint8 frames must be [T >= {frame_num}, H0, W0, 3], got {tuple(init_video.shape)}')
            return ops.video_from_u8(init_video[:frame_num].to(self.device).contiguous(), H_, W_)
        if not init_video.is_floating_point() or init_video.shape[0] != 3 or init_video.shape[1] < frame_num or tuple(init_video.shape[2:]) != (H_, W_):
            raise ValueError(f'init_video: a float clip must be [3, T >= {frame_num}, {H_}, {W_}] (already at `size`), got {init_video.dtype} '
                             f'{tuple(init_video.shape)}')
        return init_video[:, :frame_num].to(self.device, torch.float32).contiguous()

    def start_latent(self, init_video, size, frame_num, noise, sigma, keep=None):
        """the latent a video-to-video run starts from: (1 - sigma) z0 + sigma noise with z0 = vae.encode(init_clip(init_video)), one fused launch.
        keep: a MaskedEdit that receives the clip and z0 (a masked run reads both again; nothing is encoded twice)."""
        clip = self.init_clip(init_video, size, frame_num)
        z0 = self.vae.encode([clip])[0]
        if keep is not None:
            keep.clip, keep.z0 = clip, z0
        if tuple(z0.shape) != tuple(noise.shape):
            raise ValueError(f'init_video encodes to {tuple(z0.shape)}, the latent of this call is {tuple(noise.shape)}')
        # (also what makes the strength-1 start exact: 0 x finite = 0, and 0 + 1 x noise = noise)
        assert torch.isfinite(z0).all().item(), 'the encoded init_video is not finite'
        return ops.lincomb(torch.empty_like(noise), [(z0, 1.0 - sigma), (noise, sigma)])

    def _guidance_pair(self, latent, t, context, context_null, seq_len, nag=None):
        """(cond, uncond) noise predictions of one denoising step; nag: None, or what WanModel.forward(nag=) takes, for every forward of
        the conditional context (the unconditional one runs plain)"""
        kw = {} if nag is None else {'nag': nag}        # (None: the calls as they were, also for a model object without the keyword)
        pair = getattr(self.model, 'forward_pair', None)
        if self.cfgp is None and pair is not None:
            # both branches in one call: what they share (everything in front of block 0's cross-attention) is computed once,
            # the results are those of the two calls below bit for bit (WanModel.forward_pair)
            cond, uncond = pair([latent], t, context, context_null, seq_len, **kw)
            return cond[0], uncond[0]
        if self.cfgp is None:      # a model object without forward_pair: the reference's two calls (text2video.py:237-240)
            cond = self.model([latent], t=t, context=context, seq_len=seq_len, **kw)[0]
            uncond = self.model([latent], t=t, context=context_null, seq_len=seq_len)[0]
            return cond, uncond
        # this half's branch only, then swap predictions with the partner rank
        if self.cfgp.branch:
            mine = self.model([latent], t=t, context=context_null, seq_len=seq_len)[0]
        else:
            mine = self.model([latent], t=t, context=context, seq_len=seq_len, **kw)[0]
        return self.cfgp.exchange(mine)

    def _cond_prediction(self, latent, t, context, seq_len, nag=None):
        """the conditional branch alone, of a step outside the guidance interval: ONE forward — the call whose bits forward_pair promises for
        its cond half.  Under cfg_parallel both halves of the ranks run it (each its own Ulysses group) and nothing is exchanged."""
        kw = {} if nag is None else {'nag': nag}
        return self.model([latent], t=t, context=context, seq_len=seq_len, **kw)[0]

    def _window_predictions(self, run, latent, t, context, context_null, nag=None):
        """the whole-clip (cond, uncond) predictions of one step through context windows (`run`: the call's WindowRun): every window in
        ascending order is cut out of the latent, predicted on its own at positions 0 .. Fw - 1 and blended into the whole-clip buffers.
        context_null None: the conditional branch alone (a 'cond' step) -> (cond, None).  No host read.  nag: one for every window."""
        kw = {} if nag is None else {'nag': nag}
        for k, f0 in enumerate(run.plan.starts):
            ops.window_gather(latent, f0, run.lat)
            if context_null is None:
                cond, uncond = self._cond_prediction(run.lat, t, context, run.seq_len, **kw), None
            else:
                cond, uncond = self._guidance_pair(run.lat, t, context, context_null, run.seq_len, **kw)
                ops.window_blend(run.uncond, uncond, f0, run.w[k], run.first[k])
            ops.window_blend(run.cond, cond, f0, run.w[k], run.first[k])
        return run.cond, None if context_null is None else run.uncond

    def _predictions(self, kind, latent, t, context, context_null, seq_len, wrun, nag=None):
        """(cond, uncond) of a 'guided' step, (cond, None) of a 'cond' step — the one call the sampling loop makes for a forward; wrun: the
        call's WindowRun, None = the whole latent in one pass; nag: None, or (NAG, [negative context]) for the conditional forwards"""
        kw = {} if nag is None else {'nag': nag}
        if wrun is not None:
            return self._window_predictions(wrun, latent, t, context, context_null if kind == 'guided' else None, **kw)
        if kind == 'guided':
            return self._guidance_pair(latent, t, context, context_null, seq_len, **kw)
        return self._cond_prediction(latent, t, context, seq_len, **kw), None

    def _scheduler(self, sample_solver, sampling_steps, shift):
        """-> (scheduler, timesteps on the device) of the reference's two solvers (text2video.py:186-207)"""
        if sample_solver == 'unipc':
            sample_scheduler = FlowUniPCMultistepScheduler(
                num_train_timesteps=self.num_train_timesteps, shift=1, use_dynamic_shifting=False)
            sample_scheduler.set_timesteps(sampling_steps, device=self.device, shift=shift)
            return sample_scheduler, sample_scheduler.timesteps
        if sample_solver == 'dpm++':
            sample_scheduler = FlowDPMSolverMultistepScheduler(
                num_train_timesteps=self.num_train_timesteps, shift=1, use_dynamic_shifting=False)
            sampling_sigmas = get_sampling_sigmas(sampling_steps, shift)
            timesteps, _ = retrieve_timesteps(sample_scheduler, device=self.device, sigmas=sampling_sigmas)
            return sample_scheduler, timesteps
        raise NotImplementedError("Unsupported solver.")

    def _decode(self, x0, target_shape, offload_model):
        """VAE decode of the final latent -> videos (None off rank 0), with the offload policy in front of it and one retry behind it;
        sets self.last_offloaded: did the DiT's weights go to the host?"""
        offloaded = False
        if offload_model:
            # reference text2video.py:257-259 moves the DiT to the host before the VAE decode to make room on an
            # 80 GB device.  Here that is 28 GB over PCIe and back on the next call, for nothing, whenever the decode
            # fits beside the resident model — which it does on 288 GB: the flag then only drops the DiT's activation
            # workspace; the weights move only when the free memory would not hold 1.25 x the decode's estimated peak
            # (MOVIIGEN_FORCE_OFFLOAD=1 restores the reference's unconditional move), and a decode that still runs out
            # of memory is retried once with the DiT on the host.
            self.model._ws = {}
            torch.cuda.empty_cache()
            free_b, _ = torch.cuda.mem_get_info(self.device)
            need_b = self.vae.decode_peak_bytes(target_shape) if hasattr(self.vae, 'decode_peak_bytes') else 32 << 30
            need_b = need_b * 5 // 4
            if os.environ.get('MOVIIGEN_FORCE_OFFLOAD') == '1':
                need_b = free_b + 1
            if free_b > need_b:
                logging.info(f'offload_model: {free_b / 2**30:.0f} GiB free >= {need_b / 2**30:.0f} GiB for the VAE decode '
                             '-> the DiT stays resident (nothing is moved to the host)')
            else:
                self.model.cpu()
                torch.cuda.empty_cache()
                offloaded = True

        def decode():
            if self.vae_parallel:    # multi-GPU decode over all ranks, video assembled on rank 0: W bands (default), or the layer pipeline
                out = self.vae.decode_pipelined(x0) if self.vae_parallel_kind == 'pipeline' else self.vae.decode_spatial(x0)
                return out if self.rank == 0 else None
            return self.vae.decode(x0) if self.rank == 0 else None
        retry = False
        try:
            videos = decode()
        except torch.cuda.OutOfMemoryError:
            if not offload_model or offloaded or self.vae_parallel:      # (pipelined decode: one rank retrying alone would leave its peers in their send / recv)
                raise
            retry = True       # decided here, done BELOW: inside the handler the live exception's traceback still holds the failed decode's
            #                    frames — its multi-GB fp32 activations — and neither model.cpu() nor empty_cache() could free them
        if retry:
            logging.warning('offload_model: the VAE decode ran out of memory beside the resident DiT -> moving the '
                            'DiT to the host (reference text2video.py:257-259) and decoding again')
            gc.collect()
            self.model.cpu()
            torch.cuda.empty_cache()
            offloaded = True
            videos = decode()
        self.last_offloaded = offloaded
        return videos

    def generate(self, input_prompt, size=(1280, 720), frame_num=81, shift=5.0, sample_solver='unipc',
                 sampling_steps=50, guide_scale=5.0, n_prompt="", seed=-1, offload_model=True,
                 noise=None, callback=None, step_cache=None, guidance=None, windows=None, nag=None, init_video=None, strength=1.0):
        """The reference's `generate` (text2video.py:114-271), plus a video-to-video start and a step cache that are NOT part of the reference:

        init_video: an existing clip to start from instead of pure noise — uint8 RGB frames [T, H0, W0, 3] of any size (tensor or array;
            resized to cover `size` and centre-cropped on the GPU, ops.video_from_u8) or a float clip [3, T, H, W] in [-1, 1] already at
            `size`; T >= frame_num, the first frame_num frames are used.
        strength in (0, 1]: how much of the schedule runs (`v2v_steps`).  The clip is encoded (`vae.encode`, on every rank for itself: the
            same bits everywhere, no collective), the start latent is (1 - sigma) z0 + sigma noise at the sigma of schedule index i0 and the
            loop runs the steps i0 .. sampling_steps - 1; `callback(i, latent)` gets these schedule indices.  At strength 1 the start is
            0 z0 + 1 noise: the result is bit-identical to the call without init_video and the same noise.
        Without init_video nothing changes, call for call.

        step_cache (default: the object's, WanT2V(step_cache=); None = off): skip the DiT blocks of some steps and add the residual of the
            last computed step again (WanModel.step_cache; TeaCache's rule on the time embedding) — a float threshold,
            a dict of wan.utils.step_cache.step_cache_plan's arguments (thresh, coefficients, source, keep_first, keep_last), or an
            explicit plan: one bool per schedule index, True = compute.  The plan is a function of the timesteps and the weights only:
            known before the loop, the same on every rank and for both guidance branches.  The first step that runs is always computed.
            `self.last_step_plan` holds the plan of the last call (None without a step cache); the residuals are dropped when the loop ends.
            Threshold 0 and an all-True plan give the bits of step_cache=None.

        guidance (default: the object's, WanT2V(guidance=); None = off, the loop above call for call): a wan.utils.guidance.Guidance —
            which steps run both branches and how the two predictions are mixed.  Its plan, one of 'zero' | 'cond' |
            'guided' per schedule index, is a function of the schedule alone (`self.last_guidance_plan`; None without a Guidance):
            'zero' (CFG-Zero*'s zero-init): no forward, the prediction is zero; 'cond' (outside the guidance interval): ONE forward, the
            conditional branch, and its prediction is used as it is — under cfg_parallel both halves run it and nothing is exchanged;
            'guided': both branches, mixed as u + g (c - u) by mg_cfg_combine_f32 when neither zero_star nor rescale is on
            (Guidance(scale=g) alone gives the bits of guide_scale=g), else by the three launches cfg_stats -> cfg_coefficients ->
            cfg_combine_coef on scratch allocated once per call, every rank on its whole latent (no collective, no host read).
            With a step cache the residuals are per context, so a 'guided' step is computed when the last step that ran a forward was not
            'guided', and the first step that runs a forward is computed; `last_step_plan` holds the plan so adjusted.

        windows (default: the object's, WanT2V(windows=); None = off, the loop above call for call): a wan.utils.context_windows.ContextWindows
            — a clip longer than one DiT pass.  The latent is denoised as a whole; in every step each window of Fw latent
            frames (ascending starts, `self.last_window_plan`; None without windows or when the clip fits one window, which is the loop
            above call for call) is cut out (ops.window_gather), predicted on its own at positions 0 .. Fw - 1 with the window's seq_len,
            and blended with its per-frame weights into whole-clip cond / uncond buffers (ops.window_blend); the guidance mix above then runs
            ONCE on the whole-clip buffers, so the statistics of CFG-Zero* / rescale are over the whole clip.  A 'cond' step runs one
            forward per window, a 'zero' step none.  Scheduler step, masked_renoise, `callback(i, whole latent)`, decode and composite are
            unchanged: init_video, strength and `inpaint` work at any length.  The buffers and the device copies of the weights are
            allocated once per call; no host read in the loop.  Not together with a step cache (its residuals would be per window):
            ValueError before any forward.

        nag (default: the object's, WanT2V(nag=); None = off, the loop above call for call): a wan.utils.nag.NAG — normalized attention
            guidance: a negative prompt that acts inside every cross-attention of every forward of the conditional context
            (WanModel.forward(nag=)), so it also acts on the steps that run the conditional branch alone — a 'cond' step, each window of
            one, the conditional half of a 'guided' step (under cfg_parallel: the half of the ranks that runs `input_prompt`).  The
            negative prompt is nag.n_prompt (text or a pre-computed embedding, as n_prompt), or the call's n_prompt when that is None.
            The unconditional half, the guidance mix, scheduler, masked_renoise, windows blend and decode are unchanged; a 'zero' step runs
            nothing.  `self.last_nag` holds the NAG of the last call (None without).  A negative prompt at ONE forward per step:
                generate(..., guidance=Guidance(interval=(0.0, 0.0)), nag=NAG(scale, n_prompt=...))
            (no sigma of a schedule is 0, so every step is 'cond').  A `model=` object whose forward does not take the `nag` keyword:
            ValueError before any forward."""
        return self._sample(input_prompt=input_prompt, size=size, frame_num=frame_num, shift=shift, sample_solver=sample_solver,
                            sampling_steps=sampling_steps, guide_scale=guide_scale, n_prompt=n_prompt, seed=seed, offload_model=offload_model,
                            noise=noise, callback=callback, step_cache=step_cache, guidance=guidance, windows=windows,
                            init_video=init_video, strength=strength, nag=nag)

    # `generate`'s arguments behind input_prompt with their defaults: what `inpaint` takes as keywords
    _GENERATE_DEFAULTS = dict(zip(generate.__code__.co_varnames[2:generate.__code__.co_argcount], generate.__defaults__))

    def masked_edit(self, init_video, mask, keep_frames, size, frame_num):
        """`inpaint`'s mask / keep_frames -> MaskedEdit(pm, lm): the mask through the cover / crop geometry of the frames (ops.mask_from_u8), the
        first keep_frames frames kept whole, then the OR over every pixel under a latent cell (ops.mask_to_latent)."""
        W_, H_ = size
        keep_frames = int(keep_frames)
        if not 0 <= keep_frames <= frame_num:
            raise ValueError(f'keep_frames must be in [0, {frame_num}], got {keep_frames}')
        if mask is None:
            if keep_frames == 0:
                raise ValueError('inpaint needs a mask or keep_frames > 0: there is nothing to keep')
            mask = torch.full((1, H_, W_), 255, dtype=torch.uint8, device=self.device)       # everything behind the kept frames is regenerated
        else:
            mask = torch.as_tensor(mask)
            if mask.dtype == torch.bool:
                mask = mask.to(torch.uint8) * 255
            if mask.dim() == 2:
                mask = mask.unsqueeze(0)
            if mask.dtype != torch.uint8 or mask.dim() != 3 or not (mask.shape[0] == 1 or mask.shape[0] >= frame_num):
                raise ValueError(f'mask must be uint8 or bool, [Tm, H0, W0] with Tm == 1 or Tm >= {frame_num}, or [H0, W0]; got {mask.dtype} {tuple(mask.shape)}')
            # the spatial size of init_video: the mask goes through the same resize and crop as the frames, so the two stay aligned
            src = init_video if torch.is_tensor(init_video) else torch.as_tensor(init_video)
            hw0 = tuple(src.shape[1:3]) if src.dim() == 4 and src.dtype == torch.uint8 else (H_, W_)
            if tuple(mask.shape[1:]) != hw0:
                raise ValueError(f'mask is {tuple(mask.shape[1:])}, init_video is {hw0}: the mask must have the spatial size of init_video')
            mask = mask[:frame_num].to(self.device).contiguous()
        pm = ops.mask_from_u8(mask, frame_num, H_, W_, keep_frames)
        return MaskedEdit(pm, ops.mask_to_latent(pm, self.vae_stride))

    def inpaint(self, input_prompt, init_video, mask=None, keep_frames=0, strength=1.0, **kw):
        """Masked video-to-video (NOT part of the reference): keep part of `init_video` and regenerate the rest.  `kw` are `generate`'s other
        arguments (size, frame_num, shift, sample_solver, sampling_steps, guide_scale, n_prompt, seed, offload_model, noise, callback, step_cache,
        guidance, windows, nag).

        mask: uint8 or bool, tensor or array, [Tm, H0, W0] (Tm == 1: one mask for every frame, or Tm >= frame_num: the first frame_num are used)
            or [H0, W0], with the spatial size of init_video (the frame size of uint8 frames, `size` for a float clip); >= 128 / True =
            regenerate, below = keep.  Hard masks only: the resized mask is thresholded at 127.5 again.
        keep_frames = k: the first k pixel frames are kept whole (continuation); with mask=None everything behind them is regenerated.
        strength: as in `generate`; the regenerated region starts from (1 - sigma) z0 + sigma noise like every video-to-video start.

        The latent blend with the start noise re-used: a latent cell is kept only if every pixel under it is kept (lm); after every scheduler
        step, which leaves the latent at sigma_{i+1}, the kept cells are overwritten with (1 - sigma_{i+1}) z0 + sigma_{i+1} noise
        (ops.masked_renoise, before `callback`), so the solver's history holds what the model saw and, sigma ending in 0, the kept cells end
        as z0.  After the decode the kept PIXELS are copied from the source clip (ops.mask_composite): a kept pixel of the result is the
        source pixel bit for bit.  Every rank does the same element-wise passes on its whole latent: no collective is added.  An all-regenerate
        mask gives the bits of `generate(init_video=, strength=)`."""
        if init_video is None:
            raise ValueError('inpaint needs init_video: there is nothing to keep')
        for name in kw:
            if name not in self._GENERATE_DEFAULTS:
                raise TypeError(f"inpaint() got an unexpected keyword argument '{name}'")
        args = dict(self._GENERATE_DEFAULTS, **kw, input_prompt=input_prompt, init_video=init_video, strength=strength)
        return self._sample(edit=self.masked_edit(init_video, mask, keep_frames, args['size'], args['frame_num']), **args)

    def _sample(self, *, input_prompt, size, frame_num, shift, sample_solver, sampling_steps, guide_scale, n_prompt, seed, offload_model,
                noise, callback, step_cache, guidance, windows, init_video, strength, nag=None, edit=None):
        """the body of `generate` and `inpaint`, which hand it `generate`'s arguments by name; edit: None, or inpaint's MaskedEdit.
        Three parts: the arguments resolved and checked (no GPU), the tensors and the call's SamplePlan, the loop over plan.steps."""
        step_cache = self.step_cache if step_cache is None else step_cache
        guidance = _checked_guidance(self.guidance if guidance is None else guidance)
        windows = _checked_windows(self.windows if windows is None else windows)
        nag = _checked_nag(self.nag if nag is None else nag, self.model)
        n_run, i0 = v2v_steps(sampling_steps, strength)
        if init_video is None and i0:
            raise ValueError('strength < 1 needs init_video: there is nothing to start from')
        target_shape = (self.vae.model.z_dim, (frame_num - 1) // self.vae_stride[0] + 1, size[1] // self.vae_stride[1],
                        size[0] // self.vae_stride[2])
        seq_len = dit_seq_len(*target_shape[1:], self.patch_size, self.sp_size)
        wplan = None                # the context windows of this call: a function of the latent's length alone; None = one pass, the loop as it was
        if windows is not None:
            if windows.stride != self.vae_stride[0]:
                raise ValueError(f'windows: {windows!r} counts frames for a temporal VAE stride of {windows.stride}, this pipeline has {self.vae_stride[0]}')
            wplan = windows.plan(target_shape[1])
        window_starts = None if wplan is None else wplan.starts
        refuse_windows_with_step_cache(window_starts, step_cache)       # (ahead of the prompt encoder; sample_plan checks the resolved plan again)
        if isinstance(n_prompt, str) and n_prompt == "":
            n_prompt = self.sample_neg_prompt
        seed = seed if seed >= 0 else random.randint(0, sys.maxsize)
        seed_g = torch.Generator(device=self.device)
        seed_g.manual_seed(seed)
        context = self._encode(input_prompt)
        context_null = self._encode(n_prompt)
        # NAG's negative prompt: its own, or the call's (already encoded); what every conditional forward of the loop is handed
        nag_arg = None if nag is None else (nag, context_null if nag.n_prompt is None else self._encode(nag.n_prompt))
        self.last_nag = nag
        if noise is None:
            noise = torch.randn(*target_shape, dtype=torch.float32, device=self.device, generator=seed_g)
        else:
            noise = noise.to(self.device, torch.float32).contiguous()       # (the latent kernels work on dense memory; a permuted view is copied here)
            assert tuple(noise.shape) == tuple(target_shape)

        with torch.no_grad():
            sample_scheduler, timesteps = self._scheduler(sample_solver, sampling_steps, shift)

            latent = noise
            if init_video is not None:
                sample_scheduler.set_begin_index(i0)
                keep = {} if edit is None else {'keep': edit}        # (`generate` calls the five-argument form: a replaced start_latent keeps serving it)
                latent = self.start_latent(init_video, size, frame_num, noise, sample_scheduler.sigmas[i0].item() if i0 else 1.0, **keep)
            timesteps_host = timesteps.tolist()          # ONE sync for the whole loop
            sigmas_host = sample_scheduler.sigmas.tolist() if edit is not None or guidance is not None else None   # (steps + 1 entries, the last one 0)
            if next(self.model.parameters()).device != self.device:     # only after a real offload (a no-op move would
                self.model.to(self.device)                               # still drop the fused-weight views: 28 GB re-packed)
            noise_pred = torch.empty_like(latent)
            step_plan, stats = resolve_plan(step_cache, self.model, timesteps, i0)
            kinds = None if guidance is None else guidance.plan(sigmas_host[:len(timesteps_host)], i0)
            # every decision that depends on the schedule alone, made here once: wan/utils/sample_plan.py
            plan = sample_plan(len(timesteps_host), i0, kinds, step_plan, stats, own_branch_only=self.cfgp is not None, window_starts=window_starts)
            self.last_guidance_plan, self.last_step_plan, self.last_window_plan = plan.kinds, plan.step_plan, plan.window_starts
            self.last_step_timesteps = timesteps if plan.step_plan is not None else None     # what the plan was made of (tools/step_cache_calibrate.py)
            # scratch and buffers of the guided mix and of the windowed steps, once per call
            mix = GuidedMix(guidance, guide_scale, plan.any_guided, self.device)
            wrun = None if wplan is None else WindowRun(wplan, latent, plan.any_guided, self.patch_size, self.sp_size)
            for i, kind, cache in plan.steps:
                t = timesteps[i:i + 1]
                if kind == 'zero':          # CFG-Zero*'s zero-init: no forward, the scheduler steps on a zero prediction
                    pred = noise_pred.zero_()
                else:                       # a 'cond' step's prediction is used as it is (a new tensor of every forward)
                    with self.model.step_cache(cache, stats=plan.stats) if cache else contextlib.nullcontext():     # (a 'skip' scope reads no stats)
                        cond, uncond = self._predictions(kind, latent, t, context, context_null, seq_len, wrun, **({} if nag_arg is None else {'nag': nag_arg}))
                    pred = cond if kind == 'cond' else mix(noise_pred, uncond, cond)
                latent = sample_scheduler.step(pred.unsqueeze(0), timesteps_host[i], latent.unsqueeze(0),
                                               return_dict=False, generator=seed_g)[0].squeeze(0)
                if edit is not None:        # the step left the latent at sigma_{i+1}: put the kept cells back at that noise level
                    ops.masked_renoise(latent, edit.z0, noise, edit.lm, 1.0 - sigmas_host[i + 1], sigmas_host[i + 1])
                if callback is not None:
                    callback(i, latent)
            if plan.step_plan is not None:
                self.model.drop_step_cache()
            videos = self._decode([latent], target_shape, offload_model)
            if edit is not None and videos is not None:     # on the rank that holds the video: kept pixels are the source's, bit for bit
                ops.mask_composite(videos[0], edit.clip, edit.pm)

        del noise, latent, sample_scheduler
        if offload_model:
            gc.collect()
            torch.cuda.synchronize()
        if dist.is_initialized():
            dist.barrier()
        return videos[0] if self.rank == 0 else None
