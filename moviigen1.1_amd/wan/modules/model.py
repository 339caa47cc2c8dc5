"""WanModel — the MoviiGen1.1 / Wan2.1 DiT, executed by hand-written HIP kernels on MI355X.

Drop-in for the reference class of the same name (reference wan/modules/model.py:361-633):
same constructor arguments, same state_dict key names and shapes (so `from_pretrained` reads the
reference checkpoint layout: config.json + diffusion_pytorch_model*.safetensors), same
`forward(x, t, context, seq_len, clip_fea=None, y=None) -> List[Tensor[C,F,H,W] fp32]`.

What differs is HOW a forward runs.  The reference composes ~40 torch ops per block under
autocast; here a block is 15 kernel launches from libmoviigen_hip.so at head_dim 128, 14 at any other:

    self-attention    ln_modulate -> gemm(q|k|v fused, N=3*dim) -> rmsnorm_rope(q, x softmax_scale*log2e) -> rmsnorm_rope(k)
                      -> pack_kv (head_dim 128 only: K/V as 64-key tiles) -> attention -> gemm(o) with `x += y*gate` fused
    cross-attention   ln_modulate(norm3 affine) -> gemm(q) -> rmsnorm -> attention(512 cached text keys)
                      -> gemm(o) with `x += y` fused
    ffn               ln_modulate -> gemm(ffn.0)+GELU fused -> gemm(ffn.2) with `x += y*gate` fused

(tests/test_gpu_parity.py::test_dit_forward_launch_sequence pins the whole forward's sequence.)

The rounding points of the reference's autocast(bf16) execution are reproduced (SURVEY.md
Appendix B): bf16 GEMM operands/results, fp32 accumulate, fp32 residual stream, fp32 norms and
modulation, fp32 time embedding and head.  GEMM weights are stored in bf16 (what autocast feeds
the GEMM anyway); norm weights, modulation tables, time embedding and head stay fp32.
Per-prompt work that does not depend on the timestep (text_embedding, the 40 cross-attention
K/V projections) is computed once per prompt and cached — identical values, 100x fewer times.

There is no torch fallback: without the HIP library (or a GPU) forward() raises.
"""
import collections
import contextlib
import json
import math
import os

import numpy as np
import torch
import torch.nn as nn

from ..backend import ops
from ..distributed.layout import SpLayout
from .attention import attend, pack_tiles, q_prescale
from .attention import flash_attention      # operator seam (1): the reference binds it here by name (model.py:10)

__all__ = ['WanModel']

_ENGINE_FLASH_ATTENTION = flash_attention


def _rebound_flash_attention():
    """the function a caller bound as `wan.modules.model.flash_attention` (the reference calls that module-level
    name at model.py:146-151 and :176, so assigning it replaces the attention of every block), or None while the name
    still is the engine's own operator — then the fused kernels on packed operands run instead of the wrapper."""
    fn = globals()['flash_attention']
    return None if fn is _ENGINE_FLASH_ATTENTION else fn

_BF16_SUFFIXES = ('.q.weight', '.k.weight', '.v.weight', '.o.weight', 'ffn.0.weight', 'ffn.2.weight',
                  'text_embedding.0.weight', 'text_embedding.2.weight', 'patch_embedding.weight')


class _Lin(nn.Module):
    """parameter holder with nn.Linear's names (weight [out,in], bias [out]); no forward."""

    def __init__(self, out_f, in_f, wdtype, device):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_f, in_f, dtype=wdtype, device=device), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_f, dtype=torch.float32, device=device), requires_grad=False)


class _Vec(nn.Module):
    def __init__(self, dim, device, bias=False):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim, dtype=torch.float32, device=device), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(dim, dtype=torch.float32, device=device), requires_grad=False)


class _Attn(nn.Module):
    """parameters of WanSelfAttention / WanT2VCrossAttention (reference model.py:102-181).  Inside WanModel.forward
    attention runs fused in the engine's layer loop; `forward` below is the same operator stand-alone, with the
    reference's call shape — the operator seam of text2video.py:97-100 (`types.MethodType(fn, block.self_attn)`)."""
    sp = None       # a self-attention module's tag: the model's SpLayout where its Ulysses exchange is on (WanModel.set_sp_layout)

    def __init__(self, dim, device, num_heads=None, eps=1e-6):
        super().__init__()
        for n in 'qkvo':
            setattr(self, n, _Lin(dim, dim, torch.bfloat16, device))
        self.norm_q = _Vec(dim, device)
        self.norm_k = _Vec(dim, device)
        self.dim, self.num_heads, self.eps = dim, num_heads, eps
        self._xchg = {}     # (group, Lloc, device) -> HeadExchange of the stand-alone sequence-parallel operator

    def forward(self, x, seq_lens, grid_sizes, freqs=None, sp=None):
        """WanSelfAttention.forward (model.py:127-156): x [B, L, C] -> [B, L, C] bf16.  `freqs` (the reference's
        complex table) is accepted and ignored: the rotation angles are rebuilt from grid_sizes (same formula).
        sp = an SpLayout (wan/distributed/layout.py): x is the rank's token shard, Ulysses exchange around the attention
        (usp_attn_forward, xdit_context_parallel.py:155-198)."""
        if sp is not None and sp.R > 1:
            raise NotImplementedError('the stand-alone self-attention operator does not rotate K/V blocks: under the ring / '
                                      'hybrid layouts call WanModel.forward (wan/distributed/ring.py)')
        d, N = self.dim, self.num_heads
        hd = d // N
        bf = torch.bfloat16
        P, pos_rank = (sp.U, sp.rank) if sp is not None else (1, 0)
        outs = []
        for b in range(x.shape[0]):
            h = x[b].to(bf).contiguous()
            L, dev = h.shape[0], h.device
            grid = tuple(int(v) for v in grid_sizes[b].tolist())
            q, k, v, qn, kn, a, o = (torch.empty(L, d, dtype=bf, device=dev) for _ in range(7))
            for lin, dst in ((self.q, q), (self.k, k), (self.v, v)):
                ops.gemm(h, lin.weight, lin.bias, ops.BIAS_BF16, dst)
            # from here on the pieces of the fused layer loop (WanModel._self_attention): the same launches, the same bits
            self.norm_rope_qk(q, k, qn, kn, rope_cos_sin(hd, grid).to(dev), grid, pos_rank * L)
            if P > 1:
                self._exchange(sp.uly_group, P, L, dev).run(qn, kn, v, a, lambda qg, kg, vg, ag, n: attend(qg, kg, vg, ag, kg.shape[0], n, hd))
            else:
                attend(qn, kn, v, a, min(L, int(seq_lens[b])) if seq_lens is not None else L, N, hd)
            ops.gemm(a, self.o.weight, self.o.bias, ops.BIAS_BF16, o)
            outs.append(o)
        return torch.stack(outs)

    def norm_rope_qk(self, q, k, qn, kn, rope=None, grid=(1, 1, 1), pos0=0, prescale=True):
        """RMS-norm + RoPE of the projected q and k [L, dim] bf16 (column views ok) -> qn, kn.  prescale: q_prescale() is folded into
        qn before its one rounding to bf16, as attend() expects it; False for a caller-bound flash_attention, which scales itself.
        k=None: q only (cross-attention: its k is normed once per prompt, WanModel._cross_kv)."""
        hd = self.dim // self.num_heads
        ops.rmsnorm_rope(q, self.norm_q.weight, self.eps, hd, qn, rope, grid, pos0, out_scale=q_prescale(hd) if prescale else 1.0)
        if k is not None:
            ops.rmsnorm_rope(k, self.norm_k.weight, self.eps, hd, kn, rope, grid, pos0)

    def _exchange(self, group, P, L, dev):
        """the HeadExchange of the stand-alone sequence-parallel operator: one live shape, its buffers and stream are persistent"""
        from ..distributed.ulysses import HeadExchange
        key = (group, L, str(dev))
        if key not in self._xchg:
            self._xchg = {key: HeadExchange(group, P, self.num_heads, self.dim // self.num_heads, L, dev)}
        return self._xchg[key]


class _Block(nn.Module):
    def __init__(self, dim, ffn_dim, device, num_heads=None, eps=1e-6):
        super().__init__()
        self.self_attn = _Attn(dim, device, num_heads, eps)
        self.norm3 = _Vec(dim, device, bias=True)
        self.cross_attn = _Attn(dim, device, num_heads, eps)
        self.ffn = nn.ModuleDict({'0': _Lin(ffn_dim, dim, torch.bfloat16, device),
                                  '2': _Lin(dim, ffn_dim, torch.bfloat16, device)})
        self.modulation = nn.Parameter(torch.empty(1, 6, dim, dtype=torch.float32, device=device),
                                       requires_grad=False)


class _Head(nn.Module):
    def __init__(self, dim, out_f, device):
        super().__init__()
        self.head = _Lin(out_f, dim, torch.float32, device)
        self.modulation = nn.Parameter(torch.empty(1, 2, dim, dtype=torch.float32, device=device),
                                       requires_grad=False)


class _PatchEmbed(nn.Module):
    def __init__(self, dim, in_dim, patch, device):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(dim, in_dim, *patch, dtype=torch.bfloat16, device=device),
                                   requires_grad=False)
        self.bias = nn.Parameter(torch.empty(dim, dtype=torch.float32, device=device), requires_grad=False)


def _replaced_forward(attn):
    """the instance-level `forward` a caller installed on a self-attention module (types.MethodType), unless it is
    one of this engine's own entry points (usp_attn_forward only re-states what the fused loop does anyway)."""
    fn = attn.__dict__.get('forward')
    if fn is None:
        return None
    from ..distributed.xdit_context_parallel import usp_attn_forward
    if getattr(fn, '__func__', fn) in (usp_attn_forward, _Attn.forward):
        return None
    return fn


def rope_cos_sin(head_dim, grid, theta=10000.0):
    """(cos, sin) tables of reference model.py:28-36,473-478 for positions < (F, H, W), fp64 ->
    fp32, laid out [F][c0] ++ [H][c1] ++ [W][c1] as mg_rmsnorm_rope_bf16 expects."""
    c = head_dim // 2
    c1 = c // 3
    c0 = c - 2 * c1
    parts = []
    for n, cnt in zip(grid, (c0, c1, c1)):
        inv = 1.0 / np.power(theta, np.arange(0, 2 * cnt, 2, dtype=np.float64) / (2 * cnt))
        ang = np.outer(np.arange(n, dtype=np.float64), inv)
        parts.append(np.stack([np.cos(ang), np.sin(ang)], axis=-1).reshape(-1, 2))
    return torch.from_numpy(np.concatenate(parts).astype(np.float32))


# set_gemm_precision('mxfp8'): which of the six per-block linears run on mg_gemm_mxfp8.  A site is True only if activation
# quantisation + the MXFP8 GEMM is faster than mg_gemm_bf16 at its step shape (M = 131 040) in
# profiles/pr_gemm_mxfp8_shapes_131040.log (tools/bench_gemm_mxfp8.py; the three fp8 sites win by 2-3 % only); a site that loses there stays bf16 in 'mxfp8' mode too.
#   site            N      K      epilogue     bf16 ms   quantise + mxfp8 ms
#   wqkv            15360   5120  bias         13.79     13.49   fp8
#   self_attn.o      5120   5120  gate-resid    4.97      5.30   bf16  (cross_attn.q — the same shape, bias epilogue — and cross_attn.o too:
#                                                                       the GEMM alone gains 0.08 ms, the quantiser costs 0.39)
#   ffn.0           13824   5120  GELU         12.68     12.29   fp8
#   ffn.2            5120  13824  gate-resid   12.47     12.21   fp8
MXFP8_SITES = {'wqkv': True, 'self_attn.o': False, 'cross_attn.q': False, 'cross_attn.o': False, 'ffn.0': True, 'ffn.2': True}
# 'mxfp8' mode: the producers that write an fp8 site's operand themselves (no bf16 round trip, no mg_quant_mxfp8_rows pass).  A producer
# is True only if it is not slower than its unfused pair in every round of profiles/pr_mxfp8_fused_producers.log:
#   'ln_modulate'  mg_ln_modulate_mxfp8 in front of wqkv, cross_attn.q and ffn.0 (where that site is fp8 and nothing else reads h)
#   'gelu'         mg_gemm_mxfp8_gelu_q as ffn.0 when ffn.0 and ffn.2 are both fp8
# self_attn.o and cross_attn.o take an attention output: they keep the stand-alone quantiser (or stay bf16, as MXFP8_SITES says).
# That log has not been taken yet (tools/bench_gemm_mxfp8.py 131040 10 10 fused prints the two values): both producers are built and
# tested (tests/test_mxfp8_fused.py wires them in itself) but stay unwired until it has.
MXFP8_FUSED_PRODUCERS = {'ln_modulate': False, 'gelu': False}
GEMM_PRECISIONS = ('bf16', 'mxfp8')

# one forward's shape and placement (WanModel._plan): fhw = the latent's (F, H, W); grid = its token grid; Lfull = the video's tokens,
# which is also the valid key count of the self-attention (keys past it are padding); L, pos0 = this rank's rows of the (padded) sequence
# and the position of its first one; n_valid = the video tokens among them (all of them unless padded); ws = the workspace of this
# shape; rope = the (cos, sin) table of the grid; fa = _rebound_flash_attention() as this forward found it
_Plan = collections.namedtuple('_Plan', 'fhw grid Lfull L pos0 n_valid ws rope fa')
# block i's cross-attention K (RMS-normed) and V of one prompt.  layout 'fused': the operands of attend(packed=True) — 64-key tiles at
# head_dim 128, row-major [text_len, dim] otherwise; 'seam': row-major whatever the head_dim, for a rebound flash_attention
_CrossKV = collections.namedtuple('_CrossKV', 'k v layout')


class _Linears:
    """The six linears of ONE block and the LayerNorms in front of them, bound to what does not differ between their call sites: the
    block's GEMM operands `lw`, its quantised weights `mx` ({site: (bytes, scales)} of the sites on fp8; None = bf16 mode), the
    workspace and eps.  `feed` is the one place that decides which kernel quantises an fp8 site's operand."""
    __slots__ = ('lw', 'mx', 'ws', 'eps', 'fuse')

    def __init__(self, lw, mx, ws, eps, fuse):
        self.lw, self.mx, self.ws, self.eps, self.fuse = lw, mx, ws, eps, fuse

    def feed(self, site):
        """how `site` gets its A operand: None = bf16, the site runs on mg_gemm_bf16 (also: site None, a reader outside the six);
        'ln' / 'gelu' = the LayerNorm / ffn.0's GELU epilogue in front of it writes fp8 itself (the bf16 activation is NOT written);
        'quant' = mg_quant_mxfp8_rows of the bf16 activation."""
        if self.mx is None or site not in self.mx:
            return None
        if self.fuse and site in ('wqkv', 'cross_attn.q', 'ffn.0') and MXFP8_FUSED_PRODUCERS['ln_modulate']:
            return 'ln'                         # (the three sites that are the only reader of a LayerNorm's output)
        if self.fuse and site == 'ffn.2' and 'ffn.0' in self.mx and MXFP8_FUSED_PRODUCERS['gelu']:
            return 'gelu'
        return 'quant'

    def _act(self, site):
        """the quantised-activation buffers of `site`'s operand: h / a share one [L, dim] pair, u has its own"""
        return (self.ws['uq'], self.ws['us']) if site == 'ffn.2' else (self.ws['hq'], self.ws['hs'])

    def ln(self, site, x, scale, shift, add_one, round_norm_bf16=False):
        """LayerNorm + modulate of the stream x in front of `site`: bf16 into ws['h'], or straight into the site's fp8 operand"""
        if self.mx and self.feed(site) == 'ln':
            ops.ln_modulate_mxfp8(x, scale, shift, add_one, self.eps, *self._act(site), round_norm_bf16=round_norm_bf16)
        else:
            ops.ln_modulate(x, scale, shift, add_one, self.eps, self.ws['h'], round_norm_bf16=round_norm_bf16)

    def __call__(self, site, a, bias, epilogue, out, gate=None):
        """out (+)= a @ W[site]^T with `epilogue` (ops.gemm).  On an fp8 site `a` is read only where feed() says 'quant'; ffn.0 in front
        of a 'gelu'-fed ffn.2 writes that site's fp8 operand and not `out`."""
        feed = self.feed(site) if self.mx else None             # (bf16 mode: not even the call, six times a block)
        if feed is None:
            return ops.gemm(a, self.lw[site], bias, epilogue, out, gate=gate)
        aq, a_s = self._act(site)
        if feed == 'quant':
            ops.quant_mxfp8(a, aq, a_s)
        wq, w_s = self.mx[site]
        if site == 'ffn.0' and self.feed('ffn.2') == 'gelu':
            return ops.gemm_mxfp8_gelu_q(aq, a_s, wq, w_s, bias, *self._act('ffn.2'))
        return ops.gemm_mxfp8(aq, a_s, wq, w_s, bias, epilogue, out, gate=gate)


class WanModel(nn.Module):
    ignore_for_config = ['patch_size', 'cross_attn_norm', 'qk_norm', 'text_dim', 'window_size']
    _no_split_modules = ['WanAttentionBlock']

    def __init__(self, model_type='t2v', patch_size=(1, 2, 2), text_len=512, in_dim=16, dim=2048, ffn_dim=8192,
                 freq_dim=256, text_dim=4096, out_dim=16, num_heads=16, num_layers=32, window_size=(-1, -1),
                 qk_norm=True, cross_attn_norm=True, eps=1e-6, device=None):
        super().__init__()
        if model_type != 't2v':
            raise NotImplementedError('only the t2v path of MoviiGen1.1 is implemented (reference configs '
                                      'register t2v-14B / t2i-14B only)')
        if tuple(window_size) != (-1, -1) or not qk_norm or not cross_attn_norm:
            raise NotImplementedError('window attention / qk_norm=False / cross_attn_norm=False are never used '
                                      'by the reference configs')
        assert dim % num_heads == 0 and (dim // num_heads) % 2 == 0
        self.model_type, self.patch_size, self.text_len = model_type, tuple(patch_size), text_len
        self.in_dim, self.dim, self.ffn_dim, self.freq_dim, self.text_dim = in_dim, dim, ffn_dim, freq_dim, text_dim
        self.out_dim, self.num_heads, self.num_layers, self.eps = out_dim, num_heads, num_layers, eps
        self.window_size, self.qk_norm, self.cross_attn_norm = window_size, qk_norm, cross_attn_norm
        self.config = dict(model_type=model_type, text_len=text_len, in_dim=in_dim, dim=dim, ffn_dim=ffn_dim,
                           freq_dim=freq_dim, out_dim=out_dim, num_heads=num_heads, num_layers=num_layers, eps=eps)
        dv = device
        self.patch_embedding = _PatchEmbed(dim, in_dim, self.patch_size, dv)
        self.text_embedding = nn.ModuleDict({'0': _Lin(dim, text_dim, torch.bfloat16, dv),
                                             '2': _Lin(dim, dim, torch.bfloat16, dv)})
        self.time_embedding = nn.ModuleDict({'0': _Lin(dim, freq_dim, torch.float32, dv),
                                             '2': _Lin(dim, dim, torch.float32, dv)})
        self.time_projection = nn.ModuleDict({'1': _Lin(6 * dim, dim, torch.float32, dv)})
        self.blocks = nn.ModuleList([_Block(dim, ffn_dim, dv, num_heads, eps) for _ in range(num_layers)])
        self.head = _Head(dim, math.prod(self.patch_size) * out_dim, dv)
        # sequence-parallel placement: one value, written by set_sp_layout alone (sp_size / sp_rank / sp_group read it).  The attention
        # modules' tags are not written here: a never-configured module is what usp_attn_forward's default recognises
        self.sp_layout = SpLayout.single()
        self.sp_force = False   # run the Ulysses collectives even on a 1-rank group (RCCL smoke test)
        # training-side SP forward (scripts/train/model/model_seq.py): the sequence is zero-padded to seq_len before it
        # is chunked over the ranks and padded keys are masked (k_lens); cross-attention is head-sharded
        self.sp_mask_padded_keys = False
        self.cross_attn_head_sharded = False
        self._packed = None
        self._shards = None             # wan.distributed.fsdp.BlockShards installs itself here: the GEMM weights are block-sharded
        self._freqs = None              # the reference's complex RoPE table, built by the `freqs` property
        self.gemm_precision = 'bf16'   # set_gemm_precision: 'mxfp8' = the six per-block linears on the block-scaled MFMA (opt-in)
        self._mx = None                 # their quantised weights, built once per set of weights
        self._mx_fuse = True            # False: every fp8 site quantises its bf16 activation with mg_quant_mxfp8_rows (tests, tools/bench_gemm_mxfp8.py)
        self._ws = {}
        self._rope = {}
        self._ctx_cache = {}
        self._lora = []                 # load_lora: (name, strength) of the adapters merged into the weights
        self._lora_base = None          # ... and the touched weights as they were (keep_base=True), for unload_lora
        self._step_mode = None          # step_cache(): ('compute' | 'skip', stats) while the scope is open
        self.step_cache_stats = {}      # stats=True: context key -> (sum |r_new - r_old|, sum |r_old|) of its last computed step

    sp_size = property(lambda self: self.sp_layout.size)
    sp_rank = property(lambda self: self.sp_layout.rank)
    sp_group = property(lambda self: self.sp_layout.group)

    def set_sp_layout(self, layout):
        """the one writer of the sequence-parallel placement (an SpLayout, wan/distributed/layout.py): checks it against the heads, drops the
        old layout's workspace and tags every self-attention module for its stand-alone operator (usp_attn_forward)"""
        if self.num_heads % layout.U:       # reference generate.py:238-239
            raise ValueError(f'`num_heads` {self.num_heads} cannot be divided evenly by the '
                             f'{"sequence-parallel" if layout.R == 1 else "ulysses"} size {layout.U}')
        if layout.R > 1 and self.dim // self.num_heads != 128:
            raise NotImplementedError('ring attention is built on the head_dim 128 kernels')
        self.sp_layout, self._ws = layout, {}
        for blk in self.blocks:     # one rank: no exchange.  A ring / hybrid tag makes the operator refuse: only the fused forward rotates K/V blocks
            blk.self_attn.sp = layout if layout.size > 1 else None
        return self

    @property
    def freqs(self):
        """the reference's complex RoPE table [1024, head_dim/2] (model.py:473-478), built on demand for callers of
        the operator seam; the engine's kernels use rope_cos_sin() instead."""
        if self._freqs is None:
            d = self.dim // self.num_heads

            def params(dim):
                ang = torch.outer(torch.arange(1024, dtype=torch.float64),
                                  1.0 / torch.pow(10000.0, torch.arange(0, dim, 2, dtype=torch.float64) / dim))
                return torch.polar(torch.ones_like(ang), ang)
            self._freqs = torch.cat([params(d - 4 * (d // 6)), params(2 * (d // 6)), params(2 * (d // 6))], dim=1)
        return self._freqs

    # ------------------------------------------------------------------------------------------
    # checkpoint layout (reference text2video.py:87)
    # ------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, checkpoint_dir, device=None):
        from safetensors import safe_open
        with open(os.path.join(checkpoint_dir, 'config.json')) as f:
            cfg = json.load(f)
        keys = ('model_type', 'text_len', 'in_dim', 'dim', 'ffn_dim', 'freq_dim', 'text_dim', 'out_dim', 'num_heads',
                'num_layers', 'eps')
        kw = {k: cfg[k] for k in keys if k in cfg}
        if 'patch_size' in cfg:
            kw['patch_size'] = tuple(cfg['patch_size'])
        model = cls(**kw, device=device)
        idx = os.path.join(checkpoint_dir, 'diffusion_pytorch_model.safetensors.index.json')
        if os.path.exists(idx):
            with open(idx) as f:
                files = sorted(set(json.load(f)['weight_map'].values()))
        else:
            files = sorted(f for f in os.listdir(checkpoint_dir)
                           if f.startswith('diffusion_pytorch_model') and f.endswith('.safetensors'))
        if not files:
            raise FileNotFoundError(f'no diffusion_pytorch_model*.safetensors under {checkpoint_dir}')
        own = dict(model.named_parameters())
        seen = set()
        for fn in files:
            with safe_open(os.path.join(checkpoint_dir, fn), framework='pt', device='cpu') as sf:
                for k in sf.keys():
                    if k not in own:
                        raise KeyError(f'unexpected checkpoint tensor {k}')
                    own[k].data.copy_(sf.get_tensor(k).reshape(own[k].shape))
                    seen.add(k)
        missing = set(own) - seen
        if missing:
            raise KeyError(f'checkpoint is missing {sorted(missing)[:5]} ...')
        return model

    def load_state_dict(self, state_dict, strict=True, assign=False):
        out = super().load_state_dict(state_dict, strict=strict, assign=False)
        self._invalidate()
        return out

    def init_weights(self, seed=0, std=0.02):
        """seeded synthetic weights: N(0, std) GEMM weights, N(0,1)/sqrt(dim)
        modulation, unit norm weights; generated directly on the parameter's device."""
        g = torch.Generator(device=self.patch_embedding.weight.device)
        g.manual_seed(seed)
        for name, p in self.named_parameters():
            if name.endswith('modulation'):
                p.data.copy_(torch.randn(p.shape, generator=g, device=p.device) / math.sqrt(self.dim))
            elif 'norm' in name and name.endswith('weight'):
                p.data.fill_(1.0)
            elif name.endswith('bias'):
                p.data.copy_(torch.randn(p.shape, generator=g, device=p.device) * std)
            else:
                p.data.copy_((torch.randn(p.shape, generator=g, device=p.device, dtype=torch.float32) * std))
        self._invalidate()
        return self

    def _invalidate(self):
        self._packed = None
        self._mx = None
        self._ctx_cache = {}
        self.drop_step_cache()          # residuals of other weights are not residuals of these

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        # keep the storage dtypes fixed: `.to(torch.float32)`-style casts must not widen bf16 weights
        for name, p in self.named_parameters():
            want = torch.bfloat16 if name.endswith(_BF16_SUFFIXES) else torch.float32
            if p.dtype != want:
                p.data = p.data.to(want)
        if self._lora_base:             # the kept base weights follow the parameters (device moves; a cast and back is exact)
            self._lora_base = {k: fn(v) for k, v in self._lora_base.items()}
        self._invalidate()
        self._ws, self._rope = {}, {}
        return out

    # ------------------------------------------------------------------------------------------
    # LoRA adapters: merged into the weights on the device, once per model
    # ------------------------------------------------------------------------------------------
    @property
    def lora(self):
        """[(adapter file name or '<dict>', strength)] of the adapters currently merged into the weights; [] = the base weights"""
        return list(self._lora)

    def lora_targets(self):
        """{module name: weight} of every linear layer an adapter may name (`blocks.3.cross_attn.k`, `blocks.0.ffn.2`, `text_embedding.0`,
        `time_projection.1`, `head.head`, ...): bf16 storage, or fp32 for the time embedding / projection and the head.  patch_embedding
        is a convolution and is not among them."""
        return {n: m.weight for n, m in self.named_modules() if isinstance(m, _Lin)}

    @torch.no_grad()
    def load_lora(self, adapters, strength=1.0, keep_base=True, strict=True):
        """Merge LoRA adapters into the weights, in place, on the device: per target W <- round(W + sum_a s_a * up_a @ down_a), s_a =
        strength_a * alpha_a / rank_a (strength_a where the file has no alpha).  adapters: one `.safetensors` path or dict of tensors, or
        a list of them (wan/utils/lora.py: the spellings read); strength: one float, or one per adapter.  The scaled factors of ALL
        adapters are concatenated along the rank and merged by ONE mg_lora_merge per weight, in fp32 with a single rounding to the
        weight's storage type — N adapters cost one rounding, not N.  Nothing else changes: the next forward re-packs, re-quantises
        the 'mxfp8' weights and recomputes the cached cross-attention k|v, and from then on runs exactly what it would run on a
        checkpoint that held these weights.  keep_base: clone the touched weights first (unload_lora restores them bit for bit)."""
        from ..utils.lora import read_lora
        targets = self.lora_targets()
        dev = self.patch_embedding.weight.device
        if dev.type != 'cuda':
            raise RuntimeError('WanModel.load_lora needs the model on a HIP device (model.to("cuda")): the merge is a HIP kernel '
                               'and has no CPU implementation')
        if self._lora:
            raise RuntimeError(f'adapters {self._lora} are merged into the weights already: unload_lora() first')
        if self._shards is not None:
            raise NotImplementedError('load_lora needs resident weights: merge before the weights are block-sharded '
                                      '(wan.distributed.fsdp shard_model; WanT2V(lora=...) does it in that order)')
        if isinstance(adapters, (str, os.PathLike, dict)):
            adapters = [adapters]
        adapters = list(adapters)
        strengths = [float(strength)] * len(adapters) if isinstance(strength, (int, float)) else [float(s) for s in strength]
        if len(strengths) != len(adapters):
            raise ValueError(f'{len(adapters)} adapters but {len(strengths)} strengths')
        shapes = {n: tuple(w.shape) for n, w in targets.items()}
        factors = {}                    # target -> [(up, down, scale)]
        for src, s in zip(adapters, strengths):
            for name, (up, down, alpha) in read_lora(src, shapes, strict=strict).items():
                factors.setdefault(name, []).append((up, down, s if alpha is None else s * alpha / up.shape[1]))
        if keep_base:
            self._lora_base = {n: targets[n].data.clone() for n in factors}
        for name, fs in factors.items():
            ups = []
            for up, _, scale in fs:     # the scale is folded into `up` in fp32, by the engine's own kernel
                up = up.to(dev)
                ups.append(ops.lincomb(torch.empty_like(up), [(up, scale)]))
            downs = [down.to(dev) for _, down, _ in fs]
            ops.lora_merge(targets[name].data, ups[0] if len(ups) == 1 else torch.cat(ups, 1),
                           downs[0] if len(downs) == 1 else torch.cat(downs, 0))
        self._lora = [(src if isinstance(src, (str, os.PathLike)) else '<dict>', s) for src, s in zip(adapters, strengths)]
        self._invalidate()
        return self

    @torch.no_grad()
    def unload_lora(self):
        """copy the base weights back (load_lora(keep_base=True)): state_dict() is then bit-identical to before load_lora"""
        if not self._lora:
            raise RuntimeError('no adapters are loaded')
        if self._lora_base is None:
            raise RuntimeError('the adapters were loaded with keep_base=False: the base weights were not kept, reload the checkpoint')
        targets = self.lora_targets()
        for name, base in self._lora_base.items():
            targets[name].data.copy_(base)      # in place: q / k / v stay views of the fused storage
        self._lora, self._lora_base = [], None
        self._invalidate()
        return self

    # ------------------------------------------------------------------------------------------
    # engine-side packing: fused QKV / cross-KV weights, stacked modulation
    # ------------------------------------------------------------------------------------------
    def _pack(self):
        if self._packed is not None:
            return self._packed
        dev = self.patch_embedding.weight.device
        if dev.type != 'cuda':
            raise RuntimeError('WanModel.forward needs the model on a HIP device (model.to("cuda")): the hot '
                               'path has no CPU implementation — use oracle/ for CPU reference numbers')
        pk = {'layers': []}
        sharded = self._shards is not None
        for b in self.blocks:
            sa, ca = b.self_attn, b.cross_attn
            lw = dict(bqkv=torch.cat([sa.q.bias, sa.k.bias, sa.v.bias]).contiguous(),
                      bkv_c=torch.cat([ca.k.bias, ca.v.bias]).contiguous())
            if not sharded:
                wqkv = torch.cat([sa.q.weight, sa.k.weight, sa.v.weight], 0).contiguous()
                # re-point the three parameters at the fused storage: no second copy of the weights
                d = self.dim
                sa.q.weight.data, sa.k.weight.data, sa.v.weight.data = wqkv[:d], wqkv[d:2 * d], wqkv[2 * d:]
                wkv = torch.cat([ca.k.weight, ca.v.weight], 0).contiguous()
                ca.k.weight.data, ca.v.weight.data = wkv[:d], wkv[d:]
                lw.update({'wqkv': wqkv, 'wkv_c': wkv, 'self_attn.o': sa.o.weight, 'cross_attn.q': ca.q.weight,
                           'cross_attn.o': ca.o.weight, 'ffn.0': b.ffn['0'].weight, 'ffn.2': b.ffn['2'].weight})
            pk['layers'].append(lw)
        pk['modulation'] = torch.cat([b.modulation.data.reshape(6, self.dim) for b in self.blocks], 0).contiguous()
        pk['patch_w'] = self.patch_embedding.weight.data.reshape(self.dim, -1)
        self._packed = pk
        return pk

    def set_gemm_precision(self, precision):
        """Arithmetic of the six per-block linears of the layer loop (q|k|v, self_attn.o, cross_attn.q, cross_attn.o, ffn.0, ffn.2):
        'bf16' (default, the reference's) or 'mxfp8' — OCP MXFP8 operands (e4m3 elements, one power-of-two scale per 32 along K;
        include/moviigen_hip.h) on the block-scaled MFMA, fp32 accumulation, the same epilogues.  NOT the reference's arithmetic:
        an opt-in like WanVAE(mode='bf16x3'), never the default, with its own parity statement.  The weights are
        quantised once, at the next forward; the bf16 parameters stay (state_dict, and 'bf16' switches back bit for bit).  The
        embeddings, the once-per-prompt cross k|v and the head are not touched."""
        if precision not in GEMM_PRECISIONS:
            raise ValueError(f'gemm precision must be one of {GEMM_PRECISIONS}, got {precision!r}')
        if precision == 'mxfp8' and self._shards is not None:
            raise NotImplementedError("set_gemm_precision('mxfp8') needs resident weights: block-sharded weights (wan.distributed.fsdp) "
                                      'are gathered in bf16 per block and are not quantised')
        if precision != self.gemm_precision:
            self.drop_step_cache()
        self.gemm_precision = precision
        return self

    # ------------------------------------------------------------------------------------------
    # step cache: skip the blocks of a step and add the residual of the last computed one again
    # ------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def step_cache(self, mode, stats=False):
        """`with model.step_cache('compute' | 'skip', stats=False):` — how the forwards of the scope run.  NOT the reference's arithmetic:
        an opt-in like set_gemm_precision('mxfp8'); outside a scope nothing of it runs.
        'compute': the forward as always (the same bits), plus: the residual stream as it stands behind the patch embedding is kept
            (ws['xin']) and behind the last block r = x - xin goes to the residual buffer of this (workspace shape, context): fp32
            [L, dim], one per context, in the workspace.  stats=True also fills step_cache_stats[context key] =
            (sum |r - r_old|, sum |r_old|) — a host read per forward, for tools/step_cache_calibrate.py only; per-rank sums under SP.
        'skip': patch and time embedding as always, NO block (no weight gather, no exchange), then head(LN(x + r)) with the context's
            residual; RuntimeError when this (workspace shape, context) has none.
        Whatever invalidates the packed weights (load_state_dict, .to(), load_lora / unload_lora, set_gemm_precision) and a change of
        the workspace shape drop the residuals; drop_step_cache() frees them (3 x [L, dim] fp32: xin and two residuals under CFG)."""
        if mode not in ('compute', 'skip'):
            raise ValueError(f"step_cache mode must be 'compute' or 'skip', got {mode!r}")
        prev, self._step_mode = self._step_mode, (mode, bool(stats))
        try:
            yield self
        finally:
            self._step_mode = prev

    def drop_step_cache(self):
        """free the step cache's buffers (xin, the residuals, the reduction scratch) and forget the stats"""
        for ws in self._ws.values():
            for k in ('xin', 'resid', 'resid_stats'):
                ws.pop(k, None)
        self.step_cache_stats = {}

    @staticmethod
    def _ctx_key(ctx):
        """what names a prompt tensor: the key of _context()'s cache and of the step cache's residuals"""
        return (ctx.data_ptr(), tuple(ctx.shape), ctx._version)

    def _resid_key(self, ctx, nag=None):
        """what names a forward's residual in the step cache: the prompt tensor, and under NAG the negative prompt tensor and
        (scale, tau, alpha) too — a plain forward and a NAG forward of one prompt never share a residual"""
        key = self._ctx_key(ctx)
        return key if nag is None else (key, self._ctx_key(nag[1]), nag[0].params)

    def _step_resid(self, ws, ctx, create, nag=None):
        """the residual buffer of this workspace for prompt tensor `ctx` (zeros when new: r_old of a first computed step), or None"""
        key = self._resid_key(ctx, nag)
        table = ws.setdefault('resid', {})
        hit = table.get(key)
        if hit is None and create:
            if len(table) >= 4:         # as _context(): prompts come and go, [L, dim] fp32 each does not pile up
                table.pop(next(iter(table)))
            hit = table[key] = ((ctx, nag), torch.zeros_like(ws['x']))      # (the prompts are kept alive so that their data_ptr stays unique)
        return None if hit is None else hit[1]

    def time_embeddings(self, timesteps):
        """(e [N, dim], e0 [N, 6 dim]) fp32 of the N timesteps by the forward's own kernels (reference model.py:541-545): what the
        step-cache plan is a function of (wan/utils/step_cache.py)."""
        dev, d = self.patch_embedding.weight.device, self.dim
        tt = self._timesteps(timesteps)
        n = tt.numel()
        f32 = dict(dtype=torch.float32, device=dev)
        sin, e1 = torch.empty(1, self.freq_dim, **f32), torch.empty(d, **f32)
        e, e0 = torch.empty(n, d, **f32), torch.empty(n, 6 * d, **f32)
        for i in range(n):
            self._time_embedding(tt[i:i + 1], sin, e1, e[i], e0[i])
        return e, e0

    def _timesteps(self, t):
        """timesteps as a flat tensor on the model's device, of a dtype mg_sinusoid_embed reads (int64, fp32, fp64; any other -> fp32)"""
        tt = t.reshape(-1).to(self.patch_embedding.weight.device)
        return tt if tt.dtype in (torch.int64, torch.float32, torch.float64) else tt.to(torch.float32)

    def _time_embedding(self, tt, sin, e1, e, e0):
        ops.sinusoid_embed(tt, self.freq_dim, sin)
        te, tp = self.time_embedding, self.time_projection['1']
        ops.gemv(te['0'].weight, te['0'].bias, sin, e1)
        ops.gemv(te['2'].weight, te['2'].bias, e1, e, silu_in=True)
        ops.gemv(tp.weight, tp.bias, e, e0, silu_in=True)

    def _mx_layers(self):
        """per block {site: (e4m3 bytes [N, K], scale bytes [N, K/32])} for the sites MXFP8_SITES enables"""
        if self._shards is not None:
            raise NotImplementedError("gemm precision 'mxfp8' does not support block-sharded weights (wan.distributed.fsdp)")
        if self._mx is None:
            self._mx = [{site: ops.quant_mxfp8(lw[site]) for site, on in MXFP8_SITES.items() if on}
                        for lw in self._pack()['layers']]
        return self._mx

    def _layer(self, i):
        """GEMM operands of block i: resident, or (block-sharded mode, wan.distributed.fsdp) views of
        the all-gather buffer, with block i+1's gather already in flight on the comm stream."""
        lw = self._pack()['layers'][i]
        sh = self._shards
        if sh is None:
            return lw
        return {**lw, **sh.fetch(i)}

    def _workspace(self, L, dev):
        lay = self.sp_layout
        key = (L, str(dev), self.sp_force, lay)
        ws = self._ws.get(key)
        if ws is None:
            d, f = self.dim, self.ffn_dim
            bf, f32 = torch.bfloat16, torch.float32
            hd = d // self.num_heads
            e = lambda *s, dt=bf: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
            ws = dict(x=e(L, d, dt=f32), h=e(L, d), qkv=e(L, 3 * d), q=e(L, d), k=e(L, d), a=e(L, d),
                      u=e(L, f), tok=e(L, self.in_dim * math.prod(self.patch_size)),
                      hf=e(L, d, dt=f32), y=e(L, math.prod(self.patch_size) * self.out_dim, dt=f32),
                      sin=e(1, self.freq_dim, dt=f32), e1=e(d, dt=f32), e=e(d, dt=f32), e0=e(6, d, dt=f32),
                      mod=e(6 * self.num_layers, d, dt=f32), hmod=e(2, d, dt=f32))
            U, R = lay.U, lay.R
            n_loc, Lg = self.num_heads // U, L * U          # heads and tokens a rank attends after the Ulysses exchange
            n_att = n_loc
            if U > 1 or self.sp_force:     # pipelined packed exchange (wan/distributed/ulysses.py): buffers live there
                from ..distributed.ulysses import HeadExchange
                ws['xchg'] = HeadExchange(lay.uly_group, U, self.num_heads, hd, L, dev, max_groups=1 if R > 1 else None)
                n_att = max(n for _, n in ws['xchg'].groups)
            if hd == 128 and R == 1:   # K / V packed into 64-key tiles (operand layout of the MFMA attention kernel)
                n_pk = ops.packed_kv_numel(Lg, n_att)
                ws['kp'], ws['vp'] = e(n_pk), e(n_pk)
            if R > 1:                  # ring attention: two packed K/V blocks in flight, fp32 running result
                n1 = ops.packed_kv_numel(Lg, n_loc)
                ws['kp0'], ws['vp0'], ws['kp1'], ws['vp1'] = e(n1), e(n1), e(n1), e(n1)
                ws['part'], ws['acc'] = e(Lg, n_loc * hd), e(Lg, n_loc * hd, dt=f32)
                ws['lse'], ws['lse_acc'] = e(n_loc, Lg, dt=f32), e(n_loc, Lg, dt=f32)
            self._ws = {key: ws}  # one live shape at a time (activations are GBs at 14B/720p)
        if self.gemm_precision == 'mxfp8' and 'hq' not in ws:
            # quantised activations, added to the live workspace the first time the mode runs at this shape (a model switched between
            # the modes keeps ONE workspace): h / a share one [L, dim] pair, u has its own
            d, f, u8 = self.dim, self.ffn_dim, torch.uint8
            ws['hq'], ws['hs'] = torch.empty(L, d, dtype=u8, device=dev), torch.empty(L, d // 32, dtype=u8, device=dev)
            ws['uq'], ws['us'] = torch.empty(L, f, dtype=u8, device=dev), torch.empty(L, f // 32, dtype=u8, device=dev)
        return ws

    def _rope_tab(self, grid, dev):
        key = (tuple(grid), str(dev))
        if key not in self._rope:
            self._rope = {key: rope_cos_sin(self.dim // self.num_heads, grid).to(dev)}
        return self._rope[key]

    # ------------------------------------------------------------------------------------------
    # prompt-only work: text_embedding + per-layer cross-attention K/V (reference model.py:548-554,
    # 168-170) — independent of t, so done once per prompt tensor and cached
    # ------------------------------------------------------------------------------------------
    def _context(self, ctx):
        """-> (ctx, emb [text_len, dim] bf16, layers): `layers[i]` is block i's cross-attention _CrossKV — filled by
        _cross_kv the first time block i runs for this prompt, i.e. while that block's weights are at hand anyway
        (block-sharded mode: no extra all-gather sweep over the 28 GB of weights per new prompt)."""
        key = self._ctx_key(ctx)
        hit = self._ctx_cache.get(key)
        if hit is not None:
            return hit
        dev, d = ctx.device, self.dim
        Lc = self.text_len
        bf = torch.bfloat16
        pad = torch.zeros(Lc, self.text_dim, dtype=bf, device=dev)
        pad[:ctx.shape[0]].copy_(ctx)
        t0 = torch.empty(Lc, d, dtype=bf, device=dev)
        emb = torch.empty(Lc, d, dtype=bf, device=dev)
        te = self.text_embedding
        ops.gemm(pad, te['0'].weight, te['0'].bias, ops.BIAS_GELU_BF16, t0)
        ops.gemm(t0, te['2'].weight, te['2'].bias, ops.BIAS_BF16, emb)
        if len(self._ctx_cache) >= 4:
            self._ctx_cache.pop(next(iter(self._ctx_cache)))
        self._ctx_cache[key] = (ctx, emb, [None] * self.num_layers)  # keep ctx alive so data_ptr stays unique
        return self._ctx_cache[key]

    def _cross_kv(self, i, lw, emb, layout):
        """cross-attention K (RMS-normed) and V of block i for one prompt (reference model.py:168-170) -> _CrossKV in `layout`"""
        dev, d, hd = emb.device, self.dim, self.dim // self.num_heads
        Lc, bf = self.text_len, torch.bfloat16
        kv = torch.empty(Lc, 2 * d, dtype=bf, device=dev)
        ops.gemm(emb, lw['wkv_c'], lw['bkv_c'], ops.BIAS_BF16, kv)
        kc = torch.empty(Lc, d, dtype=bf, device=dev)
        ops.rmsnorm_rope(kv[:, :d], self.blocks[i].cross_attn.norm_k.weight, self.eps, hd, kc)
        if hd == 128 and layout == 'fused':
            return _CrossKV(*pack_tiles(kc, kv[:, d:], Lc, self.num_heads), layout)
        return _CrossKV(kc, kv[:, d:].clone(), layout)

    # the three parts of a block (reference model.py:297-311); `lin` is the block's _Linears, m its six modulation rows
    def _self_attention(self, plan, blk):
        """ws['qkv'] -> ws['a']: reference model.py:127-156 (and the Ulysses variant xdit_context_parallel.py:155-198)."""
        d, hd, N = self.dim, self.dim // self.num_heads, self.num_heads
        ws, L = plan.ws, plan.L
        qkv = ws['qkv']
        q, k, v, a = ws['q'], ws['k'], qkv[:, 2 * d:], ws['a']
        lay = self.sp_layout
        fa = plan.fa if lay.size == 1 and not self.sp_force else None
        blk.self_attn.norm_rope_qk(qkv[:, :d], qkv[:, d:2 * d], q, k, plan.rope, plan.grid, plan.pos0, prescale=fa is None)
        if fa is not None:
            # operator seam (1): the caller's function gets the reference's call (model.py:146-151): q, k roped
            # [1, L, N, hd] (UNSCALED: softmax_scale is the callee's business), v, k_lens, window_size
            y = fa(q=q.view(1, L, N, hd), k=k.view(1, L, N, hd), v=v.reshape(1, L, N, hd),
                   k_lens=torch.tensor([plan.Lfull]), window_size=self.window_size)
            a.copy_(y.reshape(L, d))
            return
        U, R = lay.U, lay.R
        tiles = (ws['kp'], ws['vp']) if 'kp' in ws else None
        # while an exchange is in flight the persistent attention grid leaves `reserve_cus` CUs to RCCL's kernels
        reserve = ws['xchg'].reserve_cus if 'xchg' in ws else 0

        def attn(qg, kg, vg, ag, heads):        # operands may be strided column views; ag contiguous
            if R > 1:                           # ring attention across the groups (hd 128 only)
                from ..distributed.ring import ring_attention
                ring_attention(qg, kg, vg, ag, ws, lay.ring_group, R, lay.ring_rank, heads, 1.0 / math.sqrt(hd), prescaled=True)
            else:                               # keys past the video's tokens are padding (k_lens)
                attend(qg, kg, vg, ag, min(kg.shape[0], plan.Lfull), heads, hd, tiles=tiles, reserve_cus=reserve)

        if U > 1 or self.sp_force:
            # Ulysses: packed q|k|v exchange per head group on the comm stream, pipelined against the attention
            # launches (xdit_context_parallel.py:185-190 / model_seq.py:232-256)
            ws['xchg'].run(q, k, v, a, attn)
        else:                                   # single GPU, or pure ring: every rank keeps all heads
            attn(q, k, v, a, N)

    def _block_self_attn(self, i, blk, plan, lin, m, share):
        """x += gate * self_attn(modulated LN(x)).  Block 0 is where forward_pair shares: 'save' keeps the stream as it stands
        behind this part (ws['x0']), 'reuse' takes that copy instead of computing it."""
        ws, x = plan.ws, plan.ws['x']
        if i == 0 and share == 'reuse':
            assert 'x0' in ws, "share='reuse' follows a share='save' forward of the same latent and t"
            x.copy_(ws['x0'])                   # block 0 up to here saw the latent and t only: the 'save' forward's stream, bit for bit
            return
        custom = _replaced_forward(blk.self_attn)
        if custom is None:
            lin.ln('wqkv', x, m[1], m[0], True, round_norm_bf16=(i == 0))
            lin('wqkv', ws['h'], lin.lw['bqkv'], ops.BIAS_BF16, ws['qkv'])
            self._self_attention(plan, blk)
            lin('self_attn.o', ws['a'], blk.self_attn.o.bias, ops.GATE_RESID_F32, x, gate=m[2])
        else:
            # operator seam (2) of the reference (text2video.py:97-100): the caller replaced
            # block.self_attn.forward — call it with the reference's arguments (the bf16 h) and keep the fused rest
            lin.ln(None, x, m[1], m[0], True, round_norm_bf16=(i == 0))
            y = custom(ws['h'][None], torch.tensor([plan.Lfull]), torch.tensor([list(plan.grid)]), self.freqs)
            ops.gate_residual(x, y[0].to(torch.bfloat16).contiguous(), m[2])
        if i == 0 and share == 'save':
            if 'x0' not in ws:
                ws['x0'] = torch.empty_like(x)
            ws['x0'].copy_(x)

    def _block_cross_attn(self, i, blk, plan, lin, ctx_emb, ctx_layers, nag=None):
        """x += cross_attn(norm3(x), text): the text keys / values are made the first time block i meets this prompt.
        nag: None, or (NAG, emb, layers) of the negative prompt: the attention runs a second time with the negative
        prompt's K/V — made and cached like the prompt's — into ws['q'] (the un-normed q projection there is dead behind norm_rope_qk),
        and ops.nag_combine mixes the two results per token in ws['a'], in front of the unchanged `o` projection."""
        ws, x, ca = plan.ws, plan.ws['x'], blk.cross_attn
        N, hd, fa = self.num_heads, self.dim // self.num_heads, plan.fa
        layout = 'fused' if fa is None else 'seam'
        if ctx_layers[i] is None or ctx_layers[i].layout != layout:
            ctx_layers[i] = self._cross_kv(i, lin.lw, ctx_emb, layout)
        kvs = [(ctx_layers[i], ws['a'])]
        if nag is not None:
            _, neg_emb, neg_layers = nag
            if neg_layers[i] is None or neg_layers[i].layout != layout:
                neg_layers[i] = self._cross_kv(i, lin.lw, neg_emb, layout)
            kvs.append((neg_layers[i], ws['q']))
        lin.ln('cross_attn.q', x, blk.norm3.weight, blk.norm3.bias, False)
        lin('cross_attn.q', ws['h'], ca.q.bias, ops.BIAS_BF16, ws['q'])
        ca.norm_rope_qk(ws['q'], None, ws['k'], None, prescale=fa is None)
        for (kc, vc, _), a in kvs:              # the prompt's into ws['a']; under NAG the negative prompt's into ws['q']
            if fa is not None:
                # operator seam (1), reference model.py:176: flash_attention(q, k, v, k_lens=context_lens) with
                # context_lens = None for T2V
                y = fa(ws['k'].view(1, plan.L, N, hd), kc.view(1, -1, N, hd), vc.reshape(1, -1, N, hd), k_lens=None)
                a.copy_(y.reshape(plan.L, self.dim))
            elif self.cross_attn_head_sharded and self.sp_layout.size > 1:
                self._cross_attention_head_sharded(ws, kc, vc, a)
            else:
                attend(ws['k'], kc, vc, a, self.text_len, N, hd, packed=True)
        if nag is not None:                     # per token over all its heads: behind head_to_seq on the head-sharded path
            ops.nag_combine(ws['a'], ws['q'], ws['a'], *nag[0].params)
        lin('cross_attn.o', ws['a'], ca.o.bias, ops.GATE_RESID_F32, x)

    def _cross_attention_head_sharded(self, ws, kc, vc, out):
        """model_seq.py:271-294: q through the seq->head all-to-all, K/V narrowed to this rank's heads (shrink_head),
        attention over ALL tokens x local heads, head->seq all-to-all back into `out`.  Same values as the token-local form."""
        from ..distributed import ulysses
        U, ug, ur = self.sp_layout.U, self.sp_layout.uly_group, self.sp_layout.uly_rank
        N, hd = self.num_heads, self.dim // self.num_heads
        nl, L = N // U, ws['k'].shape[0]
        qg = torch.empty(L * U, nl * hd, dtype=torch.bfloat16, device=ws['k'].device)
        ulysses.seq_to_head(ws['k'], qg, ug, U, N, hd)
        ag = torch.empty_like(qg)
        if hd == 128:      # packed K/V are head-major: this rank's heads are one contiguous range of tiles
            per_head = kc.numel() // N
            ks, vs = kc[ur * nl * per_head:(ur + 1) * nl * per_head], vc[ur * nl * per_head:(ur + 1) * nl * per_head]
        else:
            ks, vs = kc[:, ur * nl * hd:(ur + 1) * nl * hd], vc[:, ur * nl * hd:(ur + 1) * nl * hd]
        attend(qg, ks, vs, ag, self.text_len, nl, hd, packed=True)
        ulysses.head_to_seq(ag, out, ug, U, N, hd)

    # one forward: plan -> embed -> [step cache: open, skip exit] -> blocks -> [step cache: capture] -> head
    def _plan(self, lat, seq_len):
        """shape and placement of one forward (-> _Plan): what every later stage is told instead of working it out again"""
        C, F, H, W = lat.shape
        pt, ph, pw = self.patch_size
        assert pt == 1, 'temporal patch size 1 (reference config)'
        grid = (F, H // ph, W // pw)
        Lfull = grid[0] * grid[1] * grid[2]
        assert Lfull <= seq_len, 'seq_lens.max() <= seq_len (reference model.py:534)'
        lay = self.sp_layout
        P = lay.size
        Ltot = Lfull
        if P > 1 and self.sp_mask_padded_keys:
            # model_seq.py:704-706,757: pad to seq_len, chunk; padded keys masked through k_lens (:247-252)
            assert seq_len % P == 0 and self.num_heads % lay.U == 0 and lay.R == 1, \
                'training-side sequence parallel needs seq_len % sp == 0, heads % sp == 0 (Ulysses only)'
            Ltot = seq_len
        elif P > 1:
            # reference SP path does not mask padded keys (xdit_context_parallel.py:178-193): it is
            # only correct without padding, which is what every supported size gives
            assert seq_len == Lfull and Lfull % P == 0 and self.num_heads % lay.U == 0, \
                'sequence parallel needs L % sp == 0, heads % sp == 0 and no padding'
        L = Ltot // P
        pos0 = lay.rank * L
        n_valid = min(max(Lfull - pos0, 0), L)
        return _Plan((F, H, W), grid, Lfull, L, pos0, n_valid, self._workspace(L, lat.device), self._rope_tab(grid, lat.device),
                     _rebound_flash_attention())

    def _embed(self, plan, lat, t, patches=True):
        """patch embedding (reference model.py:529-531) of this rank's rows into the residual stream ws['x']: bf16 result, fp32 storage
        (patches=False: forward_pair brings x back whole); then the time embedding (:541-545, fp32) and the head's modulation rows"""
        ws, x, n_valid = plan.ws, plan.ws['x'], plan.n_valid
        if patches:
            _, ph, pw = self.patch_size
            if self.sp_layout.size == 1:
                ops.patchify(lat, ph, pw, ws['tok'])
            else:
                full = torch.empty(plan.Lfull, ws['tok'].shape[1], dtype=torch.bfloat16, device=lat.device)
                ops.patchify(lat, ph, pw, full)
                ws['tok'][:n_valid].copy_(full[plan.pos0:plan.pos0 + n_valid])  # torch.chunk(x, P, dim=1)[rank]
            if n_valid:
                ops.gemm(ws['tok'][:n_valid], self._packed['patch_w'], self.patch_embedding.bias, ops.BIAS_F32, x[:n_valid])
            if n_valid < plan.L:
                x[n_valid:].zero_()                      # rows padded AFTER the patch embedding (no bias), :704-706
        self._time_embedding(self._timesteps(t), ws['sin'], ws['e1'], ws['e'], ws['e0'])
        ops.add_rows(self.head.modulation.data.reshape(2, self.dim), ws['e'].reshape(1, self.dim), ws['hmod'], 1)

    def _step_open(self, ws, ctx, reuse, nag=None):
        """step cache 1/3, behind the embedding -> the residual buffer of (this workspace, ctx).
        'compute' keeps the embedded stream in ws['xin'] ('reuse': the 'save' half's copy — the same latent, the same data)."""
        if self._step_mode[0] == 'skip':
            # 'reuse' finds x as the 'save' half embedded it: a skipped forward reads the stream and never writes it
            resid = self._step_resid(ws, ctx, create=False, nag=nag)
            if resid is None:
                raise RuntimeError("step_cache('skip'): no residual for this sequence length and context — a step_cache('compute') forward "
                                   'of the same context has to come first (weight changes and drop_step_cache() drop the residuals)')
            return resid
        if 'xin' not in ws:
            assert not reuse, "share='reuse' follows a share='save' forward in the same step_cache scope"
            ws['xin'] = torch.empty_like(ws['x'])
        if not reuse:
            ws['xin'].copy_(ws['x'])
        return self._step_resid(ws, ctx, create=True, nag=nag)

    def _step_capture(self, ws, ctx, resid, nag=None):
        """step cache 3/3, behind the last block: resid <- x - xin, what the blocks added to the stream, for the skipped steps that follow"""
        if not self._step_mode[1]:
            return ops.step_resid_capture(resid, ws['x'], ws['xin'])
        if 'resid_stats' not in ws:
            ws['resid_stats'] = (torch.empty(2, dtype=torch.float64, device=resid.device), ops.step_resid_partials(resid.device))
        st, part = ws['resid_stats']
        ops.step_resid_capture(resid, ws['x'], ws['xin'], st, part)
        self.step_cache_stats[self._resid_key(ctx, nag)] = tuple(st.tolist())

    def _block(self, i, blk, plan, mx, ctx_emb, ctx_layers, share, nag=None):
        """block i on the residual stream ws['x'] (reference model.py:297-311); mx: its quantised weights, None in bf16 mode;
        nag: None, or (NAG, emb, layers) of the negative prompt for the cross-attention (_block_cross_attn)"""
        lin = _Linears(self._layer(i), mx, plan.ws, self.eps, self._mx_fuse)
        m = plan.ws['mod'][6 * i:6 * i + 6]
        self._block_self_attn(i, blk, plan, lin, m, share)
        self._block_cross_attn(i, blk, plan, lin, ctx_emb, ctx_layers, nag)
        ws = plan.ws                          # ffn: x += gate * ffn.2(GELU(ffn.0(modulated LN(x))))
        lin.ln('ffn.0', ws['x'], m[4], m[3], True)
        lin('ffn.0', ws['h'], blk.ffn['0'].bias, ops.BIAS_GELU_BF16, ws['u'])
        lin('ffn.2', ws['u'], blk.ffn['2'].bias, ops.GATE_RESID_F32, ws['x'], gate=m[5])

    @torch.no_grad()
    def _forward_one(self, lat, t, ctx, seq_len, share=None, nag=None):
        """share: None, or the two halves of forward_pair — 'save' keeps the residual stream as it stands behind block 0's self-attention
        (ws['x0']), 'reuse' starts from that copy instead of recomputing it (same latent, same t: nothing before that point reads `ctx`).
        nag: None, or (NAG, the negative prompt tensor of this sample) — normalized attention guidance in every cross-attention."""
        pk = self._pack()
        lat = lat.to(torch.float32).contiguous()
        plan = self._plan(lat, seq_len)
        ws, x = plan.ws, plan.ws['x']
        self._embed(plan, lat, t, patches=share != 'reuse')       # ('reuse': x comes back whole behind block 0's self-attention)
        resid = self._step_open(ws, ctx, share == 'reuse', nag) if self._step_mode else None
        if resid is not None and self._step_mode[0] == 'skip':
            # step cache 2/3, the skip exit: no block runs — the residual the blocks added at this context's last computed step is added
            # again, inside the head's LayerNorm
            ops.resid_ln_modulate(x, resid, ws['hmod'][1], ws['hmod'][0], self.eps, ws['hf'])
            return self._head_out(ws, plan.grid, plan.fhw, lat.device)

        ops.add_rows(pk['modulation'], ws['e0'], ws['mod'], 6)                       # model.py:292-295
        _, ctx_emb, ctx_layers = self._context(ctx)
        nagb = None if nag is None else (nag[0], *self._context(nag[1])[1:])         # the negative prompt: embedded and cached like any prompt
        mxl = self._mx_layers() if self.gemm_precision == 'mxfp8' else None
        for i, blk in enumerate(self.blocks):
            self._block(i, blk, plan, mxl[i] if mxl is not None else None, ctx_emb, ctx_layers, share, nagb)
        if resid is not None:
            self._step_capture(ws, ctx, resid, nag)

        # head (model.py:333-343): fp32 end to end
        ops.ln_modulate(x, ws['hmod'][1], ws['hmod'][0], True, self.eps, ws['hf'])
        return self._head_out(ws, plan.grid, plan.fhw, lat.device)

    def _head_out(self, ws, grid, fhw, dev):
        """head Linear on ws['hf'], the SP all-gather and unpatchify (model.py:342, :561-565)"""
        lay = self.sp_layout
        ops.head_gemm(ws['hf'], self.head.head.weight, self.head.head.bias, ws['y'])
        y = ws['y']
        if lay.size > 1:
            from ..distributed import ulysses
            y = ulysses.all_gather_seq(ws['y'], lay.group, lay.size)                  # get_sp_group().all_gather
        out = torch.empty(self.out_dim, *fhw, dtype=torch.float32, device=dev)
        ops.unpatchify(y, self.out_dim, grid[0], grid[1], grid[2], self.patch_size[1], self.patch_size[2], out)
        return out

    def _retry_without_peer_copies(self, run):
        """run() = the forward(s) of one call.  If a copy of the copy-engine transport was refused on some rank meanwhile (every rank
        reads the same answer), the whole group goes back to the all-to-all collective, for good, and run() is repeated on it."""
        out = run()
        return run() if self._peer_transport_failed() else out

    @staticmethod
    def _checked_nag(nag, n):
        """forward's nag= -> one (NAG, negative prompt tensor) per sample, or [None] * n"""
        if nag is None:
            return [None] * n
        from ..utils.nag import NAG
        try:
            rule, negs = nag
            negs = list(negs)
        except (TypeError, ValueError):
            raise ValueError(f'nag must be None or (NAG, [negative context tensors]), got {nag!r}') from None
        if not isinstance(rule, NAG) or len(negs) != n or not all(torch.is_tensor(c) and c.dim() == 2 for c in negs):
            raise ValueError(f'nag must be (wan.utils.nag.NAG, [one [len, text_dim] negative context tensor per sample: {n}]), got {nag!r}')
        return [(rule, c) for c in negs]

    def forward(self, x, t, context, seq_len, clip_fea=None, y=None, *, nag=None):
        """nag (NOT part of the reference): None = the forward as it is, call for call; or (NAG, [negative context tensors]),
        one tensor per sample — normalized attention guidance: every block's cross-attention runs a second time with the negative prompt's
        K/V and ops.nag_combine mixes the two results per token in front of the `o` projection.  The negative prompt is embedded and its
        K/V are made once and cached like any prompt's (the prompt cache holds 4 prompts; a guided call with NAG uses up to 3: the prompt,
        the call's negative prompt and NAG's own if it differs).  In a step_cache scope the residual of a NAG forward is kept under
        (prompt, negative prompt, (scale, tau, alpha)): a plain forward and a NAG forward of one prompt never share one."""
        if clip_fea is not None or y is not None:
            raise NotImplementedError('image conditioning (i2v) is not part of MoviiGen1.1 T2V')
        nags = self._checked_nag(nag, len(context))
        t = t.reshape(-1)
        return self._retry_without_peer_copies(lambda: [self._forward_one(u, t[i if t.numel() > 1 else 0], c, seq_len, nag=nags[i])
                                                        for i, (u, c) in enumerate(zip(x, context))])

    def forward_pair(self, x, t, context, context_null, seq_len, *, nag=None):
        """The two guidance branches of ONE denoising step (reference text2video.py:237-240: two calls of the model on the same latent and t,
        with the prompt's and the negative prompt's embeddings) -> (cond, uncond), each what forward() returns for its context, bit for bit.
        Nothing in front of block 0's cross-attention reads the context — patch embedding, time embedding, and block 0's modulated LayerNorm,
        q|k|v projection, RMS-norm + RoPE, self-attention over all L tokens and its gated residual see the latent and t only — so the second
        branch starts from a copy of the first one's residual stream at that point (2.7 GB at 1920x832x81f) instead of computing it again:
        one self-attention launch and four GEMMs of 80 per step.  A replaced self-attention forward or a rebound flash_attention (the operator
        seams) may be anything, also non-deterministic: then, and with MOVIIGEN_CFG_SHARED_PREFIX=0, the branches run as two plain forwards.
        nag: as in forward(), for the conditional half only; the other half runs plain (block 0's shared prefix reads no context)."""
        plain = os.environ.get('MOVIIGEN_CFG_SHARED_PREFIX', '1') == '0' or _rebound_flash_attention() is not None or \
            _replaced_forward(self.blocks[0].self_attn) is not None or len(x) != 1 or len(context) != 1 or len(context_null) != 1
        if plain:
            return self.forward(x, t, context, seq_len, nag=nag), self.forward(x, t, context_null, seq_len)
        nag0 = self._checked_nag(nag, 1)[0]
        t = t.reshape(-1)
        return self._retry_without_peer_copies(lambda: ([self._forward_one(x[0], t[0], context[0], seq_len, share='save', nag=nag0)],
                                                        [self._forward_one(x[0], t[0], context_null[0], seq_len, share='reuse')]))


    def _peer_transport_failed(self):
        """once per forward (one 4-byte read per open window set — nothing at all on the default collective transport): did a peer copy
        fail?  If so every HeadExchange of this model drops its windows (wan/distributed/peer_copy.py)."""
        xs = [w['xchg'] for w in self._ws.values() if 'xchg' in w]
        xs = [x for x in xs if x.peer is not None]
        if not xs or not any(x.peer_failed() for x in xs):
            return False
        for x in xs:
            x.drop_peer()
        return True

    def unpatchify(self, x, grid_sizes):
        outs = []
        for u, v in zip(x, grid_sizes.tolist()):
            f, h, w = v
            out = torch.empty(self.out_dim, f * self.patch_size[0], h * self.patch_size[1], w * self.patch_size[2],
                              dtype=torch.float32, device=u.device)
            ops.unpatchify(u.to(torch.float32).contiguous(), self.out_dim, f, h, w, self.patch_size[1],
                           self.patch_size[2], out)
            outs.append(out)
        return outs
