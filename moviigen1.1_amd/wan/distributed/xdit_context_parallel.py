"""Sequence-parallel entry points with the reference's names (wan/distributed/
xdit_context_parallel.py:65-198).  The reference installs `usp_dit_forward` / `usp_attn_forward`
by method replacement around xfuser; here sequence parallelism is a property of the engine
(WanModel.sp_layout: an SpLayout of layout.py, installed by WanModel.set_sp_layout alone) and the collectives are
in ulysses.py.  `usp_dit_forward` configures it and runs the fused forward; `usp_attn_forward` is the stand-alone sequence-parallel attention operator with the
reference's call shape, so the reference's installation sequence (text2video.py:97-100)

    for block in model.blocks:
        block.self_attn.forward = types.MethodType(usp_attn_forward, block.self_attn)
    model.forward = types.MethodType(usp_dit_forward, model)

works unchanged."""
import torch.distributed as dist

from .layout import SpLayout


def enable_sequence_parallel(model, group=None):
    """shard the token axis of `model` over `group` (default: WORLD).  heads % size must be 0."""
    if not dist.is_initialized():
        raise RuntimeError('torch.distributed is not initialised (launch with torchrun, one process per GPU)')
    return model.set_sp_layout(SpLayout.ulysses(group))


def usp_dit_forward(self, x, t, context, seq_len, clip_fea=None, y=None, guidance=None):
    if self.sp_size == 1 and dist.is_initialized() and dist.get_world_size() > 1:
        enable_sequence_parallel(self)
    return type(self).forward(self, x, t, context, seq_len, clip_fea=clip_fea, y=y)


def usp_attn_forward(self, x, seq_lens, grid_sizes, freqs, dtype=None):
    """reference xdit_context_parallel.py:155-198, same call shape: `self` is a block's self-attention module,
    x [B, L/P, C] the rank's token shard; RoPE with the rank's position offset, packed q|k|v all-to-all, attention over
    all tokens x heads/P, all-to-all back, output projection.  Installing it with
    `types.MethodType(usp_attn_forward, block.self_attn)` (reference text2video.py:97-100) is honoured: WanModel.forward
    recognises it and keeps its fused, pipelined implementation of exactly this operator."""
    # self.sp: the tag WanModel.set_sp_layout wrote.  A module no layout was ever installed on (only the class default None is there) gets
    # the reference's default, Ulysses over WORLD — once, then it is the module's tag
    if 'sp' not in vars(self) and dist.is_initialized() and dist.get_world_size() > 1:
        self.sp = SpLayout.ulysses()
    return type(self).forward(self, x, seq_lens, grid_sizes, freqs, sp=self.sp)
