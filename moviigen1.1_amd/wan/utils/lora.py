"""LoRA adapter files for the DiT: host-side parsing only.  `read_lora` turns a `.safetensors` file (or a dict of tensors) into
{module name: (up fp32 [N, r], down fp32 [r, K], alpha or None)}; it does no arithmetic on weights — the scale strength * alpha / r
and the merge itself are WanModel.load_lora's, on the device (mg_lora_merge).

Spellings: PEFT / diffusers `<m>.lora_A.weight` (down) + `<m>.lora_B.weight` (up); kohya / ComfyUI `<m>.lora_down.weight` +
`<m>.lora_up.weight`; an optional scalar `<m>.alpha`.  `<m>` is a module name of the model (`blocks.3.cross_attn.k`, `blocks.0.ffn.2`,
`text_embedding.0`, ...), optionally behind one of PREFIXES, or kohya's flat form `lora_unet_blocks_3_cross_attn_k`.  The flat form is
looked up in a table built from the model's own names with '.' replaced by '_': it cannot be split on '_', `self_attn`, `cross_attn`
and `text_embedding_0` contain underscores themselves.
"""
import logging
from collections.abc import Mapping

import torch

__all__ = ['read_lora', 'PREFIXES']

PREFIXES = ('model.diffusion_model.', 'diffusion_model.', 'transformer.')
_ROLE = {'.lora_A.weight': 'down', '.lora_down.weight': 'down', '.lora_B.weight': 'up', '.lora_up.weight': 'up', '.alpha': 'alpha'}
# what a merge of up @ down cannot express.  Full-weight / bias / norm deltas (`.diff`, `.diff_b`) and keys of other modules can be
# skipped (strict=False); never skippable are the keys an adapter NEEDS to mean what its author trained: DoRA magnitudes, LoHa / LoKr
_FATAL = ('.dora_scale', '.hada_w1_a', '.hada_w1_b', '.hada_w2_a', '.hada_w2_b', '.hada_t1', '.hada_t2', '.lokr_w1', '.lokr_w2',
          '.lokr_w1_a', '.lokr_w1_b', '.lokr_w2_a', '.lokr_w2_b', '.lokr_t2')
_FLAT = 'lora_unet_'


def _first(keys, n=5):
    keys = sorted(keys)
    return ', '.join(keys[:n]) + (f', ... ({len(keys)} keys)' if len(keys) > n else '')


def read_lora(src, module_names, strict=True):
    """src: a `.safetensors` path or a dict {key: tensor}.  module_names: the targets the model offers — a mapping
    {name: (out_features, in_features)} (the factors' shapes are then checked against it) or just an iterable of names.
    -> {name: (up fp32 [N, r], down fp32 [r, K], alpha float or None)}, on the CPU.
    strict=True: any key that is not a factor or an alpha of one of `module_names` raises ValueError.  strict=False: `.diff`, `.diff_b`
    and keys of unknown targets are skipped with one logged warning; DoRA / LoHa / LoKr keys, a factor without its partner and a factor
    whose shape does not fit its target raise either way."""
    if isinstance(src, Mapping):
        tensors = src
    else:
        from safetensors.torch import load_file
        tensors = load_file(str(src), device='cpu')
    shapes = dict(module_names) if isinstance(module_names, Mapping) else {n: None for n in module_names}
    flat = {}
    for name in shapes:
        if flat.setdefault(name.replace('.', '_'), name) != name:
            raise ValueError(f"module names {flat[name.replace('.', '_')]!r} and {name!r} have the same flat spelling")

    parts, fatal, skipped = {}, [], []
    for key in tensors:
        if key.endswith(_FATAL):
            fatal.append(key)
            continue
        suffix = next((s for s in _ROLE if key.endswith(s)), None)
        if suffix is None:
            skipped.append(key)             # .diff / .diff_b, or nothing this reader knows
            continue
        mod = key[:-len(suffix)]
        for p in PREFIXES:
            if mod.startswith(p):
                mod = mod[len(p):]
                break
        if mod not in shapes and mod.startswith(_FLAT):
            mod = flat.get(mod[len(_FLAT):], mod)
        if mod not in shapes:
            skipped.append(key)             # not a linear layer of this model
            continue
        if _ROLE[suffix] in parts.setdefault(mod, {}):
            raise ValueError(f'adapter names the {_ROLE[suffix]} factor of {mod} twice ({key})')
        parts[mod][_ROLE[suffix]] = tensors[key]
    if fatal:
        raise ValueError(f'adapter needs more than a low-rank merge (DoRA / LoHa / LoKr are not supported): {_first(fatal)}')
    if skipped:
        what = f'adapter keys that are no low-rank factor of a linear layer of this model: {_first(skipped)}'
        if strict:
            raise ValueError(what + ' (strict=False skips them)')
        logging.warning('skipped ' + what)

    out = {}
    for mod, p in parts.items():
        if 'up' not in p or 'down' not in p:
            raise ValueError(f"adapter has only {sorted(p)} for {mod}: the 'up' and the 'down' factor are both needed")
        up, down = p['up'].to(torch.float32), p['down'].to(torch.float32)      # fp16 / bf16 / fp32 files: widening is exact
        want = shapes[mod]
        if up.dim() != 2 or down.dim() != 2 or up.shape[1] != down.shape[0] or up.shape[1] < 1 or \
                (want is not None and (up.shape[0], down.shape[1]) != tuple(want)):
            raise ValueError(f'adapter factors of {mod} do not fit: up {tuple(up.shape)}, down {tuple(down.shape)}'
                             + (f', weight {tuple(want)}' if want is not None else ''))
        alpha = p.get('alpha')
        out[mod] = (up.contiguous(), down.contiguous(), None if alpha is None else float(alpha.reshape(-1)[0]))
    return out
