"""Normalized attention guidance for WanModel / WanT2V: a negative prompt that acts inside every cross-attention, so
that it survives steps that run the conditional branch alone.  NOT the reference's arithmetic — an opt-in, never the default.

Chen et al. 2025, "Normalized Attention Guidance": per token row, with p / n the cross-attention outputs for the positive / negative
prompt (all heads of the token), g = scale p - (scale - 1) n is clipped to tau times the L1 norm of p and blended with p by alpha; the
result replaces p in front of the `o` projection (wan.backend.ops.nag_combine, mg_nag_combine_bf16).  One more short-key attention launch
and one row-wise pass per block instead of a second DiT forward.

The recipe for "a negative prompt at one forward per step":
    generate(..., guidance=Guidance(interval=(0.0, 0.0)), nag=NAG(scale, n_prompt=...))
No sigma of a schedule is 0, so every step is 'cond' (one forward); the negative prompt enters through NAG alone.

Pure host code, no GPU in it.
"""
import math

MAX_SCALE = 64.0


class NAG:
    """scale in [1, 64]: how far the attention output is pushed away from the negative prompt's (1 = off: the result is the plain
    forward, bit for bit).  tau >= 1: the L1 norm of the pushed row is held at most tau times the positive row's.  alpha in [0, 1]: the
    weight of the pushed row in the blend with the positive one.  The defaults of tau and alpha are the paper's, not a recommendation of
    this project.  n_prompt: the negative prompt NAG pushes away from, text or a pre-computed embedding as WanT2V.generate's n_prompt;
    None = the call's n_prompt.

    Why 64: the promise that an equal negative prompt changes nothing rests on scale p - (scale - 1) p landing within half a bf16 ulp
    (2^-9) of p; its fp32 error is about 2 scale 2^-24, 2^-17 at the cap — a margin of 2^8, with room for every scale in use (the
    paper's go to 11)."""

    def __init__(self, scale, tau=2.5, alpha=0.25, n_prompt=None):
        vals = {}
        for name, v in (('scale', scale), ('tau', tau), ('alpha', alpha)):
            if isinstance(v, bool):
                raise ValueError(f'{name} must be a number, got {v!r}')
            try:
                v = float(v)
            except (TypeError, ValueError):
                raise ValueError(f'{name} must be a number, got {v!r}') from None
            if not math.isfinite(v):
                raise ValueError(f'{name} must be finite, got {v!r}')
            vals[name] = v
        if not 1.0 <= vals['scale'] <= MAX_SCALE:
            raise ValueError(f"scale must be in [1, {MAX_SCALE:g}], got {vals['scale']}")
        if vals['tau'] < 1.0:
            raise ValueError(f"tau must be >= 1, got {vals['tau']}")
        if not 0.0 <= vals['alpha'] <= 1.0:
            raise ValueError(f"alpha must be in [0, 1], got {vals['alpha']}")
        self.scale, self.tau, self.alpha, self.n_prompt = vals['scale'], vals['tau'], vals['alpha'], n_prompt

    @property
    def params(self):
        """(scale, tau, alpha): what the kernel is given, and what names a NAG forward's residual in the step cache"""
        return self.scale, self.tau, self.alpha

    def __repr__(self):
        n = self.n_prompt
        n = None if n is None else (n if isinstance(n, str) else '<embedding>')
        return f'NAG(scale={self.scale}, tau={self.tau}, alpha={self.alpha}, n_prompt={n!r})'
