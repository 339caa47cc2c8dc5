"""Guidance options for WanT2V.generate: which steps run both guidance branches, and how the two predictions are mixed.
NOT the reference's arithmetic — an opt-in, never the default.

    interval        guide only while lo <= sigma_i <= hi (Kynkaanniemi et al. 2024, "Applying guidance in a limited interval"): outside
                    the band only the conditional branch runs, one DiT forward instead of two
    zero_star       CFG-Zero* (Fan et al. 2025): the unconditional prediction is rescaled by the projection s* = <c, u> / |u|^2 before
                    the mix; zero_init_steps: the first steps of the schedule predict zero, no forward at all
    rescale         guidance rescale (Lin et al. 2024): the guided prediction is pulled back towards the standard deviation of the
                    conditional one by the factor phi

The plan is a function of the schedule alone: known before the loop, the same on every rank.  Pure host code, no GPU in it; the mix
itself is wan.backend.ops.cfg_stats / cfg_coefficients / cfg_combine_coef.
"""
import math
import operator

STEP_KINDS = ('zero', 'cond', 'guided')


class Guidance:
    """scale: the guide scale g of the guided steps, None = the call's `guide_scale`.  interval = (lo, hi), 0 <= lo <= hi <= 1.
    zero_star / zero_init_steps / rescale: see the module's docstring; rescale in [0, 1], 0 = off."""

    def __init__(self, scale=None, interval=(0.0, 1.0), zero_star=False, zero_init_steps=0, rescale=0.0):
        if scale is not None:
            scale = float(scale)
            if not math.isfinite(scale):
                raise ValueError(f'scale must be finite or None, got {scale!r}')
        try:
            lo, hi = (float(v) for v in interval)
        except (TypeError, ValueError):
            raise ValueError(f'interval must be (lo, hi), got {interval!r}') from None
        if not 0.0 <= lo <= hi <= 1.0:
            raise ValueError(f'interval must satisfy 0 <= lo <= hi <= 1, got ({lo}, {hi})')
        if isinstance(rescale, bool) or not 0.0 <= float(rescale) <= 1.0:
            raise ValueError(f'rescale must be in [0, 1], got {rescale!r}')
        try:
            if isinstance(zero_init_steps, bool):
                raise TypeError
            steps = operator.index(zero_init_steps)
        except TypeError:
            raise ValueError(f'zero_init_steps must be an integer >= 0, got {zero_init_steps!r}') from None
        if steps < 0:
            raise ValueError(f'zero_init_steps must be an integer >= 0, got {zero_init_steps!r}')
        self.scale, self.interval, self.zero_star, self.zero_init_steps, self.rescale = scale, (lo, hi), bool(zero_star), steps, float(rescale)

    @property
    def plain_mix(self):
        """the guided steps mix as the reference does, u + g (c - u): neither CFG-Zero* nor rescale"""
        return not self.zero_star and self.rescale == 0.0

    def plan(self, sigmas, i0=0):
        """sigmas: one per schedule index, sigmas[i] = the noise level step i starts from (scheduler.sigmas without its final 0, both
        solvers) -> one of 'zero' | 'cond' | 'guided' per index: 'zero' for i < zero_init_steps, else 'guided' where lo <= sigma_i <= hi,
        else 'cond'.  i0: the schedule index the loop starts at (video-to-video); the entries in front of it never run and are planned
        like every other, so a start at i0 >= zero_init_steps zeroes nothing."""
        sigmas = [float(s) for s in sigmas]
        if sigmas and not 0 <= int(i0) < len(sigmas):
            raise ValueError(f'i0 must be a schedule index in [0, {len(sigmas)}), got {i0}')
        lo, hi = self.interval
        return ['zero' if i < self.zero_init_steps else 'guided' if lo <= s <= hi else 'cond' for i, s in enumerate(sigmas)]

    def __repr__(self):
        return (f'Guidance(scale={self.scale}, interval={self.interval}, zero_star={self.zero_star}, zero_init_steps={self.zero_init_steps}, '
                f'rescale={self.rescale})')


def adjust_step_plan(plan, kinds, i0=0, own_branch_only=False):
    """a step-cache plan (list of bools, True = compute; wan.utils.step_cache) made consistent with a guidance plan: the residuals are kept
    per context, so after a stretch of 'cond' steps the unconditional one is arbitrarily old — a 'guided' step is computed when the last
    step that ran a forward was not 'guided', and the first step that runs a forward is computed ('zero' steps run none).
    own_branch_only (cfg-parallel groups: a 'guided' step leaves a rank the residual of its own branch alone, so the unconditional half
    has none for the prompt): a 'cond' step behind a 'guided' one is computed too.  The same plan on every rank."""
    plan, last = list(plan), None
    for i in range(i0, len(plan)):
        if kinds[i] == 'zero':
            continue
        if last is None or (kinds[i] != last and (kinds[i] == 'guided' or own_branch_only)):
            plan[i] = True
        last = kinds[i]
    return plan
