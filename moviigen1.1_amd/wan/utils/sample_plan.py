"""The plan of one WanT2V.generate / inpaint call: what each step of the sampling loop does, resolved before step 0 from
the three plans that are functions of the schedule alone — the guidance kinds (wan/utils/guidance.py), the step-cache plan
(wan/utils/step_cache.py) and the window starts (wan/utils/context_windows.py).  Pure host code, no GPU in it; the same on every rank.
"""
from collections import namedtuple

from .guidance import adjust_step_plan

# steps: one (i, kind, cache) per schedule index the loop runs, i0 .. n - 1: kind 'zero' | 'cond' | 'guided', cache the WanModel.step_cache
#     scope the step's forwards run in, None | 'skip' | 'compute'
# kinds / step_plan / window_starts: what WanT2V.last_guidance_plan / last_step_plan / last_window_plan publish (None: that feature is off)
# stats: the step cache's 'compute' scopes fill model.step_cache_stats (the calibration tool)
# any_guided: some step of the call runs both branches — the uncond buffers and the scratch of the three-launch mix are needed
SamplePlan = namedtuple('SamplePlan', 'steps kinds step_plan window_starts stats any_guided')


def refuse_windows_with_step_cache(window_starts, step_cache):
    """either argument None = that feature is off; step_cache: the argument of `generate` or its resolved plan"""
    if window_starts is not None and step_cache is not None:
        raise ValueError('windows cannot be combined with step_cache: the cached residuals would be per window (not built); pass step_cache=None')


def sample_plan(n, i0, kinds=None, step_plan=None, stats=False, own_branch_only=False, window_starts=None):
    """n schedule indices, the loop runs i0 .. n - 1.  kinds: Guidance.plan's list, None = no Guidance, every step 'guided'.
    step_plan, stats: resolve_plan's result (list of bools per schedule index, True = compute; None = no step cache); with kinds it is made
    consistent with them here (adjust_step_plan; own_branch_only: cfg-parallel groups).  window_starts: WindowPlan.starts, None = one pass.

    A step's cache scope: 'skip' when the adjusted plan says so; 'compute' — the forward as always, plus its residual kept — only when
    the next schedule index is skipped and adds it again, or when stats is on; None otherwise, and for a 'zero' step, which runs no forward."""
    refuse_windows_with_step_cache(window_starts, step_plan)
    if step_plan is not None and kinds is not None:
        step_plan = adjust_step_plan(step_plan, kinds, i0, own_branch_only=own_branch_only)
    steps = []
    for i in range(i0, n):
        kind = 'guided' if kinds is None else kinds[i]
        cache = None
        if step_plan is not None and kind != 'zero':
            if not step_plan[i]:
                cache = 'skip'
            elif stats or (i + 1 < n and not step_plan[i + 1]):
                cache = 'compute'
        steps.append((i, kind, cache))
    return SamplePlan(steps, kinds, step_plan, None if window_starts is None else list(window_starts), bool(stats),
                      any(kind == 'guided' for _, kind, _ in steps))
