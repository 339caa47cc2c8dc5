"""Step cache (TeaCache-style) for WanT2V.generate: which denoising steps run the DiT blocks and which add the last computed step's
residual again (WanModel.step_cache).  NOT the reference's arithmetic — an opt-in, never the default.

For Wan the indicator reads only the time embedding — `e0` [6 dim] (or `e` [dim]) — a function of the timestep and the weights alone.
So the whole plan is known before the loop starts, it is the same on every sequence-parallel rank, every CFG-parallel rank and both
guidance branches without a collective, and the loop needs no host sync for it.

    plan_from_distances(d, thresh, ...)          the rule, pure host code in fp64
    step_cache_plan(model, timesteps, thresh)    the distances from the model's own time-embedding kernels, then the rule
    resolve_plan(spec, model, timesteps, i0)     what WanT2V.generate(step_cache=spec) runs
"""
import math

import numpy as np

IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0)     # polyval coefficients, highest power first: p(d) = d — the threshold then bounds the summed raw distance
SOURCES = ('e0', 'e')


def plan_from_distances(d, thresh, coefficients=IDENTITY, keep_first=1, keep_last=1, first=0):
    """d[i] = relative L1 distance of step i's time embedding to step i-1's (d[0] is not read) -> list of bools, True = compute.
    TeaCache's rule: step 0, the first keep_first and the last keep_last steps are computed; for every other step
    acc += polyval(coefficients, d[i]), skipped while acc < thresh, else computed and acc = 0.  d[i] is always measured against the
    PREVIOUS step, computed or not; the accumulator starts at 0 and is also 0 behind every computed step.
    first: the schedule index the loop starts at (video-to-video): it takes step 0's place — computed, keep_first counts from it, the
    accumulator starts behind it — and the entries in front of it, which never run, read True."""
    d = [float(v) for v in d]
    n = len(d)
    thresh, keep_first, keep_last, first = float(thresh), int(keep_first), int(keep_last), int(first)
    coefficients = [float(c) for c in coefficients]
    if not coefficients or not all(math.isfinite(c) for c in coefficients):
        raise ValueError(f'coefficients must be finite numbers, highest power first, got {coefficients!r}')
    if math.isnan(thresh) or thresh < 0 or keep_first < 0 or keep_last < 0:
        raise ValueError(f'thresh >= 0, keep_first >= 0, keep_last >= 0 expected, got {thresh}, {keep_first}, {keep_last}')
    if n and not 0 <= first < n:
        raise ValueError(f'first must be a schedule index in [0, {n}), got {first}')
    plan, acc = [], 0.0
    for i in range(n):
        if i <= first or i - first < keep_first or i >= n - keep_last:
            compute = True
        else:
            if not math.isfinite(d[i]):
                raise ValueError(f'distance {i} is not finite: {d[i]}')
            acc += float(np.polyval(coefficients, d[i]))
            compute = not acc < thresh
        if compute:
            acc = 0.0
        plan.append(compute)
    return plan


def embedding_distances(emb):
    """emb [N, K] (any float array) -> d [N] fp64, d[i] = sum |emb[i] - emb[i-1]| / sum |emb[i-1]|, d[0] = 0"""
    emb = np.asarray(emb, dtype=np.float64)
    d = np.zeros(emb.shape[0], dtype=np.float64)
    for i in range(1, emb.shape[0]):
        d[i] = np.abs(emb[i] - emb[i - 1]).sum() / np.abs(emb[i - 1]).sum()
    return d


def step_distances(model, timesteps, source='e0'):
    """the N time embeddings by the model's own kernels (N x 3 gemv launches), ONE transfer to the host, distances in fp64"""
    if source not in SOURCES:
        raise ValueError(f'source must be one of {SOURCES}, got {source!r}')
    e, e0 = model.time_embeddings(timesteps)
    return embedding_distances((e0 if source == 'e0' else e).cpu().numpy())


def step_cache_plan(model, timesteps, thresh, coefficients=IDENTITY, source='e0', keep_first=1, keep_last=1, first=0):
    """the plan (list of bools, True = compute, one per timestep) of a schedule for `model`; see plan_from_distances"""
    return plan_from_distances(step_distances(model, timesteps, source), thresh, coefficients, keep_first, keep_last, first)


def resolve_plan(spec, model, timesteps, i0=0):
    """WanT2V.generate's `step_cache` argument -> (plan or None, stats).  spec: None; a float threshold; a dict of step_cache_plan's
    arguments (thresh, coefficients, source, keep_first, keep_last) or {'plan': [...]}, either with an optional 'stats': True (every
    computed step then captures its residual and fills model.step_cache_stats — the calibration tool); or an explicit plan, one bool
    per SCHEDULE index.  The first step that runs (i0, video-to-video) is always computed."""
    if spec is None:
        return None, False
    n = len(timesteps)
    stats = False
    if isinstance(spec, dict):
        spec = dict(spec)
        stats = bool(spec.pop('stats', False))
        if 'plan' in spec:
            if len(spec) != 1:
                raise ValueError(f"step_cache: 'plan' excludes {sorted(k for k in spec if k != 'plan')}")
            spec = spec['plan']
        else:
            if 'thresh' not in spec:
                raise ValueError("step_cache: a dict needs 'thresh' or 'plan'")
            spec = step_cache_plan(model, timesteps, first=i0, **spec)
    elif isinstance(spec, (bool, str)):
        raise TypeError(f'step_cache must be None, a threshold, a dict or a list of bools, got {spec!r}')
    elif isinstance(spec, (int, float)):
        spec = step_cache_plan(model, timesteps, float(spec), first=i0)
    plan = [bool(v) for v in spec]
    if len(plan) != n:
        raise ValueError(f'step_cache: a plan has one entry per schedule index: {n} expected, got {len(plan)}')
    if n:
        plan[i0] = True
    return plan, stats
