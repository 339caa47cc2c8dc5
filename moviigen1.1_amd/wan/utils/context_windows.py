"""Context windows for WanT2V.generate: a latent longer than one DiT pass is denoised as a whole, but in every step the
DiT sees it through overlapping windows of a fixed number of latent frames, and the per-window predictions are blended back into one
whole-clip prediction before the scheduler steps.  NOT the reference's loop — an opt-in, never the default.

The plan is a function of (F, Fw, O, fuse) alone: known before the loop, the same on every rank.  Pure host code, no GPU in it; the two
passes are wan.backend.ops.window_gather / window_blend.
"""
import operator

import torch

FUSES = ('pyramid', 'flat')


def _index(v, name):
    try:
        if isinstance(v, bool):
            raise TypeError
        return operator.index(v)
    except TypeError:
        raise ValueError(f'{name} must be an integer, got {v!r}') from None


class WindowPlan:
    """what `ContextWindows.plan` returns for a latent of F > Fw frames:
    starts      the first latent frame f0_k of every window, ascending, no duplicate; every window has Fw frames
    weights64   [K][Fw] Python floats: w~_k(f0_k + j) = r(j) / (the sum of r over the windows that cover the frame)
    weights     the same, rounded once to fp32: a [K, Fw] float32 CPU tensor (a frame covered by one window has exactly 1.0)
    first       [K, Fw] uint8 CPU tensor: 1 exactly when no earlier window covers the frame"""

    def __init__(self, F, Fw, starts, raw):
        self.F, self.Fw, self.starts = F, Fw, list(starts)
        total = [0] * F                     # (integers: the raw weights are, so the denominators are exact)
        for f0 in self.starts:
            for j in range(Fw):
                total[f0 + j] += raw[j]
        self.weights64 = [[raw[j] / total[f0 + j] for j in range(Fw)] for f0 in self.starts]
        self.weights = torch.tensor(self.weights64, dtype=torch.float64).to(torch.float32)
        seen, first = [False] * F, []
        for f0 in self.starts:
            first.append([0 if seen[f0 + j] else 1 for j in range(Fw)])
            for j in range(Fw):
                seen[f0 + j] = True
        assert all(seen)
        self.first = torch.tensor(first, dtype=torch.uint8)

    def cover(self, f):
        """the indices k of the windows that cover latent frame f"""
        return [k for k, f0 in enumerate(self.starts) if f0 <= f < f0 + self.Fw]


class ContextWindows:
    """frames: the pixel frames of one window, as `frame_num` counts them ((frames - 1) % stride == 0); overlap: the pixel frames two
    neighbouring windows share (overlap % stride == 0); fuse: the raw weight of a window's j-th latent frame, 'pyramid' =
    min(j + 1, Fw - j) or 'flat' = 1.  stride: the temporal stride of the VAE (config.vae_stride[0]; `generate` checks it).
    In latent frames: Fw = (frames - 1) / stride + 1 and O = overlap / stride, 0 <= O < Fw."""

    def __init__(self, frames=81, overlap=16, fuse='pyramid', stride=4):
        frames, overlap, stride = _index(frames, 'frames'), _index(overlap, 'overlap'), _index(stride, 'stride')
        if stride < 1:
            raise ValueError(f'stride must be positive, got {stride}')
        if frames < 1 or (frames - 1) % stride:
            raise ValueError(f'frames must be 1 + a multiple of {stride} (the VAE\'s temporal stride), got {frames}')
        if overlap % stride:
            raise ValueError(f'overlap must be a multiple of {stride} (the VAE\'s temporal stride), got {overlap}')
        Fw, O = (frames - 1) // stride + 1, overlap // stride
        if not 0 <= O < Fw:
            raise ValueError(f'overlap must leave 0 <= overlap / {stride} < {Fw} latent frames, got {overlap}')
        if fuse not in FUSES:
            raise ValueError(f'fuse must be one of {FUSES}, got {fuse!r}')
        self.frames, self.overlap, self.fuse, self.stride, self.Fw, self.O = frames, overlap, fuse, stride, Fw, O

    def raw_weights(self):
        Fw = self.Fw
        return [min(j + 1, Fw - j) if self.fuse == 'pyramid' else 1 for j in range(Fw)]

    def plan(self, F):
        """F: the latent frames of the clip -> None when F <= Fw (one pass, the loop without windows), else a WindowPlan: the windows
        start at k (Fw - O) while they end in front of the last frame, and a last window ends with the clip."""
        F = _index(F, 'F')
        if F < 1:
            raise ValueError(f'F must be positive, got {F}')
        Fw, step = self.Fw, self.Fw - self.O
        if F <= Fw:
            return None
        starts = list(range(0, F - Fw, step)) + [F - Fw]          # k step + Fw < F, then the end-aligned window
        return WindowPlan(F, Fw, starts, self.raw_weights())

    def __repr__(self):
        return f'ContextWindows(frames={self.frames}, overlap={self.overlap}, fuse={self.fuse!r}, stride={self.stride})'
