"""fp64 restatement of mg_video_from_u8 (include/moviigen_hip.h): resize to cover with the antialiased triangle filter, centre crop,
v / 127.5 - 1.  The reference of tests/test_v2v.py; itself checked there against F.interpolate(mode='bilinear', antialias=True)."""
import math

import torch


def axis_weights(n_in, n_out):
    """[n_out, n_in] fp64: row i holds the normalised weights of output sample i (half-pixel centres, support max(in/out, 1))."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    inv = 1.0 / support
    w = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        for j in range(lo, hi):
            w[i, j] = max(0.0, 1.0 - abs((j - c + 0.5) * inv))
        w[i] /= w[i].sum()
    return w


def resize_f64(x, Hs, Ws):
    """x [..., H0, W0] -> [..., Hs, Ws] fp64."""
    wy, wx = axis_weights(x.shape[-2], Hs), axis_weights(x.shape[-1], Ws)
    return torch.einsum('yj,...jk,xk->...yx', wy, x.double(), wx)


def cover_geometry(H0, W0, H, W):
    """(Hs, Ws, oy, ox): the resized extent that covers H x W and the crop origin in it."""
    s = max(H / H0, W / W0)
    Hs, Ws = max(H, math.floor(H0 * s + 0.5)), max(W, math.floor(W0 * s + 0.5))
    return Hs, Ws, (Hs - H) // 2, (Ws - W) // 2


def video_from_u8_f64(frames, H, W):
    """uint8 [T, H0, W0, 3] -> [3, T, H, W] fp64 in [-1, 1]."""
    T, H0, W0, _ = frames.shape
    Hs, Ws, oy, ox = cover_geometry(H0, W0, H, W)
    r = resize_f64(frames.permute(3, 0, 1, 2), Hs, Ws)[..., oy:oy + H, ox:ox + W]
    return r / 127.5 - 1.0
