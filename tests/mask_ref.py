"""fp64 restatement of mg_mask_from_u8 and a plain-loop restatement of mg_mask_to_latent_u8 (include/moviigen_hip.h), built on
tests/resize_ref.py.  The references of tests/test_inpaint.py."""
import torch

from resize_ref import cover_geometry, resize_f64

THRESHOLD = 127.5


def mask_r_f64(mask, T, H, W):
    """uint8 [Tm, H0, W0] (Tm == 1 or >= T) -> r [T, H, W] fp64: the mask's bytes through the resize to cover and the centre crop of the frames."""
    Tm, H0, W0 = mask.shape
    assert Tm == 1 or Tm >= T
    Hs, Ws, oy, ox = cover_geometry(H0, W0, H, W)
    r = resize_f64(mask[:T], Hs, Ws)[..., oy:oy + H, ox:ox + W]
    return r.expand(T, H, W) if Tm == 1 else r


def mask_from_u8_ref(mask, T, H, W, keep_frames=0):
    """-> (pm uint8 [T, H, W], r fp64 [T, H, W]): pm = 0 on frames < keep_frames, else r >= 127.5."""
    r = mask_r_f64(mask, T, H, W)
    pm = (r >= THRESHOLD).to(torch.uint8)
    pm[:keep_frames] = 0
    return pm, r


def latent_footprint(j, y, x, st, sh, sw):
    """(frames, rows, columns) of the pixels under latent cell (j, y, x) of a causal VAE: latent frame 0 is pixel frame 0 alone."""
    frames = range(0, 1) if j == 0 else range(st * (j - 1) + 1, st * j + 1)
    return frames, range(sh * y, sh * y + sh), range(sw * x, sw * x + sw)


def mask_to_latent_ref(pm, st, sh, sw):
    """uint8 [T, H, W] -> uint8 [(T-1)/st + 1, H/sh, W/sw]: 1 where any pixel under the cell is non-zero."""
    T, H, W = pm.shape
    assert (T - 1) % st == 0 and H % sh == 0 and W % sw == 0
    nz = pm != 0
    lm = torch.zeros((T - 1) // st + 1, H // sh, W // sw, dtype=torch.uint8)
    for j in range(lm.shape[0]):
        fr = latent_footprint(j, 0, 0, st, sh, sw)[0]
        plane = nz[fr.start:fr.stop].any(0)                                      # [H, W]
        lm[j] = plane.reshape(H // sh, sh, W // sw, sw).any(3).any(1).to(torch.uint8)
    return lm
