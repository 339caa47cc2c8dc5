"""FLOP count (2 x multiply-adds, as the reference's convolutions define them: no padding or tile waste) of WanVAE.encode."""


def vae_encode_stage_flops(T, H, W, dim=96, z_dim=16):
    """{stage: FLOPs} of the encode of a [3,T,H,W] clip (dim_mult 1,2,4,4; two residual blocks per level; temporal stride at levels 1, 2).
    Stages are named by their state-dict prefix."""
    n = 1 + (T - 1) // 4                      # chunks = latent frames
    f0 = 1 + 4 * (n - 1)                      # frames read; levels 0, 1
    f2, f3 = 1 + 2 * (n - 1), n               # frames at level 2 / level 3
    d = [dim, dim, 2 * dim, 4 * dim, 4 * dim]
    px = [H * W, (H // 2) * (W // 2), (H // 4) * (W // 4), (H // 8) * (W // 8)]
    frames = [f0, f0, f2, f3]
    out = {'encoder.conv1': 81 * d[0] * f0 * px[0]}

    def res(cin, cout):
        return 27 * cin * cout + 27 * cout * cout + (cin * cout if cin != cout else 0)
    idx = 0
    for lvl in range(4):
        cin, cout = d[lvl], d[lvl + 1]
        for _ in range(2):
            out[f'encoder.downsamples.{idx}.'] = res(cin, cout) * frames[lvl] * px[lvl]
            idx += 1
            cin = cout
        if lvl < 3:
            macs = 9 * cout * cout * frames[lvl] * px[lvl + 1]                              # 3x3 stride 2: per OUTPUT pixel, every frame of the level
            if lvl >= 1:
                macs += 3 * cout * cout * (frames[lvl + 1] - 1) * px[lvl + 1]               # time_conv: every output frame but the passed-through first
            out[f'encoder.downsamples.{idx}.'] = macs
            idx += 1
    c, L = d[4], px[3]
    out['encoder.middle.0.'] = res(c, c) * f3 * L
    out['encoder.middle.1.'] = (4 * c * c + 2 * L * c) * f3 * L                             # to_qkv, proj, q.k^T, p.v
    out['encoder.middle.2.'] = res(c, c) * f3 * L
    out['encoder.head'] = 27 * c * 2 * z_dim * f3 * L
    out['conv1'] = 4 * z_dim * z_dim * f3 * L
    return {k: 2 * v for k, v in out.items()}


def vae_encode_flops(T, H, W, dim=96, z_dim=16):
    return sum(vae_encode_stage_flops(T, H, W, dim, z_dim).values())
