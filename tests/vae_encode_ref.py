"""CPU restatement of the WanVAE *encode* path (test infrastructure, NOT product code; the product never imports it).

Restates, on a flat {state_dict-name: tensor} dict and on top of oracle/vae.py's CausalConv3d / RMS_norm /
ResidualBlock / AttentionBlock / feat-cache functions (pinned by the golden vectors of the imported reference):

  Encoder3d.__init__        key names and shapes                                   -> vae_encoder_shapes()
  Resample downsample2d/3d  ZeroPad2d((0,1,0,1)) + Conv2d(stride 2); time_conv     -> down()
  Encoder3d.forward         conv1, downsamples, middle, head on one chunk          -> encoder_chunk()
  WanVAE_.encode            chunks [1, 4, 4, ...], conv1, mu                       -> vae_encode()
  WanVAE.encode             (mu - mean) * (1 / std)                                   (folded into vae_encode)

Everything runs in the dtype of the parameters, so the same code gives the fp32 reference and its fp64 evaluation.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.vae import VAE_MEAN, VAE_STD, _cached_conv, attention_block, causal_conv3d, residual_block, rms_norm


def vae_encoder_shapes(dim=96, z_dim=16, dim_mult=(1, 2, 4, 4), num_res_blocks=2, temporal_downsample=(False, True, True)):
    """Shapes of conv1.* and encoder.* following Encoder3d.__init__ (built with z_dim * 2 output channels)."""
    sh = {'conv1.weight': (2 * z_dim, 2 * z_dim, 1, 1, 1), 'conv1.bias': (2 * z_dim,)}
    dims = [dim * u for u in [1] + list(dim_mult)]

    def res(pre, cin, cout):
        sh[pre + 'residual.0.gamma'] = (cin, 1, 1, 1)
        sh[pre + 'residual.2.weight'] = (cout, cin, 3, 3, 3)
        sh[pre + 'residual.2.bias'] = (cout,)
        sh[pre + 'residual.3.gamma'] = (cout, 1, 1, 1)
        sh[pre + 'residual.6.weight'] = (cout, cout, 3, 3, 3)
        sh[pre + 'residual.6.bias'] = (cout,)
        if cin != cout:
            sh[pre + 'shortcut.weight'] = (cout, cin, 1, 1, 1)
            sh[pre + 'shortcut.bias'] = (cout,)

    sh['encoder.conv1.weight'] = (dims[0], 3, 3, 3, 3)
    sh['encoder.conv1.bias'] = (dims[0],)
    idx = 0
    for i, (cin, cout) in enumerate(zip(dims[:-1], dims[1:])):
        for _ in range(num_res_blocks):
            res(f'encoder.downsamples.{idx}.', cin, cout)
            idx += 1
            cin = cout
        if i != len(dim_mult) - 1:
            pre = f'encoder.downsamples.{idx}.'
            sh[pre + 'resample.1.weight'] = (cout, cout, 3, 3)
            sh[pre + 'resample.1.bias'] = (cout,)
            if temporal_downsample[i]:
                sh[pre + 'time_conv.weight'] = (cout, cout, 3, 1, 1)
                sh[pre + 'time_conv.bias'] = (cout,)
            idx += 1
    d = dims[-1]
    res('encoder.middle.0.', d, d)
    sh['encoder.middle.1.norm.gamma'] = (d, 1, 1)
    sh['encoder.middle.1.to_qkv.weight'] = (3 * d, d, 1, 1)
    sh['encoder.middle.1.to_qkv.bias'] = (3 * d,)
    sh['encoder.middle.1.proj.weight'] = (d, d, 1, 1)
    sh['encoder.middle.1.proj.bias'] = (d,)
    res('encoder.middle.2.', d, d)
    sh['encoder.head.0.gamma'] = (d, 1, 1, 1)
    sh['encoder.head.2.weight'] = (2 * z_dim, d, 3, 3, 3)
    sh['encoder.head.2.bias'] = (2 * z_dim,)
    return sh


def make_vae_encoder_params(dim=8, seed=2, z_dim=16):
    """seeded encoder parameters, same distributions as weights.make_vae_params."""
    rs = np.random.RandomState(seed)
    P = {}
    for name, shape in vae_encoder_shapes(dim, z_dim).items():
        if name.endswith('gamma'):
            a = 1.0 + 0.1 * rs.standard_normal(shape)
        elif name.endswith('bias'):
            a = 0.05 * rs.standard_normal(shape)
        else:
            a = rs.standard_normal(shape) * (1.0 / np.sqrt(int(np.prod(shape[1:]))))
        P[name] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return P


def down(P, pre, x, cache, idx):
    """Resample in a down-sampling mode on x [1,C,T,H,W]; a downsample3d owns one cache slot, a downsample2d none."""
    b, c, t, h, w = x.shape
    y = x.permute(0, 2, 1, 3, 4).reshape(b * t, c, h, w)
    y = F.conv2d(F.pad(y, (0, 1, 0, 1)), P[pre + 'resample.1.weight'], P[pre + 'resample.1.bias'], stride=2)
    y = y.reshape(b, t, *y.shape[1:]).permute(0, 2, 1, 3, 4)
    if (pre + 'time_conv.weight') in P:
        i = idx[0]
        if cache[i] is None:                     # first chunk: pass through, remember it
            cache[i] = y.clone()
        else:
            keep = y[:, :, -1:].clone()
            y = F.conv3d(torch.cat([cache[i][:, :, -1:], y], dim=2), P[pre + 'time_conv.weight'], P[pre + 'time_conv.bias'], stride=(2, 1, 1))
            cache[i] = keep
        idx[0] += 1
    return y


def encoder_layout(P):
    n = 1 + max(int(k.split('.')[2]) for k in P if k.startswith('encoder.downsamples.'))
    return [('down' if (f'encoder.downsamples.{i}.resample.1.weight') in P else 'res', f'encoder.downsamples.{i}.') for i in range(n)]


def encoder_chunk(P, x, cache):
    """Encoder3d.forward on one chunk x [1,3,t,H,W]."""
    idx = [0]
    x = _cached_conv(P, 'encoder.conv1', x, cache, idx)
    for kind, pre in encoder_layout(P):
        x = residual_block(P, pre, x, cache, idx) if kind == 'res' else down(P, pre, x, cache, idx)
    x = residual_block(P, 'encoder.middle.0.', x, cache, idx)
    x = attention_block(P, 'encoder.middle.1.', x)
    x = residual_block(P, 'encoder.middle.2.', x, cache, idx)
    x = F.silu(rms_norm(x, P['encoder.head.0.gamma']))
    return _cached_conv(P, 'encoder.head.2', x, cache, idx)


def vae_encode(P, video):
    """WanVAE.encode for one video [3,T,H,W] -> normalised mu [z_dim, 1+(T-1)//4, H//8, W//8], in the dtype of P."""
    dt = P['conv1.weight'].dtype
    x = video[None].to(dt)
    T = x.shape[2]
    cache = [None] * sum(1 for k, v in P.items() if k.startswith('encoder.') and k.endswith('.weight') and v.dim() == 5)
    outs = []
    for i in range(1 + (T - 1) // 4):
        outs.append(encoder_chunk(P, x[:, :, :1] if i == 0 else x[:, :, 1 + 4 * (i - 1):1 + 4 * i], cache))
    out = causal_conv3d(torch.cat(outs, dim=2), P['conv1.weight'], P['conv1.bias'])
    zc = out.shape[1] // 2
    mean = torch.tensor(VAE_MEAN[:zc], dtype=dt).view(1, zc, 1, 1, 1)
    inv_std = (1.0 / torch.tensor(VAE_STD[:zc], dtype=dt)).view(1, zc, 1, 1, 1)
    return ((out[:, :zc] - mean) * inv_std)[0]
