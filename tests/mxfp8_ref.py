"""The project's definition of OCP MXFP8 (E4M3) in torch, on the CPU: the reference of mg_quant_mxfp8_rows / mg_gemm_mxfp8.

Along the last dimension every 32 consecutive elements share one E8M0 scale byte s, meaning 2^(s-127); elements are OCP
e4m3fn.  A block with maximum magnitude amax takes e = floor(log2(amax)) - 8 clamped to [-127, 127] (a block of zeros:
-127), scale byte e + 127; an element is x * 2^-e, clamped to +-448 BEFORE the round-to-nearest-even conversion, so it
saturates (500 -> 448) where torch's own cast returns NaN.  Inputs must be finite: NaN / infinity are outside the definition."""
import torch


def quant(x):
    """x [..., K] (K % 32 == 0, any float dtype) -> (q uint8 [..., K] e4m3fn bit patterns, scales uint8 [..., K/32])"""
    xf = x.detach().float().cpu()
    blocks = xf.reshape(*xf.shape[:-1], xf.shape[-1] // 32, 32)
    amax = blocks.abs().amax(-1)
    _, ex = torch.frexp(amax)                                      # amax = m 2^ex, m in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.where(amax > 0, ex - 1 - 8, torch.full_like(ex, -127)).clamp(-127, 127)
    inv = ((127 - e).to(torch.int32) << 23).view(torch.float32)    # 2^-e exactly (e <= 119 for any finite fp32 amax)
    y = (blocks * inv.unsqueeze(-1)).clamp(-448.0, 448.0)
    q = y.to(torch.float8_e4m3fn).view(torch.uint8).reshape(xf.shape)
    return q, (e + 127).to(torch.uint8)


def dequant(q, scales):
    """(q uint8 [..., K], scales uint8 [..., K/32]) -> fp32 [..., K]: e4m3 * 2^(s-127), exact"""
    v = q.cpu().view(torch.float8_e4m3fn).double()
    two_e = ((scales.cpu().to(torch.int64) - 127 + 1023) << 52).view(torch.float64)
    blocks = v.reshape(*v.shape[:-1], v.shape[-1] // 32, 32) * two_e.unsqueeze(-1)
    return blocks.reshape(v.shape).float()
