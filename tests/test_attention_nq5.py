"""Five query blocks per wave (320-query items) of the head-dim-128 attention kernel against the four-block kernel.

A row's arithmetic does not depend on the item size: its reference comes from its first key tile, its partial row sums live in
the same four lanes and its keys arrive in the same order.  So every comparison here is torch.equal — output and log-sum-exp —
between the A/B library's forced five-block launch (mg_attn_w64_debug bit 7) and the default launch of the same library, which at
these sizes is the four-block kernel.  The launcher's rule itself is a host function and is checked without a GPU."""
import math

import pytest
import torch

import weights as W

SC = 1.0 / math.sqrt(128)
LOG2E = 1.4426950408889634
FORCE_NQ5 = 128         # mg_attn_w64_debug: bit 7


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def scale_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _operands(Lq, Lk, heads, dev, seed, on_gpu=False):
    """q already carries scale * log2(e) (the pre-scaled entry's contract), rounded to bf16 once."""
    if on_gpu:
        g = torch.Generator(device=dev).manual_seed(seed)
        q = (torch.randn(Lq, heads * 128, device=dev, generator=g) * (1.5 * SC * LOG2E)).bfloat16()
        k = (torch.randn(Lk, heads * 128, device=dev, generator=g) * 1.5).bfloat16()
        v = torch.randn(Lk, heads * 128, device=dev, generator=g).bfloat16()
        return q, k, v
    q = (W.randn((Lq, heads * 128), seed) * (1.5 * SC * LOG2E)).bfloat16()
    k = (W.randn((Lk, heads * 128), seed + 1) * 1.5).bfloat16()
    v = W.randn((Lk, heads * 128), seed + 2).bfloat16()
    return q.to(dev), k.to(dev), v.to(dev)


def _attend(h, q, k, v, heads, debug, workspace='stream', reserve_cus=0, cnt=None):
    """one pre-scaled launch of the A/B library (call inside lib.ab_library()) -> (out, lse)"""
    from wan.backend import ops
    Lq, Lk = q.shape[0], k.shape[0]
    n = ops.packed_kv_numel(Lk, heads)
    kp, vp = torch.empty(n, dtype=torch.bfloat16, device=q.device), torch.empty(n, dtype=torch.bfloat16, device=q.device)
    ops.pack_kv(k, v, heads, kp, vp)
    out = torch.full_like(q, float('nan'))
    lse = torch.full((heads, Lq), float('nan'), dtype=torch.float32, device=q.device)
    h.mg_attn_w64_debug(debug)
    if cnt is not None:
        h.mg_attn_w64_flag_counter(cnt.data_ptr())
    ops.attention_hd128(q, kp, vp, out, Lk, heads, SC, prescaled=True, reserve_cus=reserve_cus, workspace=workspace, lse=lse)
    torch.cuda.synchronize()
    h.mg_attn_w64_debug(0)
    h.mg_attn_w64_flag_counter(None)
    return out, lse


def _oracle(q, k, v, heads):
    """oracle attention of the operands the kernel is GIVEN: q / (scale log2 e) in fp32 (no second rounding), so its scores are the kernel's"""
    from oracle import dit
    Lq, Lk = q.shape[0], k.shape[0]
    qe = (q.float().cpu() / (SC * LOG2E)).view(Lq, heads, 128)
    return dit.attention(qe, k.float().cpu().view(Lk, heads, 128), v.float().cpu().view(Lk, heads, 128), Lk, False).reshape(Lq, heads * 128)


# ------------------------------------------------------------------------------------------------
# CPU: the launcher's rule
# ------------------------------------------------------------------------------------------------
def test_item_rule_keeps_four_blocks_for_small_launches():
    """mg_attn_hd128_item_queries is a pure host function: every shape the suite launches keeps 256-query items — Lq <= 20 000 with few
    heads, the 512-key cross-attention, the 8192 x 260-head ticket test, the general (not pre-scaled) entry at any size."""
    from wan.backend import lib
    f = lib.load().mg_attn_hd128_item_queries
    for n_cu in (256, 248, 8):
        for Lq, Lk, heads in [(300, 300, 2), (700, 512, 3), (1, 1, 1), (20000, 20000, 4), (20000, 20000, 12), (131040, 512, 40), (32760, 512, 40),
                              (8192, 8192, 260), (2000, 640, 40), (7000, 704, 384), (320, 192, 1)]:
            assert f(Lq, Lk, heads, 1, n_cu) == 256, (Lq, Lk, heads, n_cu)
            assert f(Lq, Lk, heads, 0, n_cu) == 256, (Lq, Lk, heads, n_cu)
        assert f(131040, 131040, 40, 0, n_cu) == 256          # the general entry never
    assert f(131040, 131040, 40, 1, 0) == 256 and f(131040, 131040, 0, 1, 256) == 256      # degenerate arguments: the safe answer
    assert f(131040, 131040, 40, 1, 256) in (256, 320)


# ------------------------------------------------------------------------------------------------
# GPU: same bits as the four-block kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('Lq,Lk,heads', [(320, 192, 1), (407, 677, 3), (79, 256, 2)], ids=['one_item_3_tiles', 'ragged', 'under_one_block'])
def test_nq5_same_bits_small(dev, Lq, Lk, heads):
    from wan.backend import lib
    q, k, v = _operands(Lq, Lk, heads, dev, 40)
    with lib.ab_library() as h:
        o4, l4 = _attend(h, q, k, v, heads, 0)
        o5, l5 = _attend(h, q, k, v, heads, FORCE_NQ5)
    assert not torch.isnan(o5.float()).any() and not torch.isnan(l5).any()
    assert torch.equal(o4, o5) and torch.equal(l4, l5)
    if Lq == 407:
        assert scale_err(o5.float(), _oracle(q, k, v, heads)) < 2e-2


@pytest.mark.gpu
def test_nq5_same_bits_multi_round(dev):
    """280 items of 320 queries on 256 CUs: the persistent work loop — with a workspace, without one (the static partition), and on a
    reduced grid."""
    from wan.backend import lib
    Lq, Lk, heads = 2000, 640, 40
    q, k, v = _operands(Lq, Lk, heads, dev, 50, on_gpu=True)
    with lib.ab_library() as h:
        o4, l4 = _attend(h, q, k, v, heads, 0)
        for kw in (dict(), dict(workspace=None), dict(reserve_cus=8), dict(workspace=None, reserve_cus=16)):
            o5, l5 = _attend(h, q, k, v, heads, FORCE_NQ5, **kw)
            assert torch.equal(o4, o5) and torch.equal(l4, l5), kw


@pytest.mark.gpu
def test_nq5_tickets_rearm(dev):
    """22 x 384 = 8448 items of 320 queries = 33 rounds: items by ticket.  With a workspace, twice in a row (the counters re-arm), it
    matches the launch without one and the four-block kernel."""
    from wan.backend import lib
    Lq, Lk, heads = 7000, 704, 384
    q, k, v = _operands(Lq, Lk, heads, dev, 60, on_gpu=True)
    ws = torch.zeros(int(lib.load().mg_attn_workspace_bytes()), dtype=torch.uint8, device=dev)
    with lib.ab_library() as h:
        o_static, l_static = _attend(h, q, k, v, heads, FORCE_NQ5, workspace=None)
        for _ in range(2):
            o5, l5 = _attend(h, q, k, v, heads, FORCE_NQ5, workspace=ws)
            assert torch.equal(o_static, o5) and torch.equal(l_static, l5)
            assert int(ws.view(torch.int32)[:2].abs().sum().item()) == 0       # left zeroed for the next launch
        o4, l4 = _attend(h, q, k, v, heads, 0, workspace=ws)
    assert torch.equal(o4, o_static) and torch.equal(l4, l_static)


@pytest.mark.gpu
@pytest.mark.parametrize('bits', [100, 200], ids=['2^100_pipelined', '2^200_swept'])
def test_nq5_rescale_branch(dev, bits):
    """a key whose exponent stands `bits` above the best of its row's first tile: 2^100 stays inside the pipelined pass's range
    (reference = first-tile maximum + 64 bits, row sums up to 2^90), 2^200 flags the item, which the five-block instantiation
    repeats itself with swept row maxima (the rare paths are instantiated for five blocks too) — never the exact loop.  Both match the
    four-block kernel's bits and the oracle."""
    from wan.backend import lib
    Lq, Lk, heads = 320, 640, 1
    q = (W.randn((Lq, 128), 14) * (SC * LOG2E)).bfloat16()
    k = (W.randn((Lk, 128), 15) * 0.2).bfloat16()
    v = W.randn((Lk, 128), 16).bfloat16()
    rows = {300: 300, 7: 500}                                   # query row (fifth block of wave 3; first block of wave 0) -> its spiked key
    for r, key in rows.items():
        first = (q[r].float() @ k[:64].float().T).max().item()
        unit = (q[r].float() @ (q[r].float() / (SC * LOG2E)).bfloat16().float()).item()      # exponent per unit of the factor
        k[key] = (q[r].float() / (SC * LOG2E) * ((bits + first) / unit)).bfloat16()
    ex = q.float() @ k.float().T
    above = [(ex[r].max() - ex[r, :64].max()).item() for r in rows]
    assert all(abs(a - bits) < 4 for a in above), above
    q, k, v = q.to(dev), k.to(dev), v.to(dev)
    cnt4 = torch.zeros(2, dtype=torch.int32, device=dev)
    cnt5 = torch.zeros(2, dtype=torch.int32, device=dev)
    with lib.ab_library() as h:
        o4, l4 = _attend(h, q, k, v, heads, 0, cnt=cnt4)
        o5, l5 = _attend(h, q, k, v, heads, FORCE_NQ5, cnt=cnt5)
    assert torch.equal(o4, o5) and torch.equal(l4, l5)
    assert scale_err(o5.float(), _oracle(q, k, v, heads)) < 2e-2
    for r, key in rows.items():                                 # one-hot rows: the output is the spiked key's value row
        assert (o5[r].float() - v[key].float()).abs().max().item() < 2e-2
    assert (cnt5[0].item() > 0) == (bits > 154), (above, cnt5.tolist())
    assert (cnt4[0].item() > 0) == (bits > 154), (above, cnt4.tolist())
    assert cnt5[1].item() == 0 and cnt4[1].item() == 0          # finite scores never reach the exact loop
