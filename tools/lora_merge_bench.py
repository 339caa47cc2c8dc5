"""WanModel.load_lora at the 14B configuration, and mg_lora_merge alone on the model's matrices: one JSON line per figure.
    python tools/lora_merge_bench.py [layers]          (layers: 40 = the whole model; fewer for a rehearsal)

load_lora: synthetic weights (init_weights), an adapter on the ten linears of every block (q, k, v, o of both attentions, ffn.0,
ffn.2) at rank 16 and rank 128, handed over as a dict of tensors — no file read in the timed window — on the host (what a file read
leaves: the time includes the copy of the factors to the device) and already on the device.  The window ends in a device synchronise.

kernel: device events around mg_lora_merge over a ring of distinct matrices larger than the 256 MB last-level cache, so every launch
reads and writes its w in HBM; bytes of w moved (one read + one write) per second, next to the 6.29 TB/s a copy reaches on this part
(the row-wise kernels are held to it), and the fp32 MFMA rate of the update itself."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'moviigen1.1_amd')):
    sys.path.insert(0, p)
import torch  # noqa: E402
import wan  # noqa: E402
from wan.backend import ops  # noqa: E402

MODEL_14B = dict(dim=5120, ffn_dim=13824, freq_dim=256, num_heads=40, num_layers=40, text_len=512, text_dim=4096,
                 in_dim=16, out_dim=16, eps=1e-6)
COPY_TBS = 6.29
dev = torch.device('cuda:0')
gen = torch.Generator(device=dev).manual_seed(0)


def kernel_rows():
    for N, K in ((5120, 5120), (13824, 5120), (5120, 13824)):
        ring = max(2, int(1.0e9 // (N * K * 2)) + 1)           # > 1 GB of distinct weights
        ws = [(torch.randn(N, K, device=dev, generator=gen) * 0.02).bfloat16() for _ in range(ring)]
        for R in (16, 32, 64, 128):
            up = torch.randn(N, R, device=dev, generator=gen) * 1e-3
            down = torch.randn(R, K, device=dev, generator=gen) * 1e-3
            for w in ws:
                ops.lora_merge(w, up, down)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            rounds = 4
            a.record()
            for _ in range(rounds):
                for w in ws:
                    ops.lora_merge(w, up, down)
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) / (rounds * ring) * 1e3
            nbytes = 2 * N * K * 2
            print(json.dumps({'kernel': 'mg_lora_merge bf16', 'N': N, 'K': K, 'R': R, 'us': round(us, 1), 'w_TB_per_s': round(nbytes / us / 1e6, 3),
                              'frac_of_copy_6.29': round(nbytes / us / 1e6 / COPY_TBS, 3), 'mfma_f32_TFLOPs': round(2.0 * N * K * R / us / 1e6, 1)}),
                  flush=True)
        del ws


def model_rows(layers):
    cfg = dict(MODEL_14B, num_layers=layers)
    m = wan.modules.WanModel(**cfg, device=dev)
    m.init_weights(seed=0)
    targets = [n for n in m.lora_targets() if n.startswith('blocks.')]
    assert len(targets) == 10 * layers
    shapes = {n: tuple(w.shape) for n, w in m.lora_targets().items()}
    for R in (16, 128):
        # one random factor pair per distinct shape, shared by the blocks: the values do not matter to the time, the host memory does
        pool = {}
        adapter = {}
        for n in targets:
            if shapes[n] not in pool:
                pool[shapes[n]] = (torch.randn(shapes[n][0], R) * 0.01, torch.randn(R, shapes[n][1]) * 0.01)
            adapter[n + '.lora_up.weight'], adapter[n + '.lora_down.weight'] = pool[shapes[n]]
        on_dev = {k: v.to(dev) for k, v in adapter.items()}
        wbytes = sum(m.lora_targets()[n].numel() * 2 for n in targets)
        for where, ad in (('host', adapter), ('device', on_dev), ('host', adapter), ('device', on_dev)):      # each twice: the first pair warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.load_lora(ad, 1.0)                # keep_base=True: includes the clone of the touched weights
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            m.unload_lora()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print(json.dumps({'load_lora': f'14B x {layers} blocks, {len(targets)} linears', 'rank': R, 'factors_on': where,
                              'load_seconds': round(t1 - t0, 3), 'unload_seconds': round(t2 - t1, 3), 'weights_GB': round(wbytes / 1e9, 2)}),
                  flush=True)


if __name__ == '__main__':
    kernel_rows()
    model_rows(int(sys.argv[1]) if len(sys.argv) > 1 else 40)
