"""Time WanVAE decode (BASELINE.json configs[4]: 1920x832x81f latent -> pixels) on one MI355X.
    python tools/bench_vae.py [--size 1920x832] [--frames 81] [--chunk N]
Synthetic weights of the shipped decoder shape (dim 96), z = randn seed 7.
    python tools/bench_vae.py --chunk 4 --encode [--stages]
also times WanVAE.encode of a [3,81,832,1920] and a [3,81,720,1280] clip (median of --encode-reps calls, events around the whole
call) behind the decode leg of the same run: seconds, executed TFLOP/s against the same fp32-MFMA peak, peak memory; with --stages
the milliseconds and TFLOP/s of every encoder stage; --mode bf16x3 times the encode of a bf16x3 object; the frame ingest (mg_video_from_u8,
1080p -> 1920x832x81) is timed behind it.
    python tools/bench_vae.py --mask
times only the four passes of WanT2V.inpaint at 1920x832x81 (median of 5 calls each): milliseconds and GB/s."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'moviigen1.1_amd'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)
import torch  # noqa: E402
import weights as W  # noqa: E402
import wan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--size', default='1920x832')
ap.add_argument('--frames', type=int, default=81)
ap.add_argument('--chunk', type=int, default=1, help='latent frames per decoder chunk after the first')
ap.add_argument('--mode', default='exact', choices=('exact', 'bf16x3'), help='bf16x3: the opt-in split-bf16 convolutions (not the reference arithmetic)')
ap.add_argument('--tile', default='auto', help="voxels per workgroup of the wide exact convolutions: auto (by shape), 128, 256")
ap.add_argument('--stages', action='store_true', help='also time every decoder stage (first chunk / steady chunk) and model the layer pipeline of decode_pipelined for 2 / 4 / 8 ranks')
ap.add_argument('--bands', type=int, nargs='*', default=[], metavar='P',
                help='EMULATION on this one GPU of ONE rank of the W-band decode over P ranks (WanVAE.decode_spatial on a loop-back process group: the real '
                     "band width, halo columns, gather copies and kernel launches of an interior rank; the neighbours' data is its own): measured seconds of the "
                     'rank + the bytes it would put on a link, priced at --link-gbps.  Lines are marked `invalid: emulation`')
ap.add_argument('--link-gbps', type=float, default=45.0)
ap.add_argument('--upconv', default='phases', choices=('phases', 'gather'), help="the convs behind a 2x upsample: four 2x2 phase convs / one 3x3 through the upsample")
ap.add_argument('--encode', action='store_true', help='after the decode leg: time WanVAE.encode at 1920x832x81 and 1280x720x81 (random dim-96 encoder weights)')
ap.add_argument('--encode-reps', type=int, default=3)
ap.add_argument('--mask', action='store_true', help="only time the four passes of WanT2V.inpaint at 1920x832x81 (no decode, no encode): the mask's resize from "
                                                   '1920x1080, its reduction to the latent grid, the per-step overwrite of the kept latent cells and the final composite')
args = ap.parse_args()
Wd, Hd = (int(v) for v in args.size.split('x'))
T = (args.frames - 1) // 4 + 1
dev = torch.device('cuda:0')


def median_ms(fn, reps=5):
    """median of `reps` timed calls behind one warm-up call, HIP events around each call"""
    fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2], ms


if args.mask:
    # masked video-to-video (WanT2V.inpaint): a rectangle mask (the inside regenerated, the kept and the regenerated halves about equal), so the
    # overwrite and the composite touch about half of their elements.  Bytes = what a pass must move at least: every mask byte once, and for the
    # two masked overwrites only the elements of the kept half (sources read, destination written); a 16-byte group that straddles the mask's
    # edge also reads its destination, which is not counted.  The rate to compare with: 4.9-5.0 TB/s of the streaming kernels.
    from wan.backend import ops
    g = torch.Generator(device=dev).manual_seed(3)
    mask = torch.zeros(1, 1080, 1920, dtype=torch.uint8, device=dev)
    mask[:, 270:810, 480:1440] = 255
    pm = torch.empty(81, 832, 1920, dtype=torch.uint8, device=dev)
    lm = ops.mask_to_latent(ops.mask_from_u8(mask, 81, 832, 1920, out=pm), (4, 8, 8))
    latent, z0, noise = (torch.randn(16, 21, 104, 240, device=dev, generator=g) for _ in range(3))
    video, clip = (torch.rand(3, 81, 832, 1920, device=dev, generator=g) for _ in range(2))
    kept_lat, kept_px = float((lm == 0).float().mean()), float((pm == 0).float().mean())
    rows = 832                          # cover = the same width: 832 of the 1080 mask rows survive the crop
    passes = [
        ('mask_from_u8', '1x1080x1920 uint8 -> 81x832x1920 uint8', lambda: ops.mask_from_u8(mask, 81, 832, 1920, out=pm), rows * 1920 + pm.numel()),
        ('mask_to_latent', '81x832x1920 uint8 -> 21x104x240 uint8', lambda: ops.mask_to_latent(pm, (4, 8, 8)), pm.numel() + lm.numel()),
        ('masked_renoise', '[16,21,104,240] fp32, per step', lambda: ops.masked_renoise(latent, z0, noise, lm, 0.3753, 0.6247),
         lm.numel() + int(kept_lat * latent.numel()) * 12),
        ('mask_composite', '[3,81,832,1920] fp32, once per call', lambda: ops.mask_composite(video, clip, pm), pm.numel() + int(kept_px * video.numel()) * 8),
    ]
    for name, what, fn, nbytes in passes:
        med, ms = median_ms(fn)
        print(json.dumps({'metric': name + '_ms', 'value': med, 'all_ms': ms, 'what': what, 'bytes_min': nbytes, 'gb_per_s': nbytes / med / 1e6,
                          'kept_fraction_latent': kept_lat, 'kept_fraction_pixels': kept_px}))
    # the same two overwrites with everything kept: every element is read from its sources and written, the plain streaming case
    pm.zero_()
    lm.zero_()
    for name, fn, nbytes in (('masked_renoise_all_kept', lambda: ops.masked_renoise(latent, z0, noise, lm, 0.3753, 0.6247), lm.numel() + latent.numel() * 12),
                             ('mask_composite_all_kept', lambda: ops.mask_composite(video, clip, pm), pm.numel() + video.numel() * 8)):
        med, ms = median_ms(fn)
        print(json.dumps({'metric': name + '_ms', 'value': med, 'all_ms': ms, 'bytes_min': nbytes, 'gb_per_s': nbytes / med / 1e6}))
    sys.exit(0)

params = W.make_vae_params(96, 1)
if args.encode:
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from vae_encode_ref import make_vae_encoder_params
    params.update(make_vae_encoder_params(96, 2))            # (the decode does not read them: tests/test_vae_encode.py)
vae = wan.modules.WanVAE(state_dict=params, device=dev, upconv=args.upconv, mode=args.mode,
                         tile=args.tile if args.tile == 'auto' else int(args.tile))
z = torch.randn(16, T, Hd // 8, Wd // 8, generator=torch.Generator().manual_seed(7)).to(dev)
chunks = [1] + [args.chunk] * ((T - 1) // args.chunk) + ([(T - 1) % args.chunk] if (T - 1) % args.chunk else [])
torch.cuda.synchronize()
t0 = time.perf_counter()
video = vae.model.decode(z, chunks=chunks)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
del video
t1 = time.perf_counter()
video = vae.model.decode(z, chunks=chunks)           # second decode: the caching allocator already holds every block
torch.cuda.synchronize()
dt_warm = time.perf_counter() - t1
# conv FLOPs of the decoder at this size (1116.5 TF at 1920x832x81, scales with voxels)
# (what the MFMAs EXECUTE: the phase-decomposed up-convs do 4/9 of their taps — 1065.8 instead of 1116.5 TF, bench.py vae_decode_flops)
flops = (1065.8e12 if args.upconv == 'phases' else 1116.5e12) * (Wd * Hd * args.frames) / (1920 * 832 * 81)
print(json.dumps({'metric': 'vae_decode_sec', 'value': dt, 'second_decode_sec': dt_warm, 'upconv': args.upconv, 'mode': args.mode, 'tile': args.tile, 'size': args.size, 'frames': args.frames, 'chunks': chunks[:3],
                  'tflops_fp32': flops / dt / 1e12, 'fp32_mfma_peak_tflops': 157.3, 'frac': flops / dt / 157.3e12,
                  'finite': bool(torch.isfinite(video).all().item()), 'peak_mem_gb': torch.cuda.max_memory_allocated() / 2**30}))

if args.encode:
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from vae_flops import vae_encode_flops, vae_encode_stage_flops
    decode_frac = flops / min(dt, dt_warm) / 157.3e12
    del video
    m = vae.model
    vae.encode([torch.rand(3, 5, 64, 64, device=dev)])        # warm-up: every kernel loaded
    for (eh, ew) in ((832, 1920), (720, 1280)):
        clip = torch.rand(3, 81, eh, ew, device=dev, generator=torch.Generator(device=dev).manual_seed(9)) * 2 - 1
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base_mem = torch.cuda.memory_allocated()
        secs = []
        for _ in range(max(3, args.encode_reps)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            lat = vae.encode([clip])[0]
            b.record()
            torch.cuda.synchronize()
            secs.append(a.elapsed_time(b) / 1e3)
        med = sorted(secs)[len(secs) // 2]
        ef = vae_encode_flops(81, eh, ew)
        print(json.dumps({'metric': 'vae_encode_sec', 'value': med, 'all_sec': secs, 'mode': args.mode, 'size': f'{ew}x{eh}', 'frames': 81, 'latent': list(lat.shape),
                          'pflop': ef / 1e15, 'tflops_fp32': ef / med / 1e12, 'fp32_mfma_peak_tflops': 157.3, 'frac': ef / med / 157.3e12,
                          'decode_frac_same_run': decode_frac, 'finite': bool(torch.isfinite(lat).all().item()),
                          'peak_mem_gb': torch.cuda.max_memory_allocated() / 2**30, 'of_which_clip_and_weights_gb': base_mem / 2**30}))
        if args.stages:
            acc, order = {}, []

            def wrap(fn, key_of):
                def timed(*a_, **k_):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    y = fn(*a_, **k_)
                    e1.record()
                    key = key_of(*a_, **k_)
                    if key not in acc:
                        order.append(key)
                    acc.setdefault(key, []).append((e0, e1))
                    return y
                return timed
            o_res, o_down, o_attn, o_chunk = m._res, m._down, m._attn, m._encoder_chunk
            m._res, m._down, m._attn = wrap(o_res, lambda pre, *r: pre), wrap(o_down, lambda pre, *r: pre), wrap(o_attn, lambda pre, *r: pre)
            m._encoder_chunk = wrap(o_chunk, lambda *r: 'chunk')
            vae.encode([clip])
            torch.cuda.synchronize()
            m._res, m._down, m._attn, m._encoder_chunk = o_res, o_down, o_attn, o_chunk
            ms = {k: sum(x.elapsed_time(y) for x, y in v) for k, v in acc.items()}
            sf = vae_encode_stage_flops(81, eh, ew)
            rest = ms.pop('chunk') - sum(ms.values())               # video_in + encoder.conv1 + head (norm, conv) of every chunk
            print(f'encode {ew}x{eh}x81 stage                 total_ms   TFLOP   TFLOP/s   frac_of_peak')
            for k in [k for k in order if k != 'chunk']:
                print(f'{k:40s} {ms[k]:9.1f} {sf[k] / 1e12:7.1f} {sf[k] / ms[k] / 1e9:9.1f} {sf[k] / ms[k] / 1e9 / 157.3:10.2f}')
            fr = sf['encoder.conv1'] + sf['encoder.head']
            print(f"{'video_in + encoder.conv1 + encoder.head':40s} {rest:9.1f} {fr / 1e12:7.1f} {fr / rest / 1e9:9.1f} {fr / rest / 1e9 / 157.3:10.2f}")
        del clip, lat

if args.encode:
    # the way in of a video-to-video start: 81 uint8 frames -> the [3,81,832,1920] fp32 clip (mg_video_from_u8).  1920x1080: cover = the same width,
    # 124 rows cropped top and bottom, every output has the weights {1, 0} per axis; 3840x2160: 2x down, 5 taps per axis, then the same crop.
    # Bytes: the input rows the crop keeps are read once from HBM, the clip is written once.
    from wan.backend import ops
    clip = torch.empty(3, 81, 832, 1920, device=dev)
    for (h0, w0) in ((1080, 1920), (2160, 3840)):
        frames = torch.randint(0, 256, (81, h0, w0, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
        ops.video_from_u8(frames, 832, 1920, out=clip)
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.video_from_u8(frames, 832, 1920, out=clip)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        med = sorted(ms)[len(ms) // 2]
        kept = 81 * (832 * h0 // 1080) * w0 * 3
        print(json.dumps({'metric': 'video_from_u8_ms', 'value': med, 'all_ms': ms, 'from': f'{w0}x{h0}x81 uint8', 'to': '1920x832x81 fp32',
                          'bytes_read_kept_rows': kept, 'bytes_written': clip.numel() * 4, 'gb_per_s': (kept + clip.numel() * 4) / med / 1e6,
                          'finite': bool(torch.isfinite(clip).all().item())}))
        del frames
    del clip

if args.bands:
    # one rank of P, emulated: what the W split costs a rank in kernels and copies (measured) and in link time (bytes / rate, not overlapped)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from emulate_rank import patch_dist
    from wan.distributed._test_transport import EmulatedGroup
    patch_dist()
    for P in args.bands:
        r = 1 if P > 2 else 0                                    # an interior rank (two neighbours) whenever there is one
        grp = EmulatedGroup(P, r, f'vae bands {P}')
        vae.model.decode_spatial(z[:, :2], group=grp)            # warm-up of the band-shaped launches
        torch.cuda.synchronize()
        grp.link_bytes = {k: 0 for k in grp.link_bytes}
        t1 = time.perf_counter()
        vae.model.decode_spatial(z, group=grp)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t1
        halo_b, gather_b = grp.link_bytes['p2p'], grp.link_bytes['all_gather']
        band_video = 3 * args.frames * Hd * (Wd // P) * 4
        # halos: per direction on its own link; the k|v all-gather: 1/P of the buffer to each peer, all links concurrently (EmulatedGroup counts per link);
        # the band of the video: ranks 1..P-1 -> rank 0 on P - 1 links concurrently
        link_s = (halo_b - (band_video if r else 0) + gather_b + band_video) / (args.link_gbps * 1e9)
        print(json.dumps({'metric': 'vae_decode_band_rank_sec', 'invalid': 'emulation: one rank of P on a loop-back group, link time modelled',
                          'ranks': P, 'emulated_rank': r, 'band_columns_latent': (Wd // 8) // P, 'rank_seconds_measured': sec,
                          'link_bytes_per_link': {'halo_columns_and_video_band': halo_b, 'kv_all_gather': gather_b}, 'link_seconds_modelled_not_overlapped': link_s,
                          'modelled_makespan_s': sec + link_s, 'single_gpu_s': dt_warm, 'modelled_efficiency': dt_warm / (P * (sec + link_s)), 'size': args.size, 'frames': args.frames}))

if args.stages:
    # per-stage milliseconds (HIP events around every _run_stage call of one more decode), the cost per MAC of each kernel
    # class relative to the wide 3x3x3 convolutions (-> wan/modules/vae.py REL_MS_PER_MAC), and the modelled makespan of
    # the layer pipeline cut by these times (WanVAE_.decode_pipelined)
    from wan.modules.vae import partition_costs, pipeline_makespan
    m = vae.model
    ev, orig = [], m._run_stage

    def timed(stage, x, run):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = orig(stage, x, run)
        b.record()
        ev.append((a, b))
        return y
    m._run_stage = timed
    m.decode(z, chunks=chunks)
    torch.cuda.synchronize()
    m._run_stage = orig
    stages = m._stages()
    S = len(stages)
    ms = [[a.elapsed_time(b) for a, b in ev[c * S:(c + 1) * S]] for c in range(len(chunks))]
    first, steady = ms[0], [sum(ms[c][i] for c in range(1, len(chunks)) if chunks[c] == chunks[1]) / max(1, sum(1 for c in range(1, len(chunks)) if chunks[c] == chunks[1])) for i in range(S)]
    macs = m.stage_costs(Hd // 8, Wd // 8)
    cls = {}
    base = m.P['decoder.head.0.gamma'].numel()
    for (kind, pre, _), c, t in zip(stages, macs, steady):
        k = kind
        if kind in ('conv1', 'res'):
            k = 'narrow' if m.P[pre + ('.weight' if kind == 'conv1' else 'residual.6.weight')].shape[0] == base else 'wide'
        a = cls.setdefault(k, [0.0, 0.0])
        a[0] += t
        a[1] += c * chunks[1]
    rel = {k: (v[0] / v[1]) / (cls['wide'][0] / cls['wide'][1]) for k, v in cls.items()}
    print('stage                                kind   first_ms  steady_ms  GMAC/frame')
    for (kind, pre, _), a, b, c in zip(stages, first, steady, macs):
        print(f'{pre:36s} {kind:6s} {a:9.2f} {b:10.2f} {c / 1e9:11.1f}')
    print('REL_MS_PER_MAC =', {k: round(v, 3) for k, v in rel.items()})
    h, w = Hd // 8, Wd // 8
    for P in (2, 4, 8):
        for name, weights in (('measured ms', steady), ('MACs', macs)):
            cuts = partition_costs(weights, P)
            seg_f = [sum(first[a:b]) for a, b in zip(cuts, cuts[1:])]
            seg_s = [sum(steady[a:b]) for a, b in zip(cuts, cuts[1:])]
            # bytes over a cut per steady chunk at ~45 GB/s effective per xGMI link (one direction, one peer)
            xfer = []
            for cpos in cuts[1:-1]:
                f, hh, ww, cc = m.stage_out_shape(cpos, chunks[1], False, h, w)
                xfer.append(f * hh * ww * cc * 4 / 45e9 * 1e3)
            mk, eff = pipeline_makespan(seg_f, seg_s, len(chunks), xfer)
            print(f'P={P} cut by {name:11s}: cuts {cuts}  steady segment ms {[round(v) for v in seg_s]}  transfer ms/chunk {[round(v, 1) for v in xfer]}  '
                  f'modelled makespan {mk / 1e3:.2f} s  (single GPU {(sum(first) + (len(chunks) - 1) * sum(steady)) / 1e3:.2f} s, efficiency {eff:.2f})')
