#!/usr/bin/env python3
"""Kaldi fbank benchmark: alacgpu_fbank_device against the same steps written with float32 torch ops on the same device tensors:
unfold (a strided copy of every frame), mean removal, pre-emphasis, the Povey window, zero padding, torch.fft.rfft, |.|^2, a
matmul with the plan's dense filterbank and log of the clamped result. The torch side runs in chunks of --chunk rows, so that
its intermediates (five times the frames' size) stay bounded.

Shapes: 1 024 rows of 30 s at 16 kHz with 80 bins (25 / 10 ms: W 400, h 160, N 512), and 256 rows of 10 s at 48 kHz with 128
bins (W 1200, h 480, N 2048); --rows scales the first. --transform direct | fft | both picks the pass's transform; with both, the
two handles run on the same tensors in one process. All sides are timed by HIP events around the work on the device, the
median of --steps runs after --warmup.

Every transform that ran reports its own numbers. The direct transform's are fbank_ms, fbank_ms_all, speedup (torch_ms /
fbank_ms), tile_frames, lds_bytes, max_abs_diff_ln, and floor_ms, floor_fraction = floor_ms / fbank_ms: floor_ms is what the direct
DFT's 2 * W * K fmaf per frame take at the f32 issue peak (157.3 TFLOP/s), a floor of that transform alone. The FFT's are fft_ms,
fft_ms_all, fft_speedup_over_torch, fft_tile_frames, fft_batch_frames, fft_lds_bytes, fft_radix, fft_max_abs_diff_ln, and with both
fft_speedup_over_direct. bytes_moved is what either pass reads and writes: the samples once and the features once. Each result is
compared with the torch ops' where the mel energy lies within 1e-6 of the largest (the orders of summation differ). Prints one
JSON line; exit status 1 where a difference reaches 1e-2."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_FLOPS = 157.3e12
EPS = 2.0 ** -23


def events_ms(torch, fn, steps, warmup):
    """-> (median ms, all ms, the last result): torch events on the current stream around fn()."""
    times, out = [], None
    for k in range(warmup + steps):
        out = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b))
    return statistics.median(times), [round(t, 4) for t in times], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--transform", choices=("direct", "fft", "both"), default="direct")
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    results = []
    for name, rows, T, rate, bins in (("asr %dx30s@16k" % a.rows, a.rows, 480000, 16000, 80), ("256x10s@48k", 256, 480000, 48000, 128)):
        W, h = int(rate * 25.0 * 0.001), int(rate * 10.0 * 0.001)
        x = torch.rand((rows, T), device=dev, generator=gen) * 2 - 1
        timed = {}
        for transform in ("direct", "fft") if a.transform == "both" else (a.transform,):
            with pkg.NewKaldiFeatures(rate, W, h, num_mel_bins=bins, transform=transform) as kf:
                plan = kf.plan()
                frames = kf.out_frames(T)
                out = torch.empty((rows, frames, bins), dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                ours = []
                for k in range(a.warmup + a.steps):
                    kf.features_device(x.data_ptr(), T, rows, T, out.data_ptr(), frames * bins, bins, sync=True)
                    if k >= a.warmup:
                        ours.append(kf.last_ms())
                timed[transform] = (ours, out, plan, kf.fft_plan())
        plan = next(iter(timed.values()))[2]  # n_fft, the filterbank and frames are the same on both handles
        N, K = plan["n_fft"], plan["n_freqs"]
        fb = np.zeros((bins, K), np.float32)
        for m in range(bins):
            fb[m, plan["first"][m]:plan["first"][m] + plan["taps"]] = plan["fb"][m]
        d_fb = torch.from_numpy(fb).to(dev).T.contiguous()
        win = torch.hann_window(W, periodic=False, dtype=torch.float32, device=dev) ** 0.85

        def ops():
            parts = []
            for r0 in range(0, rows, a.chunk):
                fr = x[r0:r0 + a.chunk].unfold(-1, W, h)                       # a view; the next op copies every frame
                fr = fr - fr.mean(dim=-1, keepdim=True)
                fr = fr - 0.97 * torch.cat([fr[..., :1], fr[..., :-1]], dim=-1)
                fr = torch.nn.functional.pad(fr * win, (0, N - W))
                p = torch.fft.rfft(fr).abs() ** 2
                parts.append(torch.log(torch.clamp(torch.matmul(p, d_fb), min=EPS)))
            return torch.cat(parts)

        t_ms, t_all, want = events_ms(torch, ops, a.steps, a.warmup)
        loud = want > (want.max() - 13.8)  # within 1e-6 of the largest mel energy
        res = dict(shape=name, rows=rows, in_frames=T, frames=frames, frame_length=W, frame_shift=h, n_fft=N, num_mel_bins=bins,
                   taps=plan["taps"], transform=a.transform, torch_ms=round(t_ms, 4), torch_ms_all=t_all,
                   bytes_moved=4 * rows * (T + frames * bins))
        if "direct" in timed:
            d_all, d_out, d_plan, _ = timed["direct"]
            k_ms = statistics.median(d_all)
            floor_ms = rows * frames * 2.0 * W * K * 2.0 / PEAK_F32_FLOPS * 1e3
            res.update(tile_frames=d_plan["tile_frames"], lds_bytes=d_plan["lds_bytes"], fbank_ms=round(k_ms, 4),
                       fbank_ms_all=[round(t, 4) for t in d_all], speedup=round(t_ms / k_ms, 2), floor_ms=round(floor_ms, 4),
                       floor_fraction=round(floor_ms / k_ms, 4), max_abs_diff_ln=float((d_out - want)[loud].abs().max().item()))
        if "fft" in timed:
            f_all, f_out, f_plan, f_fft = timed["fft"]
            f_ms = statistics.median(f_all)
            res.update(fft_ms=round(f_ms, 4), fft_ms_all=[round(t, 4) for t in f_all], fft_tile_frames=f_plan["tile_frames"],
                       fft_batch_frames=f_fft["batch_frames"], fft_lds_bytes=f_plan["lds_bytes"], fft_radix=f_fft["radix"],
                       fft_speedup_over_torch=round(t_ms / f_ms, 2), fft_max_abs_diff_ln=float((f_out - want)[loud].abs().max().item()))
            if "direct" in timed:
                res["fft_speedup_over_direct"] = round(k_ms / f_ms, 2)
        results.append(res)
        del x, out, want, loud, timed, res
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "fbank_bench", "device": torch.cuda.get_device_name(0), "results": results}))
    return 0 if all(r.get(k, 0.0) < 1e-2 for r in results for k in ("max_abs_diff_ln", "fft_max_abs_diff_ln")) else 1


if __name__ == "__main__":
    sys.exit(main())
