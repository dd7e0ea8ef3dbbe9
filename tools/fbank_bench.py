#!/usr/bin/env python3
"""Kaldi fbank benchmark: alacgpu_fbank_device against the same steps written with float32 torch ops on the same device tensors:
unfold (a strided copy of every frame), mean removal, pre-emphasis, the Povey window, zero padding, torch.fft.rfft, |.|^2, a
matmul with the plan's dense filterbank and log of the clamped result. The torch side runs in chunks of --chunk rows, so that
its intermediates (five times the frames' size) stay bounded.

Shapes: 1 024 rows of 30 s at 16 kHz with 80 bins (25 / 10 ms: W 400, h 160, N 512), and 256 rows of 10 s at 48 kHz with 128
bins (W 1200, h 480, N 2048); --rows scales the first. Both sides are timed by HIP events around the work on the device, the
median of --steps runs after --warmup. floor_ms is what the direct DFT's 2 * W * K fmaf per frame take at the f32 issue peak
(157.3 TFLOP/s), floor_fraction = floor_ms / fbank_ms. The two results are compared where the mel energy lies within 1e-6 of
the largest (the orders of summation differ). Prints one JSON line."""
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
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    results = []
    for name, rows, T, rate, bins in (("asr %dx30s@16k" % a.rows, a.rows, 480000, 16000, 80), ("256x10s@48k", 256, 480000, 48000, 128)):
        W, h = int(rate * 25.0 * 0.001), int(rate * 10.0 * 0.001)
        x = torch.rand((rows, T), device=dev, generator=gen) * 2 - 1
        with pkg.NewKaldiFeatures(rate, W, h, num_mel_bins=bins) as kf:
            plan = kf.plan()
            frames = kf.out_frames(T)
            out = torch.empty((rows, frames, bins), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            ours = []
            for k in range(a.warmup + a.steps):
                kf.features_device(x.data_ptr(), T, rows, T, out.data_ptr(), frames * bins, bins, sync=True)
                if k >= a.warmup:
                    ours.append(kf.last_ms())
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
        k_ms = statistics.median(ours)
        floor_ms = rows * frames * 2.0 * W * K * 2.0 / PEAK_F32_FLOPS * 1e3
        loud = want > (want.max() - 13.8)  # within 1e-6 of the largest mel energy
        diff = float((out - want)[loud].abs().max().item())
        results.append(dict(shape=name, rows=rows, in_frames=T, frames=frames, frame_length=W, frame_shift=h, n_fft=N, num_mel_bins=bins,
                            taps=plan["taps"], tile_frames=plan["tile_frames"], lds_bytes=plan["lds_bytes"], fbank_ms=round(k_ms, 4),
                            fbank_ms_all=[round(t, 4) for t in ours], torch_ms=round(t_ms, 4), torch_ms_all=t_all,
                            speedup=round(t_ms / k_ms, 2), floor_ms=round(floor_ms, 4), floor_fraction=round(floor_ms / k_ms, 4),
                            max_abs_diff_ln=diff))
        del x, out, want, loud
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "fbank_bench", "device": torch.cuda.get_device_name(0), "results": results}))
    return 0 if all(r["max_abs_diff_ln"] < 1e-2 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
