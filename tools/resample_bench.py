#!/usr/bin/env python3
"""Resampler benchmark: alacgpu_resample_device against what torchaudio.functional.resample runs for sinc_interp_hann, which
is written out here in torch because torchaudio is not a dependency: a pad, one strided conv1d over the new / gcd kernels of 2 *
width + orig / gcd taps each (zeros included), a transpose and a slice.

Shapes: 64 x 2 rows of one second at 44 100 -> 16 000 and at 48 000 -> 44 100, and one 300-second stereo file at 44 100 ->
16 000. Both sides are timed by HIP events around the work on the device, the median of --steps runs after --warmup; the
two results are compared, and the largest difference is printed (the table entries are the same float32 values; the orders of
summation differ). Prints one JSON line."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def full_kernels(orig, new, W=6, rolloff=0.99):
    """torchaudio's _get_sinc_resample_kernel for sinc_interp_hann -> (kernels [n, 1, 2 * width + o] float32, width, o, n)."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = int(math.ceil(W * o / base))
    k = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    t = np.clip((k - np.arange(n, dtype=np.float64)[:, None] / n) * base, -W, W)
    h = np.where(np.abs(t) == W, 0.0, np.sinc(t) * np.cos(np.pi * t / (2 * W)) ** 2 * base / o)
    return h.astype(np.float32)[:, None, :], width, o, n


def conv_resample(torch, x, kernels, width, o, n, frames):
    """rows [R, T] -> [R, frames]: torchaudio's _apply_sinc_resample_kernel."""
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(x[:, None], (width, width + o)), kernels, stride=o)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :frames]


def events_ms(torch, fn, steps, warmup):
    """-> (median ms, all ms, the last result): torch events on the current stream around fn()."""
    times, out = [], None
    for k in range(warmup + steps):
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
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    results = []
    for name, rows, T, orig, new in (("64x2x1s", 128, 44100, 44100, 16000), ("64x2x1s", 128, 48000, 48000, 44100),
                                     ("1x2x300s", 2, 300 * 44100, 44100, 16000)):
        x = torch.rand((rows, T), device=dev, generator=gen) * 2 - 1
        kernels, width, o, n = full_kernels(orig, new)
        d_kernels = torch.from_numpy(kernels).to(dev)
        with pkg.NewResampler(orig, new) as rs:
            frames = rs.out_frames(T)
            out = torch.empty((rows, frames), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            ours = []
            for k in range(a.warmup + a.steps):
                rs.resample_device(x.data_ptr(), T, rows, T, out.data_ptr(), frames, sync=True)
                if k >= a.warmup:
                    ours.append(rs.last_ms())
            plan = rs.plan()
        c_ms, c_all, want = events_ms(torch, lambda: conv_resample(torch, x, d_kernels, width, o, n, frames), a.steps, a.warmup)
        k_ms = statistics.median(ours)
        moved = 4 * rows * (T + frames)
        results.append(dict(shape=name, rows=rows, in_frames=T, orig=orig, new=new, taps=plan["taps"], full_taps=2 * width + o,
                            tile_out=plan["tile_out"], resample_ms=round(k_ms, 4), resample_ms_all=[round(t, 4) for t in ours],
                            gb_per_s=round(moved / (k_ms * 1e-3) / 1e9, 1), conv1d_ms=round(c_ms, 4), conv1d_ms_all=c_all,
                            speedup=round(c_ms / k_ms, 2), max_abs_diff=float((out - want).abs().max().item())))
        del x, out, want
    print(json.dumps({"tool": "resample_bench", "device": torch.cuda.get_device_name(0), "results": results}))
    return 0 if all(r["max_abs_diff"] < 1e-4 for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
