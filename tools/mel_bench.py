#!/usr/bin/env python3
"""Spectrogram benchmark: alacgpu_mel_device against the float32 torch ops it replaces, on the same device tensors: torch.stft
(periodic Hann window, reflect padding), abs() ** 2, a matmul with the plan's dense filterbank and log10 of the clamped result.

Shapes: 1 024 rows of 30 s at 16 kHz in Whisper's configuration (n_fft 400, hop 160, 80 slaney mels), 256 rows of 10 s at 44.1
kHz with torchaudio's MelSpectrogram defaults (n_fft 400, hop 200, 128 htk mels), and 256 rows of 10 s at 48 kHz with n_fft 2048,
hop 512 and 128 htk mels; --rows scales the first. --transform direct | fft | both picks the pass's transform; with both, the
two handles run on the same tensors in one process. All sides are timed by HIP events around the work on the device, the
median of --steps runs after --warmup.

Every transform that ran reports its own numbers. The direct transform's are mel_ms, mel_ms_all, speedup (torch_ms / mel_ms),
tile_frames, lds_bytes, max_abs_diff_log10, and floor_ms, floor_fraction = floor_ms / mel_ms: floor_ms is what the direct DFT's
2 * n_fft * (n_fft / 2 + 1) fmaf per frame take at the f32 issue peak (157.3 TFLOP/s), a floor of that transform alone. The
FFT's are fft_ms, fft_ms_all, fft_speedup_over_torch, fft_tile_frames, fft_batch_frames, fft_lds_bytes, fft_radix,
fft_max_abs_diff_log10, and with both fft_speedup_over_direct. Each result is compared with the torch ops' where those lie within
1e-6 of the largest value (the orders of summation differ). Prints one JSON line; exit status 1 where a difference reaches 1e-3."""
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
    ap.add_argument("--transform", choices=("direct", "fft", "both"), default="direct")
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    floor = 1e-10
    results = []
    for name, rows, T, kw in (
            ("whisper %dx30s@16k" % a.rows, a.rows, 480000, dict(sample_rate=16000, n_fft=400, hop_length=160, n_mels=80, f_max=8000.0,
                                                               mel_scale="slaney", norm="slaney")),
            ("torchaudio 256x10s@44.1k", 256, 441000, dict(sample_rate=44100, n_fft=400, n_mels=128)),
            ("n2048 256x10s@48k", 256, 480000, dict(sample_rate=48000, n_fft=2048, hop_length=512, n_mels=128))):
        x = torch.rand((rows, T), device=dev, generator=gen) * 2 - 1
        timed = {}
        for transform in ("direct", "fft") if a.transform == "both" else (a.transform,):
            with pkg.NewMelSpectrogram(log="log10", floor=floor, transform=transform, **kw) as ms:
                plan = ms.plan()
                frames = ms.out_frames(T)
                out = torch.empty((rows, plan["bins"], frames), dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                ours = []
                for k in range(a.warmup + a.steps):
                    ms.mel_device(x.data_ptr(), T, rows, T, out.data_ptr(), plan["bins"] * frames, frames, sync=True)
                    if k >= a.warmup:
                        ours.append(ms.last_ms())
                timed[transform] = (ours, out, plan, ms.fft_plan())
        plan = next(iter(timed.values()))[2]  # n_fft, the filterbank and frames are the same on both handles
        N, hop, K = plan["n_fft"], plan["hop_length"], plan["n_freqs"]
        fb = np.zeros((plan["n_mels"], K), np.float32)
        for m in range(plan["n_mels"]):
            fb[m, plan["first"][m]:plan["first"][m] + plan["taps"]] = plan["fb"][m]
        d_fb = torch.from_numpy(fb).to(dev)
        win = torch.hann_window(plan["win_length"], periodic=True, dtype=torch.float32, device=dev)

        def ops():
            p = torch.stft(x, N, hop_length=hop, win_length=plan["win_length"], window=win, center=True, pad_mode="reflect",
                           return_complex=True).abs() ** 2
            return torch.log10(torch.clamp(torch.matmul(d_fb, p), min=floor))

        t_ms, t_all, want = events_ms(torch, ops, a.steps, a.warmup)
        loud = want > (want.max() - 6.0)  # within 1e-6 of the largest power
        res = dict(shape=name, rows=rows, in_frames=T, frames=frames, n_fft=N, hop_length=hop, n_mels=plan["n_mels"],
                   taps=plan["taps"], transform=a.transform, torch_ms=round(t_ms, 4), torch_ms_all=t_all)
        if "direct" in timed:
            d_all, d_out, d_plan, _ = timed["direct"]
            k_ms = statistics.median(d_all)
            floor_ms = rows * frames * 2.0 * N * K * 2.0 / PEAK_F32_FLOPS * 1e3
            res.update(tile_frames=d_plan["tile_frames"], lds_bytes=d_plan["lds_bytes"], mel_ms=round(k_ms, 4),
                       mel_ms_all=[round(t, 4) for t in d_all], speedup=round(t_ms / k_ms, 2), floor_ms=round(floor_ms, 4),
                       floor_fraction=round(floor_ms / k_ms, 4), max_abs_diff_log10=float((d_out - want)[loud].abs().max().item()))
        if "fft" in timed:
            f_all, f_out, f_plan, f_fft = timed["fft"]
            f_ms = statistics.median(f_all)
            res.update(fft_ms=round(f_ms, 4), fft_ms_all=[round(t, 4) for t in f_all], fft_tile_frames=f_plan["tile_frames"],
                       fft_batch_frames=f_fft["batch_frames"], fft_lds_bytes=f_plan["lds_bytes"], fft_radix=f_fft["radix"],
                       fft_speedup_over_torch=round(t_ms / f_ms, 2),
                       fft_max_abs_diff_log10=float((f_out - want)[loud].abs().max().item()))
            if "direct" in timed:
                res["fft_speedup_over_direct"] = round(k_ms / f_ms, 2)
        results.append(res)
        del x, out, want, loud, timed, res
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "mel_bench", "device": torch.cuda.get_device_name(0), "results": results}))
    return 0 if all(r.get(k, 0.0) < 1e-3 for r in results for k in ("max_abs_diff_log10", "fft_max_abs_diff_log10")) else 1


if __name__ == "__main__":
    sys.exit(main())
