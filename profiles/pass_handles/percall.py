#!/usr/bin/env python3
"""Wall time per call of each row pass's device entry (sync=True), for one library (ALACGPU_LIB picks it):

    python3 profiles/pass_handles/percall.py [--reps 7]

Per pass a small shape where the host's share dominates (8 rows of 4096 samples) and the first shape of its bench tool under
tools/. A repetition is a host clock around --calls calls, each of which ends in a stream synchronise; with --calls 0 (the
default) it is as many calls as take about --window seconds, 20 at the least, counted from warm-up calls. The line has the
median, the least and the greatest repetition in microseconds per call, and the SHA-256 of the output, so that two libraries can
be held to the same bits. Prints one JSON line per case."""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--window", type=float, default=0.2)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    dev = torch.device("cuda:0")
    whisper = dict(sample_rate=16000, n_fft=400, hop_length=160, n_mels=80, f_max=8000.0, mel_scale="slaney", norm="slaney", log="log10")
    passes = (
        ("resample", lambda: pkg.NewResampler(44100, 16000), (128, 44100),
         lambda h, frames: (frames,), lambda h, x, T, rows, out, frames: h.resample_device(x, T, rows, T, out, frames, sync=True)),
        ("mel", lambda: pkg.NewMelSpectrogram(**whisper), (1024, 480000),
         lambda h, frames: (h.bins, frames), lambda h, x, T, rows, out, frames: h.mel_device(x, T, rows, T, out, h.bins * frames, frames, sync=True)),
        ("mel_fft", lambda: pkg.NewMelSpectrogram(transform="fft", **whisper), (1024, 480000),
         lambda h, frames: (h.bins, frames), lambda h, x, T, rows, out, frames: h.mel_device(x, T, rows, T, out, h.bins * frames, frames, sync=True)),
        ("kaldi", lambda: pkg.NewKaldiFeatures(16000, 400, 160, num_mel_bins=80), (1024, 480000),
         lambda h, frames: (frames, h.cols), lambda h, x, T, rows, out, frames: h.features_device(x, T, rows, T, out, h.cols * frames, h.cols, sync=True)))
    for name, new, bench_shape, shape_of, call in passes:
        for what, (rows, T) in (("small", (8, 4096)), ("bench", bench_shape)):
            gen = torch.Generator(device=dev).manual_seed(1)
            x = torch.rand((rows, T), device=dev, generator=gen) * 2 - 1
            with new() as h:
                frames = h.out_frames(T)
                out = torch.zeros((rows,) + shape_of(h, frames), dtype=torch.float32, device=dev)
                torch.cuda.synchronize()
                for k in range(25):  # warm up, and count by the last 20 what a window holds
                    if k == 5:
                        t0 = time.perf_counter()
                    call(h, x.data_ptr(), T, rows, out.data_ptr(), frames)
                calls = a.calls or max(20, min(5000, int(a.window * 20 / (time.perf_counter() - t0))))
                reps = []
                for k in range(a.reps + 1):  # the first repetition warms up too
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        call(h, x.data_ptr(), T, rows, out.data_ptr(), frames)
                    reps.append((time.perf_counter() - t0) / calls * 1e6)
                reps = reps[1:]
                kernel_ms = h.last_ms()
            digest = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]
            print(json.dumps(dict(lib=os.path.basename(os.path.dirname(pkg.lib_path())), name=name, shape=what, rows=rows, in_frames=T,
                                  calls=calls, us_per_call=round(statistics.median(reps), 2), least=round(min(reps), 2),
                                  greatest=round(max(reps), 2), kernel_us=round(kernel_ms * 1e3, 2), sha256=digest)), flush=True)
            del x, out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
