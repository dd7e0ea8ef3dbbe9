#!/usr/bin/env python3
"""Clip gather benchmark: --clips one-second crops out of --files synthetic 60-second 16-bit stereo files (written with
save()), at random frame offsets.

1. The gather against the decode in front of it: the covering packets of every crop through one device decode, then
   alacgpu_clips_device; both timed by their own HIP events (alacgpu_last_kernel_ms, alacgpu_clips_last_ms), the median of
   --steps runs after --warmup.
2. load_clips() against what a caller writes without it: load() of each file, then slice, pad and stack with torch. Wall
   clock around the whole call, the device idle before and after, the same median; the two results compared bit for bit.
3. load(frame_offset, num_frames) against load()[:, a:b] on one of the files, likewise.

Prints one JSON line."""
import argparse
import importlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def wall(torch, fn, steps, warmup):
    """-> (median ms, all ms, the last result): wall clock around fn(), the device idle before and after."""
    times, out = [], None
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), [round(t, 3) for t in times], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    stream = importlib.import_module("saprobe-alac_amd.stream")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    fl, ch, L = 4096, 2, a.rate
    total = a.seconds * a.rate

    # the files: a few drifting sines and some noise per channel, 16-bit stereo
    files = []
    t = torch.arange(total, device=dev, dtype=torch.float32) / a.rate
    for k in range(a.files):
        gen = torch.Generator(device=dev).manual_seed(k)
        wave = torch.stack([0.3 * torch.sin(2 * np.pi * (220.0 * (k + 1) + 3 * c) * t) + 0.2 * torch.sin(2 * np.pi * 1000.3 * (c + 1) * t + k)
                            + 0.01 * torch.randn(total, device=dev, generator=gen) for c in range(ch)])
        buf = io.BytesIO()
        pkg.save(buf, wave, a.rate, bits_per_sample=16, frame_length=fl)
        files.append(buf.getvalue())
    del t, wave
    which = [int(x) for x in rng.integers(0, a.files, a.clips)]
    starts = [int(x) for x in rng.integers(0, total - L // 2, a.clips)]  # some run over their file's end
    sources = [files[k] for k in which]

    # 1. the gather and the decode in front of it
    tracks = []
    for data in sources:
        _, view, track, cfg = stream.open_track(data)
        tracks.append((np.frombuffer(view, dtype=np.uint8), track.offsets.astype(np.int64), track.sizes.astype(np.int64), cfg))
    first = [s // fl for s in starts]
    count = [max(0, min(-(-(s + L) // fl), len(t[2])) - p) for s, p, t in zip(starts, first, tracks)]
    blob, offsets, sizes, begin, limit = pkg._clip_batch(tracks, starts, first, count, fl)
    n, B = len(sizes), a.clips
    d_blob = torch.from_numpy(blob).to(dev)
    d_off = torch.from_numpy(offsets).to(dev)
    d_sz = torch.from_numpy(sizes.astype(np.int32)).to(dev)
    d_begin = torch.tensor(begin, dtype=torch.int64, device=dev)
    d_limit = torch.tensor(limit, dtype=torch.int64, device=dev)
    with pkg.NewPacketDecoder(cfg, 0) as dec:
        stride = (dec.frame_bytes + 15) // 16 * 16
        pcm = torch.empty((n, stride), dtype=torch.uint8, device=dev)
        fr = torch.zeros(n, dtype=torch.int32, device=dev)
        st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        clips = torch.empty((B, ch, L), dtype=torch.float32, device=dev)
        valid = torch.zeros(B, dtype=torch.int32, device=dev)
        dec.reserve(n)
        torch.cuda.synchronize()
        dec_ms, clip_ms = [], []
        for k in range(a.warmup + a.steps):
            dec.decode_batch_device(d_blob.data_ptr(), d_blob.numel(), d_off.data_ptr(), d_sz.data_ptr(), n, pcm.data_ptr(), stride,
                                    fr.data_ptr(), st.data_ptr(), sync=False)
            dec.clips_device(pcm.data_ptr(), stride, fr.data_ptr(), st.data_ptr(), n, d_begin.data_ptr(), d_limit.data_ptr(), B, L,
                             pkg.WAVE_FLOAT, clips.data_ptr(), L, ch * L, valid.data_ptr(), None, sync=True)
            if k >= a.warmup:
                dec_ms.append(dec.last_kernel_ms())
                clip_ms.append(dec.clips_last_ms())
        assert not bool(st.any())
    moved = int(valid.sum().item()) * ch * 2 + B * ch * L * 4  # PCM read, clips written
    g_ms = statistics.median(clip_ms)
    gather = dict(packets=n, clips=B, clip_frames=L, decode_ms=round(statistics.median(dec_ms), 4), gather_ms=round(g_ms, 4),
                  gather_ms_all=[round(x, 4) for x in clip_ms], bytes_moved=moved, gb_per_s=round(moved / (g_ms * 1e-3) / 1e9, 1))

    # 2. load_clips against load() of each file + slice, pad, stack
    def composed():
        waves = {}
        for k in sorted(set(which)):
            waves[k] = pkg.load(files[k])[0]
        rows = []
        for k, s in zip(which, starts):
            piece = waves[k][:, s:s + L]
            rows.append(torch.nn.functional.pad(piece, (0, L - piece.shape[1])))
        return torch.stack(rows)

    new_ms, new_all, got = wall(torch, lambda: pkg.load_clips(sources, starts, L), a.steps, a.warmup)
    old_ms, old_all, want = wall(torch, composed, a.steps, a.warmup)
    equal = torch.equal(got[0].view(torch.int32), want.view(torch.int32)) and torch.equal(clips.view(torch.int32), want.view(torch.int32))
    batch = dict(load_clips_ms=round(new_ms, 3), load_clips_ms_all=new_all, composed_ms=round(old_ms, 3), composed_ms_all=old_all,
                 equal=bool(equal), speedup=round(old_ms / new_ms, 2))

    # 3. load(frame_offset, num_frames) against load()[:, a:b]
    s0 = total // 2 + 1234
    r_ms, r_all, part = wall(torch, lambda: pkg.load(files[0], frame_offset=s0, num_frames=L)[0], a.steps, a.warmup)
    f_ms, f_all, whole = wall(torch, lambda: pkg.load(files[0])[0][:, s0:s0 + L], a.steps, a.warmup)
    ranged = dict(ranged_ms=round(r_ms, 3), ranged_ms_all=r_all, full_slice_ms=round(f_ms, 3), full_slice_ms_all=f_all,
                  equal=bool(torch.equal(part, whole)), speedup=round(f_ms / r_ms, 2))

    print(json.dumps({"tool": "clips_bench", "device": torch.cuda.get_device_name(0), "files": a.files, "seconds": a.seconds,
                      "gather": gather, "load_clips": batch, "load_range": ranged}))
    return 0 if batch["equal"] and ranged["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
