#!/usr/bin/env python3
"""Waveform pass benchmark: 65 536 x 4096-frame stereo MUSIC packets, device-resident, at 16 and at 24 bits.

Per depth and layout (STREAM, PACKETS; float32): the median of --steps passes after --warmup, timed by the pass's own HIP
events (alacgpu_waveform_last_ms), the bytes it reads and writes and the GB/s from them; beside it the decode of the same
batch (alacgpu_last_kernel_ms) and the composition of torch ops a caller has to write without the pass (a view, shifts and
ors for three-byte samples, a permute, a cast, a scale), run on the same device, timed with torch events, and checked
bit-equal to the pass first. Prints one JSON line.

--distinct packets are generated and the full-length ones among them named --packets / --distinct times each by the offsets (every packet is decoded and
converted on its own, so the tiling only saves generation time)."""
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

COPY_TBS = 6.3  # the device's measured copy rate
PEAK_TBS = 8.0  # bench.py's HBM figure


def composition(torch, pcm, n, fl, ch, depth, layout):
    """What a caller writes today: PCM slots [n, stride] uint8 (full packets) -> float32 [ch, n * fl] or [n, ch, fl]."""
    if depth == 16:
        v = pcm.view(torch.int16).view(n, fl, ch)
        scale = 2.0 ** -15
    else:
        b = pcm.view(n, fl, ch, 3)
        v = b[..., 0].to(torch.int32) | (b[..., 1].to(torch.int32) << 8) | (b[..., 2].to(torch.int32) << 16)
        v = (v << 8) >> 8
        scale = 2.0 ** -23
    if layout == "stream":
        return v.permute(2, 0, 1).reshape(ch, n * fl).to(torch.float32) * scale
    return v.permute(0, 2, 1).contiguous().to(torch.float32) * scale


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=65536)
    ap.add_argument("--distinct", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--depths", default="16,24")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    synth = importlib.import_module("saprobe-alac_amd.synth")
    from oracle import oracle
    dev = torch.device("cuda:0")
    n, fl, ch = a.packets, a.frames, 2
    results = []
    for depth in [int(d) for d in a.depths.split(",")]:
        ocfg = oracle.make_config(fl, depth, ch)
        cfg = pkg.PacketConfig(FrameLength=fl, BitDepth=depth, NumChannels=ch)
        bpf = ch * pkg.bytes_per_sample(depth)
        b = synth.gen_batch(ocfg, a.distinct, threads=a.threads, want_pcm=False)
        # synth's stream has a few short packets of its own; the benchmark batch is full packets only
        full = torch.from_numpy(np.nonzero(b.frames == fl)[0]).to(dev)
        pick = full[torch.arange(n, device=dev) % full.numel()]
        d_blob = torch.from_numpy(b.blob).to(dev)
        d_off = torch.from_numpy(b.offsets.astype(np.int64)).to(dev)[pick].contiguous()
        d_sz = torch.from_numpy(b.sizes.astype(np.int32)).to(dev)[pick].contiguous()
        stride = fl * bpf  # a multiple of 16: the decode's fast layout
        pcm = torch.empty((n, stride), dtype=torch.uint8, device=dev)
        fr = torch.zeros(n, dtype=torch.int32, device=dev)
        st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        wave = torch.empty(n * ch * fl, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with pkg.NewPacketDecoder(cfg, 0) as dec:
            dec.reserve(n)
            dec_times = []
            for k in range(a.warmup + 3):
                dec.decode_batch_device(d_blob.data_ptr(), d_blob.numel(), d_off.data_ptr(), d_sz.data_ptr(), n, pcm.data_ptr(), stride,
                                        fr.data_ptr(), st.data_ptr(), sync=True)
                if k >= a.warmup:
                    dec_times.append(dec.last_kernel_ms())
            assert bool((st == 0).all()) and bool((fr == fl).all())
            for layout in ("stream", "packets"):
                cs, ps = (n * fl, 0) if layout == "stream" else (fl, ch * fl)
                times = []
                for k in range(a.warmup + a.steps):
                    dec.waveform_device(pcm.data_ptr(), stride, fr.data_ptr(), st.data_ptr(), n,
                                        pkg.WAVE_STREAM if layout == "stream" else pkg.WAVE_PACKETS, pkg.WAVE_FLOAT, wave.data_ptr(), cs, ps,
                                        None, sync=True)
                    if k >= a.warmup:
                        times.append(dec.waveform_last_ms())
                # the baseline, checked equal first
                comp = composition(torch, pcm, n, fl, ch, depth, layout)
                equal = torch.equal(comp.reshape(-1).view(torch.int32), wave.view(torch.int32))
                del comp
                comp_times = []
                for k in range(a.warmup + a.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    comp = composition(torch, pcm, n, fl, ch, depth, layout)
                    e1.record()
                    e1.synchronize()
                    del comp
                    if k >= a.warmup:
                        comp_times.append(e0.elapsed_time(e1))
                ms, comp_ms = statistics.median(times), statistics.median(comp_times)
                moved = n * fl * bpf + n * fl * ch * 4 + n * 8  # PCM in, waveform out, frame counts and status words
                tbs = moved / (ms * 1e-3) / 1e12
                results.append(dict(depth=depth, layout=layout, type="float32", packets=n, frames=fl, channels=ch,
                                    wave_ms=round(ms, 4), wave_ms_all=[round(t, 4) for t in times], bytes_moved=moved,
                                    gb_per_s=round(tbs * 1e3, 1), fraction_of_copy_rate=round(tbs / COPY_TBS, 3),
                                    fraction_of_peak=round(tbs / PEAK_TBS, 3), decode_ms=round(statistics.median(dec_times), 4),
                                    torch_ms=round(comp_ms, 4), torch_ms_all=[round(t, 4) for t in comp_times],
                                    equal_to_torch=bool(equal), faster_than_torch=bool(max(times) < min(comp_times)),
                                    speedup_vs_torch=round(comp_ms / ms, 2)))
        del pcm, wave
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "waveform_bench", "device": torch.cuda.get_device_name(0), "results": results}))
    return 0 if all(r["equal_to_torch"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
