#!/usr/bin/env python3
"""Batch encoder benchmark: 65 536 x 4096-frame stereo MUSIC packets, device-resident, at 16 and at 24 bits.

Per depth: the median kernel time of --steps encodes (HIP events around all of an encode's kernels, after --warmup),
Msamples/s from it, encoded bytes / raw bytes, a bit-exact round trip through the GPU decoder (d_sizes = NULL, the
encoder's offsets), and the CPU baseline: the host build of csrc/alac_enc.h (tests/host_sim/enc_sim.cpp) on --threads
threads over --cpu-packets of the same packets. Prints one JSON line.

The PCM is synth's seeded MUSIC source: --distinct packets generated, tiled to --packets (each packet is encoded on its own,
so the tiling only saves generation time)."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=65536)
    ap.add_argument("--distinct", type=int, default=8192)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--depths", default="16,24")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-packets", type=int, default=2048)
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    synth = importlib.import_module("saprobe-alac_amd.synth")
    from oracle import oracle
    from tests.test_encoder_host import build_enc_sim
    sim = build_enc_sim()
    dev = torch.device("cuda:0")
    results = []
    for depth in [int(d) for d in a.depths.split(",")]:
        ocfg = oracle.make_config(a.frames, depth, 2)
        cfg = pkg.PacketConfig(FrameLength=a.frames, BitDepth=depth, NumChannels=2)
        bpf = 2 * (2 if depth == 16 else 3)
        b = synth.gen_batch(ocfg, a.distinct, threads=a.threads)
        rows = b.pcm
        reps = (a.packets + a.distinct - 1) // a.distinct
        d_rows = torch.from_numpy(rows).to(dev)
        d_pcm = d_rows.repeat(reps, 1)[:a.packets].contiguous().view(-1)
        frames = a.packets * a.frames
        raw = frames * bpf
        with pkg.NewPacketEncoder(cfg) as enc:
            cap = enc.max_bytes(frames)
            d_blob = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_off = torch.zeros(a.packets + 1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            times = []
            for k in range(a.warmup + a.steps):
                enc.encode_device(d_pcm.data_ptr(), frames, d_blob.data_ptr(), cap, d_off.data_ptr(), sync=True)
                if k >= a.warmup:
                    times.append(enc.last_kernel_ms())
        ms = statistics.median(times)
        total = int(d_off[-1].item())
        # round trip through the GPU decoder
        stride = a.frames * bpf
        d_out = torch.empty((a.packets, stride), dtype=torch.uint8, device=dev)
        d_fr = torch.zeros(a.packets, dtype=torch.int32, device=dev)
        d_st = torch.full((a.packets,), -1, dtype=torch.int32, device=dev)
        with pkg.NewPacketDecoder(cfg, 0) as dec:
            dec.decode_batch_device(d_blob.data_ptr(), total, d_off.data_ptr(), None, a.packets, d_out.data_ptr(), stride,
                                    d_fr.data_ptr(), d_st.data_ptr(), sync=True)
            dec_ms = dec.last_kernel_ms()
        exact = bool((d_st == 0).all()) and bool((d_fr == a.frames).all()) and torch.equal(d_out.view(-1), d_pcm)
        del d_out, d_blob, d_pcm
        torch.cuda.empty_cache()
        # CPU baseline: the host build of the same logic
        m = min(a.cpu_packets, a.distinct)
        cpu_pcm = np.ascontiguousarray(rows[:m]).reshape(-1)
        cpu_cap = int(sim.enc_sim_max_bytes(ctypes.byref(ocfg), m * a.frames))
        cpu_blob = np.empty(cpu_cap, np.uint8)
        cpu_off = np.zeros(m + 1, np.uint64)
        t0 = time.perf_counter()
        sim.enc_sim_encode(ctypes.byref(ocfg), cpu_pcm.ctypes.data, m * a.frames, cpu_blob.ctypes.data, cpu_cap,
                           cpu_off.ctypes.data, None, None, a.threads)
        cpu_s = time.perf_counter() - t0
        samples = frames * 2
        gpu_ms_s = samples / (ms * 1e3)
        cpu_ms_s = m * a.frames * 2 / (cpu_s * 1e6)
        results.append(dict(depth=depth, packets=a.packets, frames=a.frames, kernel_ms=round(ms, 3),
                            kernel_ms_all=[round(t, 3) for t in times], msamples_per_s=round(gpu_ms_s, 1),
                            ratio=round(total / raw, 4), roundtrip_bit_exact=exact, decode_ms=round(dec_ms, 3),
                            cpu_threads=a.threads, cpu_packets=m, cpu_msamples_per_s=round(cpu_ms_s, 1),
                            speedup_vs_cpu=round(gpu_ms_s / cpu_ms_s, 1)))
    print(json.dumps({"tool": "encode_bench", "device": torch.cuda.get_device_name(0), "results": results}))
    return 0 if all(r["roundtrip_bit_exact"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
