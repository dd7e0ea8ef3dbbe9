#!/usr/bin/env python3
"""Pack pass benchmark: the waveform of 65 536 x 4096-frame stereo MUSIC packets, device-resident float32, at 16 and at 24 bits.

Per depth and layout (STREAM, PACKETS), each the median and range of --steps runs after --warmup:
  pass        alacgpu_pcm_from_waveform_device alone, timed by its own HIP events (alacgpu_encoder_waveform_last_ms), the bytes
              it reads and writes and the GB/s from them
  encode      alacgpu_encode_device on the ready PCM (alacgpu_encoder_last_kernel_ms)
  fused       alacgpu_encode_waveform_device: the sum of its two event pairs (pass + encode kernels), and the time between
              two events recorded on the handle's stream around the whole call (fused_stream), which includes what lies
              between the pass and the encode
  torch       the composition of torch ops a caller writes without the pass (scale, round, clamp, cast, permute,
              contiguous; at 24 bits shifts, masks and three strided byte scatters as well), run on the same device, timed
              with torch events, and checked byte-equal to the pass first
Prints one JSON line; --out also writes it to a file.

--distinct packets are generated and the full-length ones among them repeated to --packets (every packet is packed and
encoded on its own, so the tiling only saves generation time)."""
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


def composition(torch, wave, depth, layout):
    """What a caller writes today: float32 [ch, T] or [n, ch, fl] -> interleaved PCM bytes (uint8, flat)."""
    q = 16 if depth == 16 else 24
    top = float(1 << (q - 1))
    v = (wave * top).round().clamp(-top, top - 1)
    if depth == 16:
        v = v.to(torch.int16)
        v = v.t().contiguous() if layout == "stream" else v.permute(0, 2, 1).contiguous()
        return v.view(torch.uint8).reshape(-1)
    v = v.to(torch.int32)
    v = v.t().contiguous() if layout == "stream" else v.permute(0, 2, 1).contiguous()
    out = torch.empty(v.shape + (3,), dtype=torch.uint8, device=wave.device)
    out[..., 0] = v & 0xFF
    out[..., 1] = (v >> 8) & 0xFF
    out[..., 2] = (v >> 16) & 0xFF
    return out.reshape(-1)


def source_wave(torch, pcm, n, fl, ch, depth):
    """PCM [n, fl * bpf] uint8 (full packets) -> float32 [ch, n * fl]: the decoder's waveform of it."""
    if depth == 16:
        v = pcm.view(torch.int16).view(n * fl, ch).to(torch.float32) * 2.0 ** -15
    else:
        b = pcm.view(n * fl, ch, 3)
        v = b[..., 0].to(torch.int32) | (b[..., 1].to(torch.int32) << 8) | (b[..., 2].to(torch.int32) << 16)
        v = ((v << 8) >> 8).to(torch.float32) * 2.0 ** -23
    return v.t().contiguous()


def spread(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), all=[round(x, 4) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=65536)
    ap.add_argument("--distinct", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--depths", default="16,24")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    synth = importlib.import_module("saprobe-alac_amd.synth")
    from oracle import oracle
    dev = torch.device("cuda:0")
    n, fl, ch = a.packets, a.frames, 2
    total = n * fl
    runs = a.warmup + a.steps
    results = []
    for depth in [int(d) for d in a.depths.split(",")]:
        ocfg = oracle.make_config(fl, depth, ch)
        cfg = pkg.PacketConfig(FrameLength=fl, BitDepth=depth, NumChannels=ch)
        bpf = ch * pkg.bytes_per_sample(depth)
        b = synth.gen_batch(ocfg, a.distinct, threads=a.threads)
        # synth's stream has a few short packets of its own; the benchmark batch is full packets only
        full = torch.from_numpy(np.nonzero(b.frames == fl)[0]).to(dev)
        pick = full[torch.arange(n, device=dev) % full.numel()]
        src = torch.from_numpy(np.ascontiguousarray(b.pcm[:, :fl * bpf])).to(dev)[pick].contiguous()
        stream_wave = source_wave(torch, src, n, fl, ch, depth)
        del src
        with pkg.NewPacketEncoder(cfg, 0) as enc:
            cap = enc.max_bytes(total)
            pcm = torch.empty(total * bpf, dtype=torch.uint8, device=dev)
            blob = torch.empty(cap, dtype=torch.uint8, device=dev)
            blob2 = torch.empty(cap, dtype=torch.uint8, device=dev)
            off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            off2 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            clip = torch.zeros(1, dtype=torch.int64, device=dev)
            ext = torch.cuda.ExternalStream(enc._lib.alacgpu_encoder_stream(enc._h), device=dev)
            for layout in ("stream", "packets"):
                if layout == "stream":
                    wave, cs, ps, lay = stream_wave, total, 0, pkg.WAVE_STREAM
                else:
                    wave = stream_wave.view(ch, n, fl).permute(1, 0, 2).contiguous()
                    cs, ps, lay = fl, ch * fl, pkg.WAVE_PACKETS
                torch.cuda.synchronize()
                pass_ms, enc_ms, fused_ms, fused_stream_ms = [], [], [], []
                for k in range(runs):
                    enc.pcm_from_waveform_device(wave.data_ptr(), lay, pkg.WAVE_FLOAT, cs, ps, total, pcm.data_ptr(), clip.data_ptr(), sync=True)
                    if k >= a.warmup:
                        pass_ms.append(enc.waveform_last_ms())
                clipped = int(clip.item())
                # the baseline, checked equal first
                comp = composition(torch, wave, depth, layout)
                equal = torch.equal(comp, pcm)
                del comp
                torch_ms = []
                for k in range(runs):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    comp = composition(torch, wave, depth, layout)
                    e1.record()
                    e1.synchronize()
                    del comp
                    if k >= a.warmup:
                        torch_ms.append(e0.elapsed_time(e1))
                torch.cuda.synchronize()
                for k in range(runs):
                    enc.encode_device(pcm.data_ptr(), total, blob.data_ptr(), cap, off.data_ptr(), sync=True)
                    if k >= a.warmup:
                        enc_ms.append(enc.last_kernel_ms())
                for k in range(runs):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(ext)
                    enc.encode_waveform_device(wave.data_ptr(), lay, pkg.WAVE_FLOAT, cs, ps, total, blob2.data_ptr(), cap, off2.data_ptr(),
                                               clip.data_ptr(), sync=False)
                    e1.record(ext)
                    enc.synchronize()
                    e1.synchronize()
                    if k >= a.warmup:
                        fused_ms.append(enc.waveform_last_ms() + enc.last_kernel_ms())
                        fused_stream_ms.append(e0.elapsed_time(e1))
                size = int(off[n].item())
                same_blob = torch.equal(off, off2) and torch.equal(blob[:size], blob2[:size])
                moved = total * ch * 4 + total * bpf  # waveform in, PCM out
                tbs = moved / (statistics.median(pass_ms) * 1e-3) / 1e12
                results.append(dict(depth=depth, layout=layout, type="float32", packets=n, frames=fl, channels=ch, clipped=clipped,
                                    pass_ms=spread(pass_ms), encode_ms=spread(enc_ms), fused_ms=spread(fused_ms),
                                    fused_stream_ms=spread(fused_stream_ms), torch_ms=spread(torch_ms), bytes_moved=moved,
                                    gb_per_s=round(tbs * 1e3, 1), fraction_of_copy_rate=round(tbs / COPY_TBS, 3),
                                    fraction_of_peak=round(tbs / PEAK_TBS, 3), equal_to_torch=bool(equal),
                                    fused_equals_encode=bool(same_blob), blob_bytes=size,
                                    faster_than_torch=bool(max(pass_ms) < min(torch_ms)),
                                    speedup_vs_torch=round(statistics.median(torch_ms) / statistics.median(pass_ms), 2),
                                    fused_minus_parts_ms=round(statistics.median(fused_stream_ms) - statistics.median(pass_ms) -
                                                               statistics.median(enc_ms), 4)))
                if layout == "packets":
                    del wave
            del pcm, blob, blob2
        del stream_wave
        torch.cuda.empty_cache()
    line = json.dumps({"tool": "encode_waveform_bench", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
                       "results": results})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["equal_to_torch"] and r["fused_equals_encode"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
