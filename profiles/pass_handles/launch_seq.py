#!/usr/bin/env python3
"""One pass of 3 rows on each of the four row-pass handles, T chosen from plan() so that every row spans two tiles:

    ALACGPU_LIB=<library> rocprofv3 --kernel-trace --output-format csv -d DIR -o out -- python3 profiles/pass_handles/launch_seq.py
    python3 profiles/pass_handles/launch_seq.py --reduce DIR/.../out_kernel_trace.csv > <name>.txt

--reduce prints the library's kernels (alac_*) of such a trace in dispatch order: name, grid, workgroup, static LDS."""
import csv
import importlib
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = 3


def passes():
    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    dev = torch.device("cuda:0")
    mel = dict(n_fft=16, hop_length=4, n_mels=4)
    for name, new, length in (
            ("resampler", lambda: pkg.NewResampler(2, 3), lambda p: p["tile_out"]),  # 1.5 tile_out columns
            ("mel", lambda: pkg.NewMelSpectrogram(16000, **mel), lambda p: 4 * (p["tile_frames"] + 1)),  # tile_frames + 2 frames
            ("mel_fft", lambda: pkg.NewMelSpectrogram(16000, transform="fft", **mel), lambda p: 4 * (p["tile_frames"] + 1)),
            ("kaldi", lambda: pkg.NewKaldiFeatures(16000, 16, 4, num_mel_bins=4, low_freq=20.0),
             lambda p: 16 + 4 * p["tile_frames"])):  # tile_frames + 1 frames
        with new() as h:
            plan = h.plan()
            T = length(plan)
            tile = plan.get("tile_out") or plan["tile_frames"]
            frames = h.out_frames(T)
            assert tile < frames <= 2 * tile, (name, T, frames, tile)
            out = h(torch.zeros((ROWS, T), dtype=torch.float32, device=dev))
            print("%s: T %d, %d frames in tiles of %d, out %s, %.4f ms" % (name, T, frames, tile, tuple(out.shape), h.last_ms()))


def reduce(path):
    name = re.compile(r"(?:^|::|\s)(alac_\w+)")  # the trace demangles: "(anonymous namespace)::alac_mel_rows(alacmel::Params, ...)"
    rows = [r for r in csv.DictReader(open(path)) if name.search(r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        print("%-22s grid %s x %s x %s  wg %s x %s x %s  lds %s" % (
            name.search(r["Kernel_Name"]).group(1), r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"],
            r["Workgroup_Size_Y"], r["Workgroup_Size_Z"], r["LDS_Block_Size"]))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--reduce":
        reduce(sys.argv[2])
    else:
        passes()
