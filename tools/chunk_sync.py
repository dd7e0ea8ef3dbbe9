#!/usr/bin/env python3
"""chunk_sync.py — where the waves of the ungated four-wave workgroups wait: reads back what a build with -DALAC_SYNC_DIAG
(csrc/alac_gpu.h: kClaimDw; `make EXTRA=-DALAC_SYNC_DIAG`) leaves in the wave slots' records after one decode, and prints, per
key group (taps of the longer predictor), role and phase: the share of the slot's cycles spent inside duo_sync, the cycles
per chunk barrier, and how often the role was the last to arrive. The diagnostic build times waves and perturbs them (it is
about twice as slow): the table is a ranking, and for nothing but that.

    python tools/chunk_sync.py [--packets 65536 --depth 16 --channels 2] diag_lib.so"""
import argparse
import collections
import ctypes
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DW = 16  # kClaimDw of the diagnostic build
ROLES = ("entropy", "predictor", "writer")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib")
    ap.add_argument("--packets", type=int, default=65536)
    ap.add_argument("--depth", type=int, default=16)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--frame-length", type=int, default=4096)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--warm", type=int, default=6, help="decodes before the one that is looked at")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    synth = importlib.import_module("saprobe-alac_amd.synth")
    synth.build()
    P, FL, ch = args.packets, args.frame_length, args.channels
    cfg = pkg.PacketConfig(FrameLength=FL, BitDepth=args.depth, NumChannels=ch)
    stride = FL * ch * pkg.bytes_per_sample(args.depth)
    b = synth.gen_batch(cfg, P, profile=args.profile, threads=min(os.cpu_count() or 1, 32))
    dev = torch.device("cuda:0")
    d_blob = torch.from_numpy(b.blob).to(dev)
    d_off = torch.from_numpy(b.offsets.astype(np.int64)).to(dev)
    d_sz = torch.from_numpy(b.sizes.astype(np.int32)).to(dev)
    d_out = torch.zeros((P, stride), dtype=torch.uint8, device=dev)
    d_fr = torch.zeros(P, dtype=torch.int32, device=dev)
    d_st = torch.full((P,), -1, dtype=torch.int32, device=dev)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L = ctypes.CDLL(os.path.abspath(args.lib))
    L.alacgpu_create.argtypes = [ctypes.POINTER(pkg.PacketConfig), ctypes.c_int, ctypes.POINTER(vp)]
    L.alacgpu_decode_batch_device.argtypes = [vp, vp, sz, vp, vp, sz, vp, sz, vp, vp, ctypes.c_int]
    L.alacgpu_pair_placement.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    L.alacgpu_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.alacgpu_destroy.argtypes = [vp]
    h = vp()
    assert L.alacgpu_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
    for _ in range(args.warm):
        assert L.alacgpu_decode_batch_device(h, d_blob.data_ptr(), d_blob.numel(), d_off.data_ptr(), d_sz.data_ptr(), P,
                                             d_out.data_ptr(), stride, d_fr.data_ptr(), d_st.data_ptr(), 1) == 0
    ms = ctypes.c_float()
    L.alacgpu_last_kernel_ms(h, ctypes.byref(ms))
    raw = np.zeros(DW * (P // 8 + 4096), np.uint32)
    got = sz()
    assert L.alacgpu_pair_placement(h, raw.ctypes.data, raw.size, ctypes.byref(got)) == 0
    L.alacgpu_destroy(h)
    rec = raw[:DW * got.value].reshape(-1, DW).astype(np.int64)
    rec = rec[rec[:, 14] != 0]  # slots a four-wave workgroup of the diagnostic build decoded
    assert int(d_st.abs().sum()) == 0
    print("decode %.3f ms (diagnostic build: timed waves); %d wave slots with a record of %d" % (ms.value, len(rec), got.value))
    if not len(rec):
        print("no records: is the library built with -DALAC_SYNC_DIAG, and the batch one for the ungated four-wave kernel?")
        return
    key = rec[:, 15]
    taps = np.maximum((key >> 5) & 31, key & 31)
    groups = collections.OrderedDict()
    for t in sorted(set(taps.tolist())):
        groups["%d taps" % t] = taps == t
    groups["all"] = np.ones(len(rec), bool)
    print("%-9s %5s %-9s %-5s %9s %12s %9s" % ("key", "slots", "role", "phase", "wait/slot", "cycles/chunk", "last"))
    for name, m in groups.items():
        r = rec[m]
        total = r[:, 14].astype(np.float64)  # the entropy wave's cycles in the slot
        for role in range(3):
            for ph in range(2):
                wait, last = r[:, 4 * role + 2 * ph].astype(np.float64), r[:, 4 * role + 2 * ph + 1].astype(np.float64)
                if ph == 0 and ch != 2:
                    continue
                # every wave of a workgroup passes the same barriers: their number is the sum of the roles' "last" counts
                bars = sum(r[:, 4 * q + 2 * ph + 1] for q in range(3)).astype(np.float64)
                bars = np.maximum(bars, 1.0)
                print("%-9s %5d %-9s %-5s %8.1f%% %12.0f %8.1f%%" % (name, len(r), ROLES[role], "UV"[ph], 100.0 * (wait / total).mean(),
                                                                (wait / bars).mean(), 100.0 * (last / bars).mean()))
    print("(wait/slot: share of the slot's cycles the wave spent inside duo_sync; cycles/chunk: the same per barrier; last: share of"
          " the barriers at which the wave arrived last; s_memtime ticks)")


if __name__ == "__main__":
    main()
