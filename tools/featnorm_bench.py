#!/usr/bin/env python3
"""Time the feature normalisation pass (FeatureNorm) against the torch ops that compute the same masked result on the same
tensors, with HIP events, median of 10 after warm-up:

    [1024, 2998, 80]  frames layout, per-utterance CMN (stat mean) with ragged lengths
    [1024, 80, 3000]  bins layout, Whisper's clamp: stat max, range 8, then (x + 4) / 4, every frame valid
    [256, 998, 128]   frames layout, CMVN (stat mean_var) with ragged lengths

and report the bytes the pass has to move (each reduction reads the valid elements once, the apply step reads them again and
writes every element) over its time, as a share of the 6.3 TB/s of HBM bandwidth that is achievable on an MI355X. One JSON line
per shape; --out FILE appends them to a file as well."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def torch_ops(torch, x, lengths, stat, layout, pad=0.0):
    """The same function in torch ops -> y"""
    fdim, bdim = (1, 2) if layout == "frames" else (2, 1)
    F = x.shape[fdim]
    if lengths is None:
        mask = None
    else:
        shape = [1, 1, 1]
        shape[fdim] = F
        mask = torch.arange(F, device=x.device).reshape(shape) < lengths.reshape(-1, 1, 1)
        n = lengths.clamp(min=1).to(torch.float32).reshape(-1, 1, 1)
    if stat == "max":
        v = x if mask is None else torch.where(mask, x, float("-inf"))
        y = (torch.maximum(x, v.amax(dim=(1, 2), keepdim=True) - 8.0) + 4.0) / 4.0
    else:
        if mask is None:
            n = float(F)
            m = x.sum(dim=fdim, keepdim=True) / n
        else:
            m = torch.where(mask, x, 0.0).sum(dim=fdim, keepdim=True) / n
        y = x - m
        if stat == "mean_var":
            d2 = y * y if mask is None else torch.where(mask, y * y, 0.0)
            y = y * torch.rsqrt((d2.sum(dim=fdim, keepdim=True) / n).clamp(min=1e-20))
    return y if mask is None else torch.where(mask, y, pad)


def median_ms(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiply the row counts (a quick look at a smaller batch)")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("saprobe-alac_amd")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    cases = [("cmn", (1024, 2998, 80), "frames", "mean", True, {}),
             ("whisper", (1024, 80, 3000), "bins", "max", False, dict(range=8.0, shift=-4.0, scale=0.25)),
             ("cmvn", (256, 998, 128), "frames", "mean_var", True, {})]
    for name, shape, layout, stat, ragged, kw in cases:
        shape = (max(1, int(shape[0] * args.scale)),) + shape[1:]
        rows = shape[0]
        F, bins = (shape[1], shape[2]) if layout == "frames" else (shape[2], shape[1])
        x = torch.randn(shape, device=dev, generator=gen) * 1.5 - 5.0
        lengths = None
        if ragged:
            lengths = torch.randint(F // 2, F + 1, (rows,), device=dev, generator=gen, dtype=torch.int32)
            lengths[0] = F
        valid = rows * F if lengths is None else int(lengths.sum())
        reductions = {"mean": 1, "mean_var": 2, "max": 1}[stat]
        moved = 4 * bins * (valid * (reductions + 1) + rows * F)
        out = torch.empty_like(x)
        with pkg.NewFeatureNorm(bins, stat, **kw) as h:
            times = []
            for k in range(args.warmup + args.reps):
                h(x, lengths, layout, out=out)
                if k >= args.warmup:
                    times.append(h.last_ms())
            ours = statistics.median(times)
            want = torch_ops(torch, x, lengths, stat, layout)
            err = float((out - want).abs().max())
            del want
        theirs = median_ms(torch, lambda: torch_ops(torch, x, lengths, stat, layout), args.reps, args.warmup)
        line = dict(case=name, shape=list(shape), layout=layout, stat=stat, ragged=ragged, valid_share=round(valid / (rows * F), 4),
                    pass_ms=round(ours, 4), torch_ms=round(theirs, 4), speedup=round(theirs / ours, 2), bytes_moved=moved,
                    tb_per_s=round(moved / ours / 1e9, 3), hbm_share=round(moved / ours / 1e9 / HBM_TBS, 3), max_abs_diff_vs_torch=err)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del x, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
