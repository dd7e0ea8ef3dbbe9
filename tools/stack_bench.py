#!/usr/bin/env python3
"""Time the frame stacking pass (FrameStack) against the torch ops that compute the same masked result on the same tensors, with
HIP events, median of 10 after warm-up, one process:

    [1024, 2998, 80]  LFR 7 / 6 (left 3, right 3, stride 6), ragged lengths
    [1024, 2998, 13]  add-deltas, order 2 at window 2, ragged lengths
    [256, 998, 80]    order 2 at window 2 and a splice of +-3 frames, ragged lengths

The torch chain clamps every frame index to the row's own last valid frame (a gather per tap and per context position), sums the
taps with the pass's weights, concatenates and masks the frames behind each row's count. The bytes the pass has to move (the valid
input elements once, every output element once) over its time are reported as a share of the 6.3 TB/s of HBM bandwidth that is
achievable on an MI355X. One JSON line per shape; --out FILE appends them to a file as well."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def torch_ops(torch, x, lengths, tables, order, left, right, stride, pad=0.0):
    """The same function in torch ops: x [rows, F, bins], lengths int32 [rows], tables [w_1, w_2] as lists -> y [rows, G, D]"""
    rows, F, bins = x.shape
    n = lengths.clamp(0, F).to(torch.int64)
    last = (n - 1).clamp(min=0)[:, None]

    def take(src, frames):
        """src[r, clamp(frames, 0, n_r - 1)] for frames [T] -> [rows, T, bins]"""
        idx = torch.minimum(frames[None, :].clamp(min=0), last)
        return torch.gather(src, 1, idx[:, :, None].expand(-1, -1, bins))

    t = torch.arange(F, device=x.device)
    d = [x]
    for k in range(1, order + 1):
        w = tables[k - 1]
        M = (len(w) - 1) // 2
        acc = torch.zeros_like(x)
        for i in range(-M, M + 1):
            if w[i + M] != 0.0:
                acc = acc + w[i + M] * take(x, t + i)
        d.append(acc)
    G = -(-F // stride)
    g = torch.arange(G, device=x.device) * stride
    y = torch.cat([take(dk, g + c - left) for c in range(left + right + 1) for dk in d], dim=2)
    m = torch.div(n + stride - 1, stride, rounding_mode="floor")
    return torch.where(torch.arange(G, device=x.device)[None, :, None] < m[:, None, None], y, pad)


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
    cases = [("lfr_7_6", (1024, 2998, 80), dict(order=0, window=2, left=3, right=3, stride=6)),
             ("add_deltas", (1024, 2998, 13), dict(order=2, window=2, left=0, right=0, stride=1)),
             ("deltas_splice_3", (256, 998, 80), dict(order=2, window=2, left=3, right=3, stride=1))]
    for name, shape, kw in cases:
        rows, F, bins = max(1, int(shape[0] * args.scale)), shape[1], shape[2]
        x = torch.randn((rows, F, bins), device=dev, generator=gen) * 1.5 - 5.0
        lengths = torch.randint(F // 2, F + 1, (rows,), device=dev, generator=gen, dtype=torch.int32)
        lengths[0] = F
        with pkg.NewFrameStack(bins, **kw) as h:
            pl = h.plan()
            G, D = h.out_frames(F), pl["columns"]
            moved = 4 * (bins * int(lengths.sum()) + rows * G * D) + 8 * rows
            out = torch.empty((rows, G, D), device=dev)
            times = []
            for k in range(args.warmup + args.reps):
                h(x, lengths, out=out)
                if k >= args.warmup:
                    times.append(h.last_ms())
            ours = statistics.median(times)
            tables = [[float(v) for v in pl[key]] for key in ("w1", "w2") if pl[key] is not None]
        run = lambda: torch_ops(torch, x, lengths, tables, kw["order"], kw["left"], kw["right"], kw["stride"])  # noqa: E731
        err = float((out - run()).abs().max())
        theirs = median_ms(torch, run, args.reps, args.warmup)
        line = dict(case=name, shape=[rows, F, bins], out_shape=[rows, G, D], tile_out=pl["tile_out"], lds_bytes=pl["lds_bytes"],
                    valid_share=round(int(lengths.sum()) / (rows * F), 4), pass_ms=round(ours, 4), torch_ms=round(theirs, 4),
                    speedup=round(theirs / ours, 2), bytes_moved=moved, tb_per_s=round(moved / ours / 1e9, 3),
                    hbm_share=round(moved / ours / 1e9 / HBM_TBS, 3), max_abs_diff_vs_torch=err, **kw)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del x, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
