#!/usr/bin/env python3
"""Time the SpecAugment pass (SpecAugment) against the torch ops that compute the same result from the pass's own draws on the
same tensors, with HIP events, median of 10 after warm-up, one process:

    [1024, 2998, 80]  frames layout, 2 + 2 masks, no warp, in place
    [1024, 2998, 80]  frames layout, 2 + 2 masks, warp 5, out of place
    [1024, 80, 3000]  bins layout, 2 + 2 masks, no warp, out of place

Lengths are uniform in [F / 2, F]. The torch chain takes the draws as given (it draws nothing): arange comparisons and where for
the masks and the padding; for the warp a gather of the two source frames and a lerp with the pass's floored weight. The bytes the
pass has to move (the valid input elements once, every output element once, the draws) over its time are reported as a share of
the 6.3 TB/s of HBM bandwidth that is achievable on an MI355X. One JSON line per shape; --out FILE appends them to a file as
well."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def torch_ops(torch, x, lengths, draws, nf, nt, mask_value=0.0, pad_value=0.0):
    """The same function in torch ops: x [rows, F, bins], lengths int32 [rows], draws int32 [rows, P] -> y [rows, F, bins]"""
    rows, F, bins = x.shape
    n = lengths.clamp(0, F).to(torch.int64)[:, None]
    d = draws.to(torch.int64)
    t = torch.arange(F, device=x.device)[None, :]
    c, w = d[:, 0:1], d[:, 1:2]
    if bool((w > 0).any()):
        head = t < w
        a = torch.where(head, c, n - c).clamp(min=1)
        b = torch.where(head, w, n - w).clamp(min=1)
        ts = torch.where(head, t, t - w)
        num = ((2 * ts + 1) * a - b).clamp(min=0)
        i0 = torch.div(num, 2 * b, rounding_mode="floor")
        lq = torch.div((num - i0 * 2 * b) << 23, 2 * b, rounding_mode="floor")
        i1 = torch.minimum(i0 + 1, a - 1)
        base = torch.where(head, torch.zeros_like(c), c)
        warped = (w > 0) & (t < n)
        i0 = torch.where(warped, base + i0, t).clamp(0, F - 1)
        i1 = torch.where(warped, base + i1, t).clamp(0, F - 1)
        lam = torch.where(warped, lq.to(torch.float32) * 2.0 ** -23, torch.zeros((), device=x.device))
        x0 = torch.gather(x, 1, i0[:, :, None].expand(-1, -1, bins))
        x1 = torch.gather(x, 1, i1[:, :, None].expand(-1, -1, bins))
        y = torch.lerp(x0, x1, lam[:, :, None])
    else:
        y = x
    fb = torch.arange(bins, device=x.device)[None, :]
    bin_mask = torch.zeros((rows, bins), dtype=torch.bool, device=x.device)
    for i in range(nf):
        f0, fw = d[:, 2 + 2 * i, None], d[:, 3 + 2 * i, None]
        bin_mask |= (fb >= f0) & (fb < f0 + fw)
    frame_mask = torch.zeros((rows, F), dtype=torch.bool, device=x.device)
    for i in range(nt):
        t0, tw = d[:, 2 + 2 * nf + 2 * i, None], d[:, 3 + 2 * nf + 2 * i, None]
        frame_mask |= (t >= t0) & (t < t0 + tw)
    y = torch.where(bin_mask[:, None, :] | frame_mask[:, :, None], mask_value, y)
    return torch.where((t < n)[:, :, None], y, pad_value)


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
    masks = dict(freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=1.0)
    cases = [("masks_in_place", (1024, 2998, 80), "frames", dict(warp=0, **masks), True),
             ("masks_warp_5", (1024, 2998, 80), "frames", dict(warp=5, **masks), False),
             ("masks_bins_layout", (1024, 3000, 80), "bins", dict(warp=0, **masks), False)]
    for name, shape, layout, kw, in_place in cases:
        rows, F, bins = max(1, int(shape[0] * args.scale)), shape[1], shape[2]
        x = torch.randn((rows, F, bins), device=dev, generator=gen) * 1.5 - 5.0  # the logical [rows, F, bins]
        lengths = torch.randint(F // 2, F + 1, (rows,), device=dev, generator=gen, dtype=torch.int32)
        lengths[0] = F
        given = x if layout == "frames" else x.transpose(1, 2).contiguous()  # what the pass is handed: [rows, bins, F] for "bins"
        with pkg.NewSpecAugment(bins, **kw) as h:
            pl = h.plan()
            moved = 4 * (bins * int(lengths.sum()) + rows * F * bins) + 4 * rows * pl["draws"] + 4 * rows
            work = given.clone()
            out = work if in_place else torch.empty_like(given)
            times = []
            for k in range(args.warmup + args.reps):
                if in_place:
                    work.copy_(given)
                _, draws = h(work, lengths, seed=k, layout=layout, out=out, return_draws=True)
                if k >= args.warmup:
                    times.append(h.last_ms())
            ours = statistics.median(times)
        run = lambda: torch_ops(torch, x, lengths, draws, kw["freq_masks"], kw["time_masks"])  # noqa: E731
        got = out if layout == "frames" else out.transpose(1, 2)
        err = float((got - run()).abs().max())
        theirs = median_ms(torch, run, args.reps, args.warmup)
        line = dict(case=name, shape=list(given.shape), layout=layout, in_place=in_place, tile_out=pl["tile_out"], lds_bytes=pl["lds_bytes"],
                    valid_share=round(int(lengths.sum()) / (rows * F), 4), pass_ms=round(ours, 4), torch_ms=round(theirs, 4),
                    speedup=round(theirs / ours, 2), bytes_moved=moved, tb_per_s=round(moved / ours / 1e9, 3),
                    hbm_share=round(moved / ours / 1e9 / HBM_TBS, 3), max_abs_diff_vs_torch=err, **kw)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del x, given, work, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
