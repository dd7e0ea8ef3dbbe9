#!/usr/bin/env python3
"""Time the waveform augmentation pass (WaveAugment) against the torch ops that compute the same masked result from the pass's own
draws on the same tensors, with HIP events, median of 10 after 3 warm-ups, one process:

    [1024, 480000]  lengths uniform in [T / 2, T], a bank of 64 x 160000, SNR 5..20 dB, gain -6..3 dB, without and with dither
    [256, 160000]   the same

The torch chain takes the draws as given (it draws nothing): a masked sum of squares of x, a modular gather out of the flat bank
(no copy of a row's clip), a masked sum of squares of the segment, pow and sqrt for the two scalars, two broadcasts and a where. It
has no dither, so the dither cases are compared with the same chain: what dither costs is the difference between the pass's own two
times. The bytes the pass has to move (the valid input samples twice, the noise segment twice where it is applied, every output
sample once) over its time are reported as a share of the 6.3 TB/s of HBM bandwidth that is achievable on an MI355X. One JSON line
per case; --out FILE appends them to a file as well."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3


def torch_ops(torch, x, lengths, draws, bank, bank_lengths, pad_value=0.0):
    """The same function in torch ops: x [rows, T], lengths int32 [rows], draws int32 [rows, 5] -> y [rows, T]"""
    rows, T = x.shape
    n = lengths.clamp(0, T).to(torch.int64)[:, None]
    t = torch.arange(T, device=x.device)[None, :]
    valid = t < n
    d = draws.to(torch.int64)
    ex = torch.where(valid, x, 0.0).square().sum(1)
    k, o = d[:, 1], d[:, 2]
    m = bank_lengths.to(torch.int64)[k].clamp(min=1)
    z = torch.take(bank, k[:, None] * bank.shape[1] + (o[:, None] + t) % m[:, None])  # no copy of the rows' clips
    en = torch.where(valid, z, 0.0).square().sum(1)
    a = torch.pow(10.0, d[:, 4].to(torch.float32) / 5120.0)
    b = torch.where(d[:, 0] > 0, torch.sqrt(ex / en) * torch.pow(10.0, -d[:, 3].to(torch.float32) / 5120.0) * a, 0.0)
    return torch.where(valid, a[:, None] * x + b[:, None] * z, pad_value)


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
    bank = torch.randn((64, 160000), device=dev, generator=gen) * 0.05
    bank_lengths = torch.randint(80000, 160001, (64,), device=dev, generator=gen, dtype=torch.int32)
    for shape in ((1024, 480000), (256, 160000)):
        rows, T = max(1, int(shape[0] * args.scale)), shape[1]
        x = torch.randn((rows, T), device=dev, generator=gen) * 0.1
        lengths = torch.randint(T // 2, T + 1, (rows,), device=dev, generator=gen, dtype=torch.int32)
        lengths[0] = T
        out = torch.empty_like(x)
        theirs = None
        for dither in (0.0, 1e-5):
            kw = dict(snr=(5, 20), gain=(-6, 3), noise_prob=0.8, dither=dither)
            with pkg.NewWaveAugment(**kw) as h:
                pl = h.plan()
                times = []
                for k in range(args.warmup + args.reps):
                    _, draws, stats = h(x, lengths, seed=k, noise=bank, noise_lengths=bank_lengths, out=out, return_draws=True,
                                        return_stats=True)
                    if k >= args.warmup:
                        times.append(h.last_ms())
                ours = statistics.median(times)
            applied = draws[:, 0] > 0
            moved = 4 * (2 * int(lengths.sum()) + 2 * int(lengths[applied].sum()) + rows * T)
            run = lambda: torch_ops(torch, x, lengths, draws, bank, bank_lengths)  # noqa: E731
            err = float((out - run()).abs().max()) if dither == 0.0 else None
            if theirs is None:
                theirs = median_ms(torch, run, args.reps, args.warmup)
            line = dict(case="noise_gain" + ("_dither" if dither else ""), shape=[rows, T], bank=list(bank.shape), tile=pl["tile"],
                        lds_bytes=pl["lds_bytes"], valid_share=round(int(lengths.sum()) / (rows * T), 4),
                        applied_share=round(float(applied.float().mean()), 4), pass_ms=round(ours, 4), torch_ms=round(theirs, 4),
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
