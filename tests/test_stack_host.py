"""The frame stacking pass on the CPU: csrc/alac_stack.h built with g++, contraction off (tests/host_sim/stack_sim.cpp),
workgroup for workgroup and work item for work item what the gfx950 kernel of k_stack.hip runs, against tests/stack_ref.py's numpy
restatement bit for bit, against restatements of its sources (Kaldi's ComputeDeltas, conv1d over a replicate pad, FunASR's
apply_lfr, splice-feats and subsample-feats by index lists) and against float64 within a bound computed from the data.

* every parameter set of sr.PARAMS at the bins 1, 23, 80, 129, the frames 1, tile_in - 1, tile_in, tile_in + 1 and 2 * tile_in +
  3 of the plan's own input span, six rows with the lengths 0, 1, a middle value, frames, -5 and frames + 7, both layouts in and
  both out, which give the same bits; a row alone gives what it gives in the batch. (1, 8, 16, 16, 64) has 66 columns per bin: at
  80 and 129 bins it is more than 4096 columns, which create refuses, and that refusal is what is checked there. One more set,
  order 2 at window 8 over 700 bins, is the one whose bins go through the tile in slabs; and at the wide bins 193, 257, 513, 1025
  and 4096 (sr.WIDE_BINS) every set that create takes there, with nothing cut: at 4096 bins the plain copy alone remains;
* rows and lines padded apart, every base offset, NaN and Inf in all padding and gaps, canaries around and between everything
  written;
* the plan, the weight tables, what is refused (by the host build, by the library before any HIP call, by the Python class and by
  the C++ mirror), the structs' sizes, the stand-alone program that the sanitizer run uses, the new names."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import host_build
from tests import stack_ref as sr

F32 = np.float32
ROWS = 6
CANARY = F32(-12345.5)
SLABS = (2, 8, 0, 0, 1)  # at 700 bins: tile_bins 44
CASES = [(ps, bins) for ps in sr.PARAMS for bins in sr.BINS] + [(SLABS, 700)]
# the wide bins: every parameter set that create takes there (at most 4096 columns); at 4096 bins that is the plain copy alone
WIDE = [(ps, bins) for bins in sr.WIDE_BINS for ps in sr.PARAMS if sr.accepted(ps, bins)]
IDS = ["%s-%d" % (sr.param_id(ps), bins) for ps, bins in CASES]
WIDE_IDS = ["%s-%d" % (sr.param_id(ps), bins) for ps, bins in WIDE]


@pytest.fixture(scope="module")
def sim():
    return sr.build_stack_sim()


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------
def test_plan_of_every_case_and_of_lfr_at_every_bin_count(sim):
    """tile_out in [1, 64], the largest whose images fit; tile_in its input span; the LDS within 25 600 bytes; all bins in one slab
    wherever one output frame's images fit"""
    cases = [c for c in CASES if sr.accepted(*c)] + WIDE + [((0, 2, 3, 3, 6), bins) for bins in range(1, 301)]
    cases += [((2, 8, 16, 16, 1), 41), ((2, 8, 0, 0, 1), 1365), ((0, 1, 0, 0, 64), 4096), ((1, 8, 0, 0, 1), 2048)]
    for ps, bins in cases:
        order, window, left, right, stride = ps
        rc, pl, _ = sr.sim_plan(sim, ps, bins)
        assert rc == 0 and pl == sr.plan_of(ps, bins), (ps, bins, pl)
        K, C, M = order + 1, left + right + 1, order * window
        T, tb = pl["tile_out"], pl["tile_bins"]
        assert 1 <= T <= 64 and 1 <= tb <= bins and pl["columns"] == C * K * bins <= 4096
        assert pl["tile_in"] == (T - 1) * stride + C + 2 * M
        assert pl["lds_bytes"] == 4 * ((K * tb * (pl["tile_in"] | 1) + 3) & ~3) <= 25600
        assert T == 64 or 4 * K * tb * ((pl["tile_in"] + stride) | 1) > 25600, "a larger tile would fit"
        assert (tb == bins) == (4 * K * bins * ((C + 2 * M) | 1) <= 25600)
    assert sr.plan_of((0, 2, 3, 3, 6), 80)["tile_out"] == 13 and sr.plan_of(SLABS, 700)["tile_bins"] == 44


def test_weight_tables_are_exact(sim):
    """1/10 [-2 .. 2] for window 2 at order 1, the 9 taps [4, 4, 1, -4, -10, -4, 1, 4, 4] / 100 at order 2; every table of every
    window the integer numerators over (sum j^2)^k rounded once; each table sums to 0 and is odd (order 1) or even (order 2)"""
    _, _, (w1, w2) = sr.sim_plan(sim, (2, 2, 0, 0, 1), 13)
    assert sr.same_bits(w1, (np.array([-2, -1, 0, 1, 2], np.float64) / 10).astype(F32))
    assert sr.same_bits(w2, (np.array([4, 4, 1, -4, -10, -4, 1, 4, 4], np.float64) / 100).astype(F32))
    assert sr.numerators(2, 2) == ([[-2, -1, 0, 1, 2], [4, 4, 1, -4, -10, -4, 1, 4, 4]], 10)
    from fractions import Fraction
    for window in range(1, 9):
        tabs, norm = sr.numerators(2, window)
        rc, pl, got = sr.sim_plan(sim, (2, window, 0, 0, 1), 1)
        assert rc == 0 and (pl["w1_entries"], pl["w2_entries"]) == (2 * window + 1, 4 * window + 1)
        for k, (t, g) in enumerate(zip(tabs, got), 1):
            assert sum(t) == 0 and t == [(-1) ** k * v for v in reversed(t)]
            want = np.array([F32(float(Fraction(v, norm ** k))) for v in t], F32)  # float(Fraction) rounds once, float32 of it again:
            assert sr.same_bits(g, want) and sr.same_bits(g, sr.weights(2, window)[k - 1])  # harmless here (alac_stack.h)
    _, pl, got = sr.sim_plan(sim, (0, 2, 0, 0, 1), 13)
    assert pl["w1_entries"] == pl["w2_entries"] == 0


# ---- 2. bit for bit against the numpy restatement, both layouts in and out -----------------------------------------------
@pytest.mark.parametrize("ps,bins", CASES + WIDE, ids=IDS + WIDE_IDS)
def test_bits_against_the_reference(sim, ps, bins):
    """The yardstick of tests/test_gpu_stack.py: the host build's output and out lengths are numpy's, at the wide bins too, with the
    plan's own frame counts, both layouts in and out and the same six lengths; nothing is cut there"""
    if not sr.accepted(ps, bins):
        assert sr.columns_of(ps, bins) > 4096 and sr.sim_plan(sim, ps, bins)[0] == -2
        x, y = np.zeros(bins, F32), np.full(sr.columns_of(ps, bins), CANARY, F32)
        assert sr.host_run(sim, ps, bins, x.ctypes.data, (bins, bins, 1), 1, 1, None, y.ctypes.data, (y.size, y.size, 1)) == -2
        assert (y == CANARY).all()
        return
    rng = np.random.default_rng(1000 + bins)
    for frames in sr.frames_of(ps, bins):
        x = sr.features(rng, ROWS, frames, bins)
        lengths = sr.lengths_of(frames)
        want, want_len = sr.reference(x, lengths, ps, pad=-3.5)
        for in_layout in ("frames", "bins"):
            for out_layout in ("frames", "bins"):
                y, out_len = sr.host_values(sim, x, lengths, ps, in_layout, out_layout, pad=-3.5)
                assert sr.same_bits(y, want), "%d frames, %s -> %s" % (frames, in_layout, out_layout)
                assert np.array_equal(out_len, want_len)
        # a row's result does not depend on the rows around it
        alone, alone_len = sr.host_values(sim, x[2:3], lengths[2:3], ps, pad=-3.5)
        assert sr.same_bits(alone[0], want[2]) and alone_len[0] == want_len[2]
        # no lengths: every frame is valid
        full, full_len = sr.host_values(sim, x[:2], None, ps, "bins", "frames")
        assert sr.same_bits(full, sr.reference(x[:2], None, ps)[0]) and (full_len == -(-frames // ps[4])).all()


# ---- 3. against the sources' own definitions -----------------------------------------------------------------------------
def kaldi_compute_deltas(feats, order, window):
    """Kaldi's DeltaFeatures (feature-functions.cc): the scales by its loops, Process frame by frame, in float64
    -> [n, (order + 1) * bins]"""
    scales = [np.array([1.0])]
    for i in range(1, order + 1):
        prev = scales[i - 1]
        prev_offset = (len(prev) - 1) // 2
        cur_offset = prev_offset + window
        cur = np.zeros(len(prev) + 2 * window)
        normalizer = 0.0
        for j in range(-window, window + 1):
            normalizer += j * j
            for k in range(-prev_offset, prev_offset + 1):
                cur[j + k + cur_offset] += j * prev[k + prev_offset]
        scales.append(cur * (1.0 / normalizer))
    n, dim = feats.shape
    out = np.zeros((n, dim * (order + 1)))
    for frame in range(n):
        for i in range(order + 1):
            max_offset = (len(scales[i]) - 1) // 2
            row = out[frame, i * dim:(i + 1) * dim]
            for j in range(-max_offset, max_offset + 1):
                offset_frame = min(max(frame + j, 0), n - 1)
                scale = scales[i][j + max_offset]
                if scale != 0.0:
                    row += scale * feats[offset_frame]
    return out


def apply_lfr(inputs, lfr_m, lfr_n):
    """FunASR's apply_lfr (wav_frontend.py), literally"""
    LFR_inputs = []
    T = inputs.shape[0]
    T_lfr = int(np.ceil(T / lfr_n))
    left_padding = np.tile(inputs[0], ((lfr_m - 1) // 2, 1))
    inputs = np.vstack((left_padding, inputs))
    T = T + (lfr_m - 1) // 2
    for i in range(T_lfr):
        if lfr_m <= T - i * lfr_n:
            LFR_inputs.append((inputs[i * lfr_n:i * lfr_n + lfr_m]).reshape(1, -1))
        else:
            num_padding = lfr_m - (T - i * lfr_n)
            frame = inputs[i * lfr_n:].reshape(-1)
            for _ in range(num_padding):
                frame = np.hstack((frame, inputs[-1]))
            LFR_inputs.append(frame)
    return np.vstack(LFR_inputs).astype(np.float32)


def within_the_bound(y, v, ps, other64=None):
    """|y - y64| <= gamma(taps + 1) sum|w_i||x_i| + 2^-24 sum|w_i||x_i| per element of a row's valid output (the chain's roundings and
    the weights'), the float64 reference's own roundings added; order 0 columns have a bound of 0: they are copies -> the largest
    fraction of the bound"""
    y64, mag, taps = sr.reference64(v, ps)
    lim = (sr.gamma(taps + 1) + sr.U + (taps + 2) * 2.0 ** -53) * mag
    err = np.abs(y.astype(np.float64) - y64)
    assert (err <= lim).all(), (ps, float((err / np.maximum(lim, 1e-300)).max()))
    if other64 is not None:  # another float64 evaluation of the same sums: it differs from ours by float64 roundings only
        assert (np.abs(other64 - y64) <= (2 * taps + 8) * 2.0 ** -53 * mag).all()
    return float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0


@pytest.mark.parametrize("bins", sr.BINS + sr.WIDE_BINS[:-1])
def test_deltas_against_kaldi_conv1d_and_float64(sim, bins):
    """The bound is the same at every bin count. 4096 bins are left out: no parameter set with deltas has at most 4096 columns there"""
    import torch
    rng = np.random.default_rng(2000 + bins)
    worst = 0.0
    for ps in [p for p in sr.PARAMS + ((2, 8, 0, 0, 1), (1, 4, 0, 0, 1)) if p[0] > 0 and sr.accepted(p, bins)]:
        order, window = ps[:2]
        frames = sr.plan_of(ps, bins)["tile_in"] + 1
        x = sr.features(rng, ROWS, frames, bins)
        lengths = sr.lengths_of(frames)
        y, _ = sr.host_values(sim, x, lengths, ps)
        for r, n in enumerate(sr.clamp_lengths(lengths, ROWS, frames)):
            if n == 0:
                continue
            v = x[r, :n]  # each row cut to its own length first
            m = -(-n // ps[4])
            other = None
            if ps[2:] == (0, 0, 1):
                other = kaldi_compute_deltas(v.astype(np.float64), order, window)
                assert sr.same_bits(y[r, :n, :bins], v), "d_0 is a copy"
                if order == 1 and n > 1:  # torchaudio's compute_deltas, mode replicate: conv1d of the ramp over the padded row, / sum j^2
                    t = torch.from_numpy(v.astype(np.float64).T.copy())[:, None]  # [bins, 1, n]
                    t = torch.nn.functional.pad(t, (window, window), mode="replicate")
                    kern = torch.arange(-window, window + 1, dtype=torch.float64)[None, None]
                    conv = torch.nn.functional.conv1d(t, kern)[:, 0] / (window * (window + 1) * (2 * window + 1) / 3)
                    assert np.allclose(conv.numpy().T, other[:, bins:], rtol=0, atol=1e-12)
            worst = max(worst, within_the_bound(y[r, :m], v, ps, other))
    print("bins %d: largest error / bound %.3f" % (bins, worst))


@pytest.mark.parametrize("bins", sr.BINS)
def test_order_0_is_lfr_splice_and_subsample_bit_for_bit(sim, bins):
    rng = np.random.default_rng(3000 + bins)
    frames = 100
    x = sr.features(rng, ROWS, frames, bins)
    lengths = sr.lengths_of(frames)
    ns = sr.clamp_lengths(lengths, ROWS, frames)
    for m, n in ((7, 6), (1, 1), (5, 3), (4, 4), (2, 7), (11, 2)):
        left = (m - 1) // 2
        y, out_len = sr.host_values(sim, x, lengths, (0, 0, left, m - 1 - left, n))
        for r, nr in enumerate(ns):
            assert out_len[r] == -(-nr // n)
            if nr:
                assert sr.same_bits(y[r, :out_len[r]], apply_lfr(x[r, :nr], m, n)), "apply_lfr(%d, %d), row %d" % (m, n, r)
            assert not y[r, out_len[r]:].view(np.uint32).any()
    for left, right in ((3, 3), (0, 4), (5, 0), (16, 16)):  # splice-feats: frame t is the frames t - left .. t + right, clamped
        y, out_len = sr.host_values(sim, x[:, :, :min(bins, 100)], lengths, (0, 0, left, right, 1))
        for r, nr in enumerate(ns):
            want = np.concatenate([x[r, [min(max(t + c, 0), nr - 1) for t in range(nr)], :min(bins, 100)]
                                   for c in range(-left, right + 1)], axis=1) if nr else np.zeros((0, 0), F32)
            assert out_len[r] == nr and (nr == 0 or sr.same_bits(y[r, :nr], want))
    for n in (1, 2, 3, 10, 64):  # subsample-feats: the frames 0, n, 2 n, ...
        y, out_len = sr.host_values(sim, x, lengths, (0, 0, 0, 0, n))
        for r, nr in enumerate(ns):
            assert out_len[r] == len(range(0, nr, n)) and sr.same_bits(y[r, :out_len[r]], x[r, list(range(0, nr, n))])


# ---- 4. strides, gaps, canaries, non-finite padding ----------------------------------------------------------------------
def run_over_buffers(sim, x, lengths, ps, in_layout, out_layout, row_gap, inner_gap, lead, poison, pad):
    """x laid out with gaps -> asserts the output, and that nothing but the output's elements and the lengths changed"""
    rows, frames, bins = x.shape
    G, D = -(-frames // ps[4]), sr.columns_of(ps, bins)
    xin = x.copy()
    if poison is not None:
        for r, n in enumerate(sr.clamp_lengths(lengths, rows, frames)):
            xin[r, n:] = poison
    buf, view, st = sr.lay_out(xin, in_layout, row_gap, inner_gap, lead, fill=CANARY if poison is None else poison)
    olead = (lead + 1) % 4
    obuf, oview, ost = sr.lay_out(np.zeros((rows, G, D), F32), out_layout, row_gap + 1, inner_gap + 2, olead, fill=CANARY)
    before = buf.copy()
    out_len = np.full(rows + 2, -77, np.int32)
    rc = sr.host_run(sim, ps, bins, view.ctypes.data, st, rows, frames, lengths, oview.ctypes.data, ost, out_len[1:], pad)
    assert rc == 0
    rest = sr.outside(obuf, lambda b: sr.view_like(b, olead, (rows, G, D), ost))
    assert rest.size and (rest.view(np.uint32) == CANARY.view(np.uint32)).all(), "an element outside the output was written"
    assert np.array_equal(buf.view(np.uint32), before.view(np.uint32)), "the input changed"
    want, want_len = sr.reference(x, lengths, ps, pad)
    assert sr.same_bits(oview, want)
    assert out_len[0] == out_len[-1] == -77 and np.array_equal(out_len[1:-1], want_len), "exactly rows lengths are written"


@pytest.mark.parametrize("ps,bins", [c for c in CASES if sr.accepted(*c) and c[1] != 129 or c[0] == (2, 2, 3, 3, 6)],
                         ids=[i for c, i in zip(CASES, IDS) if sr.accepted(*c) and c[1] != 129 or c[0] == (2, 2, 3, 3, 6)])
def test_gaps_offsets_and_poisoned_padding(sim, ps, bins):
    """Rows a row_gap apart and lines an inner_gap apart at the four base offsets, either layout in and either out, the padded
    frames and every gap of the input NaN or Inf: the result is the clean input's, and nothing around or between is written"""
    rng = np.random.default_rng(4000 + bins)
    frames = sr.plan_of(ps, bins)["tile_in"] + 3
    x = sr.features(rng, ROWS, frames, bins)
    lengths = sr.lengths_of(frames)
    k = 0
    for in_layout in ("frames", "bins"):
        for out_layout in ("frames", "bins"):
            for lead in range(4):
                poison = (F32(np.nan), F32(np.inf), F32(-np.inf), None)[k % 4]
                k += 1
                run_over_buffers(sim, x, lengths, ps, in_layout, out_layout, row_gap=(0, 5, 1, 7)[lead], inner_gap=(0, 3, 1, 2)[lead],
                                 lead=lead, poison=poison, pad=-1.0)


def test_one_frame_and_one_bin_take_either_stride(sim):
    """The stride of an axis of one element is free, in and out"""
    rng = np.random.default_rng(5)
    x = sr.features(rng, 3, 70, 1)
    ps = (1, 2, 0, 0, 1)
    want, _ = sr.reference(x, [70, 3, 0], ps)
    for st in ((70, 1, 1), (70, 1, 70), (70, 1, 99)):
        flat, out = np.ascontiguousarray(x.reshape(-1)), np.zeros(3 * 70 * 2, F32)
        assert sr.host_run(sim, ps, 1, flat.ctypes.data, st, 3, 70, [70, 3, 0], out.ctypes.data, (140, 2, 1)) == 0
        assert sr.same_bits(out.reshape(3, 70, 2), want)
    x = sr.features(rng, 3, 1, 23)
    ps = (0, 0, 2, 2, 5)
    want, _ = sr.reference(x, [1, 0, 1], ps, pad=9.0)
    for st in ((23, 1, 1), (23, 23, 1), (23, 5, 1)):
        for ost in ((115, 115, 1), (115, 1, 1), (115, 7, 1)):  # G = 1: the output's frame stride is free too
            flat, out = np.ascontiguousarray(x.reshape(-1)), np.zeros(3 * 115, F32)
            assert sr.host_run(sim, ps, 23, flat.ctypes.data, st, 3, 1, [1, 0, 1], out.ctypes.data, ost, pad=9.0) == 0
            assert sr.same_bits(out.reshape(3, 1, 115), want)


# ---- 5. what is refused --------------------------------------------------------------------------------------------------
def test_refusals_of_the_host_build(sim):
    x = np.zeros(4 * 10 * 8 + 64, F32)
    out = np.full(4 * 10 * 24 + 64, CANARY, F32)

    def run(ps=(0, 2, 1, 1, 1), strides=(80, 8, 1), ostrides=(240, 24, 1), rows=4, frames=10, bins=8, inp=x.ctypes.data,
            outp=out.ctypes.data):
        return sr.host_run(sim, ps, bins, inp, strides, rows, frames, None, outp, ostrides)

    assert run() == 0 and sr.columns_of((0, 2, 1, 1, 1), 8) == 24
    for bad in (dict(bins=0), dict(bins=4097), dict(ps=(3, 2, 0, 0, 1)), dict(ps=(1, 0, 0, 0, 1)), dict(ps=(1, 9, 0, 0, 1)),
                dict(ps=(2, 9, 0, 0, 1)), dict(ps=(0, 2, 17, 0, 1)), dict(ps=(0, 2, 0, 17, 1)), dict(ps=(0, 2, 1, 1, 0)),
                dict(ps=(0, 2, 1, 1, 65)), dict(ps=(0, 2, 1, 1, 2 ** 32 - 1)), dict(ps=(2 ** 32 - 1, 2, 1, 1, 1)),
                dict(ps=(0, 2, 0, 0, 1), bins=4097), dict(ps=(0, 2, 0, 1, 1), bins=2049), dict(ps=(2, 2, 16, 16, 1), bins=42),
                dict(inp=None), dict(outp=None), dict(inp=x.ctypes.data + 2), dict(outp=out.ctypes.data + 1),
                dict(strides=(80, 8, 2)), dict(ostrides=(480, 48, 2)), dict(strides=(79, 8, 1)), dict(ostrides=(239, 24, 1)),
                dict(strides=(80, 7, 1)), dict(ostrides=(240, 23, 1)), dict(strides=(80, 1, 9)), dict(ostrides=(240, 1, 9)),
                dict(strides=(2 ** 62, 8, 1)), dict(frames=2 ** 31, strides=(2 ** 34, 8, 1), ostrides=(2 ** 36, 24, 1)),
                # the output on the input, behind its start, and ending inside it: there is no in place
                dict(outp=x.ctypes.data), dict(outp=x.ctypes.data + 4 * 100), dict(inp=out.ctypes.data + 4 * 900),
                dict(inp=out.ctypes.data + 4 * 23, rows=1, frames=1, strides=(8, 8, 1))):
        out[...] = CANARY
        assert run(**bad) == -2, bad
        assert (out == CANARY).all() and not x.any()
    assert run(ps=(0, 0, 1, 1, 1)) == 0 and run(ps=(0, 99, 1, 1, 1)) == 0, "window is read with an order above 0 only"
    assert run(inp=out.ctypes.data + 4 * 24, rows=1, frames=1, strides=(8, 8, 1), ostrides=(24, 24, 1)) == 0, "end to end is apart"
    out[...] = CANARY
    x[...] = 0
    assert run(rows=0) == 0 and run(frames=0) == 0 and run(rows=0, inp=None, outp=None) == 0 and (out == CANARY).all()


def test_refusals_of_the_library_and_its_mirrors(pkg):
    """alacgpu_stack_create refuses before any HIP call (this runs without a GPU), and so do the Python class, the functional
    entries and the C++ mirror; a NULL handle is refused by every entry"""
    pkg.build()
    L = pkg.lib()
    h = ctypes.c_void_p()
    for cfg in ((0, 0, 2, 0, 0, 1), (4097, 0, 2, 0, 0, 1), (80, 3, 2, 0, 0, 1), (80, 1, 0, 0, 0, 1), (80, 2, 9, 0, 0, 1),
                (80, 0, 2, 17, 0, 1), (80, 0, 2, 0, 17, 1), (80, 0, 2, 0, 0, 0), (80, 0, 2, 0, 0, 65), (80, 1, 8, 16, 16, 64),
                (2049, 1, 2, 0, 0, 1)):
        assert L.alacgpu_stack_create(0, ctypes.byref(pkg.StackConfig(*cfg, 0.0)), ctypes.byref(h)) == -2 and not h, cfg
        assert b"no stacking plan" in L.alacgpu_last_error()
    assert L.alacgpu_stack_create(0, None, ctypes.byref(h)) == -2
    assert L.alacgpu_stack_create(0, ctypes.byref(pkg.StackConfig(80, 0, 2, 0, 0, 1, 0.0)), None) == -2
    ms = ctypes.c_float()
    assert L.alacgpu_stack_device(None, 16, 80, 8, 1, 1, 10, None, 4096, 80, 8, 1, None, 1) == -2
    assert L.alacgpu_stack_last_ms(None, ctypes.byref(ms)) == -2 and L.alacgpu_stack_synchronize(None) == -2
    assert L.alacgpu_stack_plan(None, ctypes.byref(pkg.StackInfo()), None, 0) == -2
    assert L.alacgpu_stack_out_frames(None, 7) == 0 and not L.alacgpu_stack_stream(None)
    L.alacgpu_stack_destroy(None)
    for kw in (dict(bins=0), dict(bins=4097), dict(bins=80, order=3), dict(bins=80, order=-1), dict(bins=80, order=1, window=0),
               dict(bins=80, order=2, window=9), dict(bins=80, left=17), dict(bins=80, right=-1), dict(bins=80, stride=0),
               dict(bins=80, stride=65), dict(bins=80, order=1, window=8, left=16, right=16, stride=64), dict(bins=80.5),
               dict(bins=True), dict(bins=80, order=1.5)):
        with pytest.raises(ValueError):
            pkg.NewFrameStack(**kw)
    import torch
    x = torch.zeros(2, 10, 80)
    for call in (lambda: pkg.stack_frames(x, order=3), lambda: pkg.stack_frames(x, stride=0), lambda: pkg.add_deltas(x, window=9),
                 lambda: pkg.lfr(x, m=34), lambda: pkg.lfr(x, m=0), lambda: pkg.lfr(x, n=65), lambda: pkg.lfr(x, m=60, n=6),
                 lambda: pkg.stack_frames(x, layout="rows"), lambda: pkg.stack_frames(x.numpy()),
                 lambda: pkg.load_features([], [], 1, deltas=3), lambda: pkg.load_features([], [], 1, context=(17, 0)),
                 lambda: pkg.load_features([], [], 1, context=3), lambda: pkg.load_features([], [], 1, subsample=0)):
        with pytest.raises(ValueError):
            call()
    S = sr.build_stack_shim(pkg)
    sizes = np.zeros(3, np.uint64)
    S.stack_shim_sizes(sizes.ctypes.data)
    assert ctypes.sizeof(pkg.StackConfig) == sizes[0] == 28 and ctypes.sizeof(pkg.StackInfo) == sizes[1] == 52
    assert pkg.StackConfig.pad_value.offset == sizes[2] == 24
    assert S.stack_shim_create(ctypes.byref(pkg.StackConfig(80, 3, 2, 0, 0, 1, 0.0))) == -6
    assert b"no stacking plan" in S.stack_shim_last_error()
    assert S.stack_shim_create(ctypes.byref(pkg.StackConfig(80, 1, 8, 16, 16, 64, 0.0))) == -6


# ---- 6. the stand-alone program ------------------------------------------------------------------------------------------
def test_standalone_program_builds_and_runs(tmp_path):
    """tests/host_sim/stack_san_main.cpp, the program with its own main over stack_sim.cpp's functions that DESIGN.md §17 runs
    under the sanitizers on a CPU: here it is built plainly and run once, so that it stays in step with the header"""
    exe = str(tmp_path / "stack_san")
    host_build.compile("stack_san_main.cpp", exe, ["-O1", "-ffp-contract=off", "-fwrapv", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count("-> 0,") == 23 * 4 and "92 passes" in r.stdout and "nan" not in r.stdout.lower()


# ---- 7. the names --------------------------------------------------------------------------------------------------------
def test_names_in_library_and_binding(pkg):
    import inspect
    for name in ("StackConfig", "StackInfo", "FrameStack", "NewFrameStack", "stack_frames", "add_deltas", "lfr"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("create", "destroy", "stream", "synchronize", "last_ms", "out_frames", "device", "plan"):
        assert "alacgpu_stack_" + name in pkg._EXPORTS
    assert issubclass(pkg.FrameStack, pkg._RowPass)
    assert list(inspect.signature(pkg.NewFrameStack).parameters) == ["bins", "order", "window", "left", "right", "stride", "pad_value",
                                                                    "device"]
    assert list(inspect.signature(pkg.FrameStack.__call__).parameters) == ["self", "feats", "lengths", "layout", "out", "out_layout"]
    assert list(inspect.signature(pkg.stack_frames).parameters)[:9] == ["feats", "lengths", "order", "window", "left", "right", "stride",
                                                                        "layout", "pad_value"]
    par = inspect.signature(pkg.add_deltas).parameters
    assert list(par)[:5] == ["feats", "lengths", "order", "window", "layout"] and (par["order"].default, par["window"].default) == (2, 2)
    par = inspect.signature(pkg.lfr).parameters
    assert list(par)[:5] == ["feats", "lengths", "m", "n", "layout"] and (par["m"].default, par["n"].default) == (7, 6)
    par = inspect.signature(pkg.load_features).parameters
    assert list(par)[:8] == ["sources", "frame_offsets", "num_frames", "sample_rate", "kind", "norm", "channel", "transform"]
    assert list(par)[8:13] == ["device", "deltas", "delta_window", "context", "subsample"]
    assert [par[k].default for k in ("deltas", "delta_window", "context", "subsample")] == [0, 2, (0, 0), 1]
    assert "not compute_deltas applied twice" in " ".join(pkg.FrameStack.__doc__.split())
    mk = open(os.path.join(sr.ROOT, "saprobe-alac_amd", "csrc", "Makefile")).read()
    assert "k_stack" in mk.split("UNITS =")[1].split("\n")[0].split() and "build/k_stack.o: alac_stack.h" in mk
    assert b"alacgpu 0.7.0 gfx950" == pkg.lib().alacgpu_version()
