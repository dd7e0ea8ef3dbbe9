"""The SpecAugment pass on the CPU: csrc/alac_specaug.h built with g++, contraction off (tests/host_sim/specaug_sim.cpp), workgroup
for workgroup and work item for work item what the gfx950 kernel of k_specaug.hip runs, against tests/specaug_ref.py's numpy
restatement bit for bit, against the properties the definition promises, and against float64 linear interpolation within a bound
computed from the data.

* Philox4x32-10's two known answers, from the host build and from numpy;
* the parameter sets of sa.PARAMS (nothing, masks only, a warp only, everything, the maxima) at the bins 1, 23, 80, 129, the frames
  1, 2, tile_out - 1, tile_out, tile_out + 1 and 3 tile_out + 5, seven rows with the lengths -3, 0, 1, 2 W, 2 W + 1, frames and
  frames + 9, both layouts in and both out; the maxima also at 530 frames, where a warp of 256 takes effect; the same at the wide
  bins 193, 257, 513, 1025 and 4096 (sa.WIDE_BINS), where the masked bins fill up to 128 words and the tile shrinks to one
  frame;
* rows and lines padded apart, every base offset, NaN and Inf in all padding and gaps, canaries around the output and the draws;
* the properties: nothing in, the input's bits out; a row alone is the row in its batch; every draw in its range; every width
  occurs; the padding is never read; a row of at most 2 W frames is not warped;
* what is refused (by the host build, by the library before any HIP call, by the Python entries and by the C++ mirror), the
  structs' sizes, the stand-alone program that the sanitizer run uses, the new names."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import host_build
from tests import specaug_ref as sa

F32 = np.float32
CANARY = F32(-12345.5)
SEED = 0x1234_5678_9ABC_DEF1
CASES = [(name, bins) for name in sa.PARAMS for bins in sa.BINS]
CASES += [(name, bins) for bins in sa.WIDE_BINS for name in sa.PARAMS]  # tile_out 31, 23, 11, 5 and 1; nothing is cut there
IDS = ["%s-%d" % c for c in CASES]
KW = dict(mask_value=-7.0, pad_value=-3.5)


@pytest.fixture(scope="module")
def sim():
    return sa.build_specaug_sim()


# ---- 1. the random words and the plan ------------------------------------------------------------------------------------
def test_philox_known_answers(sim):
    zero = [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    pi = [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    counter, key = [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0)
    assert sa.philox4x32_10([0, 0, 0, 0], (0, 0)) == zero and sa.sim_philox(sim, [0, 0, 0, 0], (0, 0)) == zero
    assert sa.philox4x32_10(counter, key) == pi and sa.sim_philox(sim, counter, key) == pi
    # word j of a row: word j % 4 of the block at (id low, id high, j // 4, 0) under (seed low, seed high)
    ident, seed = 0x85A308D3_243F6A88, 0x299F31D0_A4093822
    assert sa.words_of(seed, ident, 7) == (sa.philox4x32_10([0x243F6A88, 0x85A308D3, 0, 0], key) +
                                           sa.philox4x32_10([0x243F6A88, 0x85A308D3, 1, 0], key))[:7]


def test_plan_is_a_function_of_the_bins(sim):
    """tile_out in [1, 64], the largest whose image fits; the LDS within 25 600 bytes; P = 2 + 2 nf + 2 nt"""
    for bins in list(range(1, 301)) + [512, 1000, 2048, 4095, 4096]:
        for ps in ((0, 0, 0, 0, 0, 0), (8, bins, 16, 65535, 65536, 256)):
            rc, pl = sa.sim_plan(sim, ps, bins)
            assert rc == 0 and pl == sa.plan_of(ps, bins), (bins, pl)
            T = pl["tile_out"]
            assert 1 <= T <= 64 and pl["lds_bytes"] <= 25600 and pl["draws"] == 2 + 2 * ps[0] + 2 * ps[2]
            assert T == 64 or bins * ((T + 1) | 1) > sa.IMAGE_FLOATS, "a larger tile would fit"
    assert [sa.tile_out_of(b) for b in (1, 23, 80, 129, 4096)] == [64, 64, 64, 45, 1]


# ---- 2. bit for bit against the numpy restatement: gaps, offsets, poisoned padding, canaries --------------------------------
def run_over_buffers(sim, x, lengths, ps, in_layout, out_layout, row_gap, inner_gap, lead, poison, **kw):
    """x laid out with gaps -> (y, draws) of the host build; asserts that nothing but the output's elements and the rows' draws
    changed"""
    rows, frames, bins = x.shape
    P = 2 + 2 * ps[0] + 2 * ps[2]
    xin = x.copy()
    if poison is not None:
        for r, n in enumerate(sa.clamp_lengths(lengths, rows, frames)):
            xin[r, n:] = poison
    buf, view, st = sa.lay_out(xin, in_layout, row_gap, inner_gap, lead, fill=CANARY if poison is None else poison)
    olead = (lead + 1) % 4
    obuf, oview, ost = sa.lay_out(np.zeros_like(x), out_layout, row_gap + 1, inner_gap + 2, olead, fill=CANARY)
    before = buf.copy()
    draws = np.full((rows + 2, P), -77, np.int32)
    rc = sa.host_run(sim, ps, bins, view.ctypes.data, st, rows, frames, lengths, SEED, oview.ctypes.data, ost, draws[1:], **kw)
    assert rc == 0
    rest = sa.outside(obuf, lambda b: sa.view_like(b, olead, x.shape, ost))
    assert rest.size and (rest.view(np.uint32) == CANARY.view(np.uint32)).all(), "an element outside the output was written"
    assert np.array_equal(buf.view(np.uint32), before.view(np.uint32)), "the input changed"
    assert (draws[0] == -77).all() and (draws[-1] == -77).all(), "exactly rows x P draws are written"
    return oview.copy(), draws[1:-1]


@pytest.mark.parametrize("name,bins", CASES, ids=IDS)
def test_bits_against_the_reference(sim, name, bins):
    ps = sa.for_bins(sa.PARAMS[name], bins)
    assert sa.accepted(ps, bins)
    rng = np.random.default_rng(1000 + bins)
    k = 0
    for frames in sa.frames_of(bins) + ((530,) if name == "max" and bins == 23 else ()):
        lengths = sa.lengths_of(frames, ps[5])
        x = sa.features(rng, len(lengths), frames, bins)
        want, want_draws = sa.reference(x, lengths, ps, SEED, row_base=11, **KW)
        if frames == 530:
            assert want_draws[5, 1] > 0 and want_draws[4, 1] > 0 and want_draws[3, 1] == 0, "513 frames and more are warped"
        for in_layout in ("frames", "bins"):
            for out_layout in ("frames", "bins"):
                lead = k % 4
                poison = (F32(np.nan), F32(np.inf), None, F32(-np.inf))[(k // 4) % 4]
                k += 1
                y, draws = run_over_buffers(sim, x, lengths, ps, in_layout, out_layout, (0, 5, 1, 7)[lead], (0, 3, 1, 2)[lead], lead,
                                            poison, row_base=11, **KW)
                assert sa.same_bits(y, want), "%d frames, %s -> %s, lead %d" % (frames, in_layout, out_layout, lead)
                assert np.array_equal(draws, want_draws)
        # no lengths: every frame is valid; ids in place of the row base
        ids = [2 ** 63 - 1, -1, 11 + 2]
        full, fd = sa.host_values(sim, x[:3], None, ps, SEED, "bins", "frames", ids=ids, **KW)
        want3, wd3 = sa.reference(x[:3], None, ps, SEED, ids=ids, **KW)
        assert sa.same_bits(full, want3) and np.array_equal(fd, wd3)
        # in place where there is no warp, either layout
        if ps[5] == 0:
            for layout in ("frames", "bins"):
                _, view, st = sa.lay_out(x, layout, 3, 2, 1)
                assert sa.host_run(sim, ps, bins, view.ctypes.data, st, len(lengths), frames, lengths, SEED, view.ctypes.data, st,
                                   row_base=11, **KW) == 0
                assert sa.same_bits(view, want), "in place, %s" % layout


# ---- 3. the properties ---------------------------------------------------------------------------------------------------
def test_nothing_to_do_returns_the_inputs_bits(sim):
    """No masks and no warp: the valid frames' bits, NaN payloads, infinities and -0.0 included, and pad_value behind them; with a
    warp parameter but rows too short for it, the same"""
    rng = np.random.default_rng(3)
    frames, bins = 70, 23
    raw = rng.integers(0, 2 ** 32, (5, frames, bins), dtype=np.uint64).astype(np.uint32)
    raw[0, :4, :4] = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0x80000000], np.uint32)
    x = raw.view(F32)
    lengths = [frames, 0, 33, 64, 65]
    for ps in (sa.PARAMS["noop"], (0, 0, 0, 0, 65536, 40)):  # 2 W = 80 >= every length: no row is warped
        for il in ("frames", "bins"):
            for ol in ("frames", "bins"):
                y, draws = sa.host_values(sim, x, lengths, ps, SEED, il, ol, pad_value=9.0)
                for r, n in enumerate(lengths):
                    assert np.array_equal(y[r, :n].view(np.uint32), raw[r, :n]) and (y[r, n:] == 9.0).all()
                assert not draws.any()


def test_a_row_alone_is_the_row_in_its_batch(sim):
    rng = np.random.default_rng(4)
    frames, bins, ps = 150, 23, sa.for_bins(sa.PARAMS["all"], 23)
    x = sa.features(rng, 6, frames, bins)
    lengths = [150, 90, 11, 140, 0, 77]
    batch, bd = sa.host_values(sim, x, lengths, ps, SEED, row_base=1000)
    for k in range(6):
        alone, ad = sa.host_values(sim, x[k:k + 1], lengths[k:k + 1], ps, SEED, ids=[1000 + k])
        assert sa.same_bits(alone[0], batch[k]) and np.array_equal(ad[0], bd[k])
        moved, md = sa.host_values(sim, x[k:k + 1], lengths[k:k + 1], ps, SEED, row_base=1000 + k)
        assert sa.same_bits(moved[0], batch[k]) and np.array_equal(md[0], bd[k])
    other, od = sa.host_values(sim, x, lengths, ps, SEED, row_base=2000)
    again, gd = sa.host_values(sim, x, lengths, ps, SEED + 1, row_base=1000)
    for k in (0, 1, 3, 5):
        assert not np.array_equal(od[k], bd[k]) and not sa.same_bits(other[k], batch[k]), "another row_base, other draws"
        assert not np.array_equal(gd[k], bd[k]), "another seed, other draws"


def test_every_draw_in_its_range_and_every_width_occurs(sim):
    """4096 identities at Fw = 10, Tw = 20, W = 5 with lengths over [0, frames]: c in [W, n - W), w in [c - W + 1, c + W], a frequency
    mask inside the bins, a time mask inside [0, n) and no longer than its cap; every width from 0 to the cap occurs (the words
    are fixed by the seed: the counts below are what this seed gives)"""
    rows, frames, bins = 4096, 40, 23
    ps = (2, 10, 2, 20, 65536, 5)
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, frames + 1, rows).astype(np.int32)
    lengths[:4] = (0, 10, 11, frames)
    x = np.zeros((rows, frames, bins), F32)
    _, d = sa.host_values(sim, x, lengths, ps, SEED, row_base=7)
    assert np.array_equal(d[:64], np.array([sa.draws_of(ps, bins, int(lengths[r]), SEED, 7 + r) for r in range(64)], np.int32))
    n = lengths.astype(np.int64)
    c, w = d[:, 0].astype(np.int64), d[:, 1].astype(np.int64)
    warped = n > 10
    assert (c[~warped] == 0).all() and (w[~warped] == 0).all()
    assert (c[warped] >= 5).all() and (c[warped] < n[warped] - 5).all()
    assert (w[warped] >= c[warped] - 4).all() and (w[warped] <= c[warped] + 5).all()
    assert (w[warped] >= 1).all() and (w[warped] <= n[warped] - 1).all()
    assert set((w - c)[warped].tolist()) == set(range(-4, 6)), "every displacement occurs"
    for i in range(2):
        f0, fw = d[:, 2 + 2 * i], d[:, 3 + 2 * i]
        assert (fw >= 0).all() and (fw <= 10).all() and (f0 >= 0).all() and (f0 + fw <= bins).all()
        assert set(fw.tolist()) == set(range(11))
        t0, tw = d[:, 6 + 2 * i].astype(np.int64), d[:, 7 + 2 * i].astype(np.int64)
        assert (tw >= 0).all() and (tw <= np.minimum(20, n)).all() and (t0 >= 0).all() and (t0 + tw <= n).all()
        assert set(tw.tolist()) == set(range(21))
    # the ratio caps a mask by the row's own length
    _, dq = sa.host_values(sim, x, lengths, (0, 0, 2, 20, 13107, 0), SEED)
    assert (dq[:, 3] <= (n * 13107) >> 16).all() and (dq[:, 5] <= (n * 13107) >> 16).all() and dq[:, 3].max() == (frames * 13107) >> 16


def test_the_padding_is_never_read_and_short_rows_are_not_warped(sim):
    rng = np.random.default_rng(6)
    frames, bins = 90, 23
    for name in ("warp", "all", "max"):
        ps = sa.for_bins(sa.PARAMS[name], bins)
        lengths = sa.lengths_of(frames, 5) + [2 * 5 - 1, 40]
        x = sa.features(rng, len(lengths), frames, bins)
        clean, cd = sa.host_values(sim, x, lengths, ps, SEED, **KW)
        for poison in (np.nan, np.inf, 1e30):
            bad = x.copy()
            for r, n in enumerate(sa.clamp_lengths(lengths, len(lengths), frames)):
                bad[r, n:] = poison
            for il in ("frames", "bins"):
                y, d = sa.host_values(sim, bad, lengths, ps, SEED, il, "frames", **KW)
                assert sa.same_bits(y, clean) and np.array_equal(d, cd)
    # W > 0 and n <= 2 W: the identity
    ps = sa.PARAMS["warp"]
    lengths = [0, 1, 9, 10, 11]
    x = sa.features(rng, 5, 30, bins)
    y, d = sa.host_values(sim, x, lengths, ps, SEED)
    for r, n in enumerate(lengths):
        assert (d[r, 1] > 0) == (n > 10)
        if n <= 10:
            assert sa.same_bits(y[r, :n], x[r, :n])
    assert not sa.same_bits(y[4, :11], x[4, :11])


# ---- 4. the warp against float64 -----------------------------------------------------------------------------------------
def test_warp_against_float64_interpolation(sim):
    """F.interpolate(mode="linear", align_corners=False) in float64 over the two segments that the draws name. Per element
    |y - y64| <= 2^-23 |x1 - x0| + u (|x1 - x0| + |y|), u = 2^-24: the floored weight, the subtraction's rounding and the fma's.
    Largest observed fraction of the bound over these cases: 0.994."""
    import torch
    rng = np.random.default_rng(7)
    worst = 0.0
    for bins, frames, W in ((23, 200, 5), (80, 130, 40), (1, 600, 256), (129, 91, 1), (513, 40, 5), (4096, 13, 2)):
        ps = (0, 0, 0, 0, 65536, W)
        rows = 8
        x = rng.normal(0.0, 1.0, (rows, frames, bins)).astype(F32)
        lengths = [frames, 2 * W + 1, 2 * W + 2, frames - 1, frames - 7, (frames + 2 * W) // 2, frames, frames]
        y, d = sa.host_values(sim, x, lengths, ps, SEED, row_base=bins)
        for r, n in enumerate(lengths):
            c, w = int(d[r, 0]), int(d[r, 1])
            assert W <= c < n - W and c - W + 1 <= w <= c + W
            v = torch.from_numpy(x[r, :n].astype(np.float64).T.copy())[None]  # [1, bins, n]
            y64 = torch.cat([torch.nn.functional.interpolate(v[..., :c], size=w, mode="linear", align_corners=False),
                             torch.nn.functional.interpolate(v[..., c:], size=n - w, mode="linear", align_corners=False)], dim=2)
            y64 = y64[0].numpy().T
            i0, i1, _ = sa.row_plan(n, c, w)
            gap = np.abs(x[r, i1].astype(np.float64) - x[r, i0].astype(np.float64))
            got = y[r, :n].astype(np.float64)
            lim = 2.0 ** -23 * gap + sa.U * (gap + np.abs(got))
            err = np.abs(got - y64)
            frac = float((err / np.maximum(lim, 1e-300)).max())
            print("bins %d, n %d, c %d -> w %d: largest error / bound %.3f" % (bins, n, c, w, frac))
            assert (err <= lim).all(), (bins, n, c, w, frac)
            worst = max(worst, frac)
            if c == w:  # a segment of as many output frames as source frames is copied
                assert sa.same_bits(y[r, :w], x[r, :c])
    print("largest error / bound %.3f" % worst)


# ---- 5. what is refused --------------------------------------------------------------------------------------------------
def test_refusals_of_the_host_build(sim):
    x = np.zeros(4 * 10 * 8 + 64, F32)
    out = np.full(4 * 10 * 8 + 64, CANARY, F32)
    draws = np.full(4 * 10 + 1, -77, np.int32)
    ids = np.zeros(5, np.int64)

    def run(ps=(2, 4, 2, 5, 65536, 0), strides=(80, 8, 1), ostrides=(80, 8, 1), rows=4, frames=10, bins=8, inp=x.ctypes.data,
            outp=out.ctypes.data, lengths=None, idp=None, drp=draws.ctypes.data):
        cfg = sa.config_words(ps, bins)
        return sim.specaug_sim_run(cfg.ctypes.data, 0.0, 0.0, inp, *strides, rows, frames, lengths, SEED, 0, idp, outp, *ostrides, drp)

    assert run() == 0 and (draws[:40] != -77).all() and draws[40] == -77
    warp = (2, 4, 2, 5, 65536, 3)
    for bad in (dict(bins=0), dict(bins=4097), dict(ps=(9, 4, 2, 5, 65536, 0)), dict(ps=(2, 9, 2, 5, 65536, 0)),
                dict(ps=(2, 4, 17, 5, 65536, 0)), dict(ps=(2, 4, 2, 65536, 65536, 0)), dict(ps=(2, 4, 2, 5, 65537, 0)),
                dict(ps=(2, 4, 2, 5, 65536, 257)), dict(ps=(2 ** 32 - 1, 4, 2, 5, 65536, 0)), dict(ps=(2, 4, 2, 5, 65536, 2 ** 32 - 1)),
                dict(inp=None), dict(outp=None), dict(inp=x.ctypes.data + 2), dict(outp=out.ctypes.data + 1),
                dict(lengths=x.ctypes.data + 2), dict(idp=ids.ctypes.data + 4), dict(drp=draws.ctypes.data + 2),
                dict(strides=(80, 8, 2)), dict(ostrides=(160, 16, 2)), dict(strides=(79, 8, 1)), dict(ostrides=(79, 8, 1)),
                dict(strides=(80, 7, 1)), dict(ostrides=(80, 7, 1)), dict(strides=(80, 1, 9)), dict(ostrides=(80, 1, 9)),
                dict(strides=(2 ** 62, 8, 1)), dict(frames=2 ** 31, strides=(2 ** 34, 8, 1), ostrides=(2 ** 34, 8, 1)),
                # an output that overlaps the input: behind its start, ending inside it, the same base under other strides
                dict(outp=x.ctypes.data + 4 * 100), dict(inp=out.ctypes.data + 4 * 40, rows=1),
                dict(outp=x.ctypes.data, ostrides=(80, 1, 10)), dict(outp=x.ctypes.data, ostrides=(81, 8, 1)),
                # in place with a warp
                dict(ps=warp, outp=x.ctypes.data), dict(ps=(0, 0, 0, 0, 0, 1), outp=x.ctypes.data)):
        out[...] = CANARY
        draws[...] = -77
        assert run(**bad) == -2, bad
        assert (out == CANARY).all() and not x.any() and (draws == -77).all()
    assert run(outp=x.ctypes.data) == 0, "in place without a warp"
    assert run(outp=x.ctypes.data, strides=(80, 1, 10), ostrides=(80, 1, 10)) == 0, "in the bins layout too"
    x[...] = 0
    assert run(ps=warp) == 0 and run(inp=out.ctypes.data + 4 * 80, rows=1, ostrides=(80, 8, 1)) == 0, "end to end is apart"
    assert run(idp=ids.ctypes.data, drp=None) == 0 and run(ps=(0, 0, 0, 0, 0, 0), drp=None) == 0
    out[...] = CANARY
    assert run(rows=0) == 0 and run(frames=0) == 0 and run(rows=0, inp=None, outp=None) == 0 and (out == CANARY).all()


def test_refusals_of_the_library_and_its_mirrors(pkg):
    """alacgpu_specaug_create refuses before any HIP call (this runs without a GPU), and so do the Python class, the functional
    entries and the C++ mirror; a NULL handle is refused by every entry"""
    pkg.build()
    L = pkg.lib()
    h = ctypes.c_void_p()
    for cfg in ((0, 2, 0, 2, 100, 65536, 0), (4097, 2, 27, 2, 100, 65536, 0), (80, 9, 27, 2, 100, 65536, 0), (80, 2, 81, 2, 100, 65536, 0),
                (80, 2, 27, 17, 100, 65536, 0), (80, 2, 27, 2, 65536, 65536, 0), (80, 2, 27, 2, 100, 65537, 0),
                (80, 2, 27, 2, 100, 65536, 257)):
        assert L.alacgpu_specaug_create(0, ctypes.byref(pkg.SpecAugConfig(*cfg, 0.0, 0.0)), ctypes.byref(h)) == -2 and not h, cfg
        assert b"no SpecAugment plan" in L.alacgpu_last_error()
    assert L.alacgpu_specaug_create(0, None, ctypes.byref(h)) == -2
    assert L.alacgpu_specaug_create(0, ctypes.byref(pkg.SpecAugConfig(80, 2, 27, 2, 100, 65536, 0, 0.0, 0.0)), None) == -2
    ms = ctypes.c_float()
    assert L.alacgpu_specaug_device(None, 16, 80, 8, 1, 1, 10, None, 1, 0, None, 4096, 80, 8, 1, None, 1) == -2
    assert L.alacgpu_specaug_last_ms(None, ctypes.byref(ms)) == -2 and L.alacgpu_specaug_synchronize(None) == -2
    assert L.alacgpu_specaug_plan(None, ctypes.byref(pkg.SpecAugInfo())) == -2 and not L.alacgpu_specaug_stream(None)
    L.alacgpu_specaug_destroy(None)
    for kw in (dict(bins=0), dict(bins=4097), dict(bins=80, freq_masks=9), dict(bins=80, freq_masks=-1), dict(bins=80, freq_width=81),
               dict(bins=23), dict(bins=80, time_masks=17), dict(bins=80, time_width=65536), dict(bins=80, time_ratio=1.5),
               dict(bins=80, time_ratio=-0.1), dict(bins=80, time_ratio="1"), dict(bins=80, warp=257), dict(bins=80, warp=2.5),
               dict(bins=80.5), dict(bins=True)):
        with pytest.raises(ValueError):
            pkg.NewSpecAugment(**kw)
    import torch
    x = torch.zeros(2, 10, 80)
    for call in (lambda: pkg.spec_augment(x), lambda: pkg.spec_augment(x, None), lambda: pkg.spec_augment(x, seed=1, freq_masks=9),
                 lambda: pkg.spec_augment(x, seed=1, warp=257), lambda: pkg.spec_augment(x, seed=1, time_ratio=2),
                 lambda: pkg.spec_augment(x[..., :20], seed=1), lambda: pkg.spec_augment(x, seed=1, layout="rows"),
                 lambda: pkg.spec_augment(x.numpy(), seed=1), lambda: pkg.load_features([], [], 1, augment={"warp": 2}),
                 lambda: pkg.load_features([], [], 1, augment={}), lambda: pkg.load_features([], [], 1, augment=7),
                 lambda: pkg.load_features([], [], 1, augment={"seed": 1, "out": x})):
        with pytest.raises(ValueError):
            call()
    S = sa.build_specaug_shim(pkg)
    sizes = np.zeros(5, np.uint64)
    S.specaug_shim_sizes(sizes.ctypes.data)
    assert ctypes.sizeof(pkg.SpecAugConfig) == sizes[0] == 36 and ctypes.sizeof(pkg.SpecAugInfo) == sizes[1] == 48
    assert pkg.SpecAugConfig.mask_value.offset == sizes[2] == 28 and sizes[3] == round(0.2 * 65536) == 13107 and sizes[4] == 65536
    assert S.specaug_shim_create(ctypes.byref(pkg.SpecAugConfig(80, 9, 27, 2, 100, 65536, 0, 0.0, 0.0))) == -6
    assert b"no SpecAugment plan" in S.specaug_shim_last_error()
    assert S.specaug_shim_create(ctypes.byref(pkg.SpecAugConfig(80, 2, 27, 2, 100, 65536, 300, 0.0, 0.0))) == -6


# ---- 6. the stand-alone program ------------------------------------------------------------------------------------------
def test_standalone_program_builds_and_runs(tmp_path):
    """tests/host_sim/specaug_san_main.cpp, the program with its own main over specaug_sim.cpp's functions that DESIGN.md §18 runs
    under the sanitizers on a CPU: here it is built plainly and run once, so that it stays in step with the header"""
    exe = str(tmp_path / "specaug_san")
    host_build.compile("specaug_san_main.cpp", exe, ["-O1", "-ffp-contract=off", "-fwrapv", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count("-> 0,") == 100 and "100 passes" in r.stdout and "nan" not in r.stdout.lower()


# ---- 7. the names --------------------------------------------------------------------------------------------------------
def test_names_in_library_and_binding(pkg):
    import inspect
    for name in ("SpecAugConfig", "SpecAugInfo", "SpecAugment", "NewSpecAugment", "spec_augment"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("create", "destroy", "stream", "synchronize", "last_ms", "device", "plan"):
        assert "alacgpu_specaug_" + name in pkg._EXPORTS
    assert issubclass(pkg.SpecAugment, pkg._FeaturePass)
    par = inspect.signature(pkg.NewSpecAugment).parameters
    assert list(par) == ["bins", "freq_masks", "freq_width", "time_masks", "time_width", "time_ratio", "warp", "mask_value", "pad_value",
                         "device"]
    assert [par[k].default for k in list(par)[1:]] == [2, 27, 2, 100, 1.0, 0, 0.0, 0.0, 0]
    par = inspect.signature(pkg.SpecAugment.__call__).parameters
    assert list(par) == ["self", "feats", "lengths", "seed", "ids", "row_base", "layout", "out", "out_layout", "return_draws"]
    assert [par[k].default for k in list(par)[2:]] == [None, 0, None, 0, "frames", None, None, False]
    par = inspect.signature(pkg.spec_augment).parameters
    assert list(par)[:3] == ["feats", "lengths", "seed"] and par["lengths"].default is None
    assert not isinstance(par["seed"].default, (int, float)) and par["seed"].default is not None, "no usable default seed"
    par = inspect.signature(pkg.load_features).parameters
    assert list(par)[8:14] == ["device", "deltas", "delta_window", "context", "subsample", "augment"] and par["augment"].default is None
    mk = open(os.path.join(sa.ROOT, "saprobe-alac_amd", "csrc", "Makefile")).read()
    assert "k_specaug" in mk.split("UNITS =")[1].split("\n")[0].split() and "build/k_specaug.o: alac_specaug.h" in mk
