"""The resampler on the CPU: csrc/alac_resample.h built with g++ (tests/host_sim/resample_sim.cpp), tile for tile and work
item for work item what the gfx950 kernel of k_resample.hip runs, against the numpy float64 restatement of
tests/resample_ref.py.

* the plan (o, n, width, the float32 window table, the window starts) against the full double table, for every pair the plan
  must accept;
* a sweep over ratios, row counts, lengths around the filter width and the tile boundaries, and every input and output
  base offset of 0..3 elements with odd row strides: the WHOLE sentinel-filled output buffer is compared, the sentinel outside
  the rows' columns [0, out_frames), inside them the float32 dot-product bound against the restatement run on the plan's own
  table; once more with the input ending at an inaccessible page;
* the same sweep over other filter widths, rolloffs, upsampling pairs and every tile_out, within the running-error bound of the
  chain as well (rr.running_bound), which is 5 to 50 times tighter; what the sweeps reach, computed from the tile cut;
* impulses, which come out as single table entries bit for bit: the index arithmetic checked exactly and independently of the
  plan's own walk;
* the restatement itself against analytic sines and a constant;
* the arguments the entries reject, and the new names in the library, the header and the binding."""
import ctypes
import os
import re
import time

import numpy as np
import pytest

from tests import resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = [(2, 3), (3, 2), (7, 5), (8000, 48000), (48000, 16000), (44100, 16000), (48000, 44100), (192000, 8000)]
NAMES = ["alacgpu_resampler_create", "alacgpu_resampler_destroy", "alacgpu_resampler_stream", "alacgpu_resampler_synchronize",
         "alacgpu_resampler_last_ms", "alacgpu_resample_out_frames", "alacgpu_resample_device", "alacgpu_resampler_plan"]


@pytest.fixture(scope="module")
def sim():
    return rr.build_resample_sim()


def aligned(elems, fill=None):
    """A float32 array of `elems` elements on a 16-byte boundary."""
    own = np.zeros(elems + 8, np.uint32)
    off = (-own.ctypes.data // 4) % 4
    a = own[off:off + elems]
    assert a.ctypes.data % 16 == 0
    if fill is not None:
        a[:] = fill
    return a


def run_sim(S, orig, new, x, in_off=0, out_off=0, guard=0, W=6, rolloff=0.99):
    """The rows x laid out with an odd stride in_off elements behind a 16-byte boundary, the pass into a sentinel-filled
    buffer whose rows start out_off elements behind one -> (image uint32, out_lead, out_stride, frames)."""
    rows, T = x.shape
    frames = rr.out_frames(orig, new, T)
    in_stride, in_lead, in_elems, out_stride, out_lead, out_elems = rr.layout(rows, T, frames, in_off, out_off)
    src = aligned(in_elems, 0x7FC00000)  # NaN between the rows: a read outside a row's [0, T) shows
    for r in range(rows):
        src[in_lead + r * in_stride: in_lead + r * in_stride + T] = x[r].view(np.uint32)
    img = aligned(out_elems, rr.SENTINEL)
    rc = S.resample_sim_run(orig, new, W, rolloff, src.ctypes.data + 4 * in_lead, in_stride, rows, T, img.ctypes.data + 4 * out_lead,
                            out_stride, guard)
    assert rc == 0
    return img.copy(), out_lead, out_stride, frames


# ---- 1. the plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", rr.PAIRS)
def test_plan_against_the_restatement(sim, orig, new):
    t0 = time.time()
    plan = rr.sim_plan(sim, orig, new)
    took = time.time() - t0
    assert plan is not None, "no plan"
    info, h32, first = plan
    o, n, base, width = rr.geometry(orig, new)
    assert (info["o"], info["n"], info["width"]) == (o, n, width)
    taps = info["taps"]
    assert 1 <= taps <= 2 * width + 2 and h32.shape == (n, taps)
    assert info["tile_out"] % 64 == 0 and 64 <= info["tile_out"] <= 1024
    assert 0 < sim.resample_sim_stage_need(orig, new, 6, 0.99) <= sim.resample_sim_stage_floats()
    assert first.min() >= 0 and first.max() + taps <= 2 * width + o
    # the window: every entry one float32 rounding of the peak tap from the double value, doubled
    want = rr.taps_at(orig, new, np.arange(n)[:, None], first[:, None].astype(np.int64) + np.arange(taps)[None, :])
    assert np.abs(h32.astype(np.float64) - want).max() <= 2.0 ** -23 * base / o
    # outside the window the full table is exactly zero (44 100 -> 22 051: 22 051 rows of 44 126 taps, so a sample of rows)
    rng = np.random.default_rng(orig + new)
    phases = np.arange(n) if n * (2 * width + o) <= 2_000_000 else np.unique(np.concatenate([np.arange(8), n - 1 - np.arange(8),
                                                                                                rng.integers(0, n, 48)]))
    H = rr.table(orig, new, phases=phases)
    k = np.arange(2 * width + o)[None, :]
    f = first[phases][:, None]
    assert not H[(k < f) | (k >= f + taps)].any()
    assert np.count_nonzero(H, axis=1).max() <= taps
    if (orig, new) == (44100, 22051):
        assert took < 5.0, "the plan took %.1f s" % took


# ---- 2. the sweep -----------------------------------------------------------------------------------------------------
ALL16 = [(out_off, in_off) for in_off in range(4) for out_off in range(4)]


def sweep(sim, orig, new, W, rolloff, Ts, offsets, wide=False):
    """Over rows and lengths Ts and the (out_off, in_off) pairs: the whole buffer, the dot-product bound and the running
    bound. wide: the second of five rows is randn * exp(U(-20, 0)), values over nine decades. -> the worst error / bound and
    error / running bound"""
    info, h32, first = rr.sim_plan(sim, orig, new, W, rolloff)
    rng = np.random.default_rng(orig * 7 + new)
    worst = worst_run = 0.0
    for rows in (1, 5):
        for T in Ts:
            x = rr.signal(rng, rows, T)
            if wide and rows > 1:
                x[1] = (rng.standard_normal(T) * np.exp(rng.uniform(-20.0, 0.0, T))).astype(np.float32)
            ref = rr.resample64(x, orig, new, W, rolloff, h=h32, first=first)
            lim = rr.bound(h32, first, x, orig, new, W, rolloff)
            run = rr.running_bound(h32, first, x, orig, new, W, rolloff)
            assert (run <= lim + info["taps"] * 2.0 ** -149).all(), "the running bound is above the dot-product bound"
            images = set()
            for out_off, in_off in offsets:
                img, lead, stride, frames = run_sim(sim, orig, new, x, in_off, out_off, guard=int(in_off == 1), W=W, rolloff=rolloff)
                assert frames == ref.shape[1] == sim.resample_sim_out_frames(orig, new, T)
                got = np.stack([img[lead + r * stride: lead + r * stride + frames] for r in range(rows)]).view(np.float32)
                want = rr.expected_image(got, img.size, lead, stride)
                if not np.array_equal(img, want):
                    bad = np.nonzero(img != want)[0]
                    raise AssertionError("rows %d T %d offsets %d/%d: element %d of the buffer (rows start at %d, stride %d) is "
                                         "%#x" % (rows, T, in_off, out_off, bad[0], lead, stride, img[bad[0]]))
                images.add(got.tobytes())
                err = np.abs(got.astype(np.float64) - ref)
                assert (err <= lim).all(), "rows %d T %d offsets %d/%d: error %g above the bound %g" % (
                    rows, T, in_off, out_off, err.max(), lim.flat[np.argmax(err - lim)])
                assert (err <= run).all(), "rows %d T %d offsets %d/%d: error %g above the running bound %g" % (
                    rows, T, in_off, out_off, err.flat[np.argmax(err - run)], run.flat[np.argmax(err - run)])
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst = max(worst, float(np.nanmax(np.where(lim > 0, err / lim, 0.0))))
                worst_run = max(worst_run, float((err / run).max()))
            assert len(images) == 1, "the values depend on the alignment"
    print("%d -> %d W %d rolloff %g: worst error / bound %.3f, / running bound %.3f" % (orig, new, W, rolloff, worst, worst_run))
    return worst, worst_run


@pytest.mark.parametrize("orig,new", SWEEP)
def test_host_build_within_the_bound_over_the_whole_buffer(sim, orig, new):
    info, _, _ = rr.sim_plan(sim, orig, new)
    sweep(sim, orig, new, 6, 0.99, rr.boundary_frames(info, orig, new), ALL16)


# the cases of rr.CASES the sweep above does not hold already
NEW_CASES = [c for c in rr.CASES if not (c[2:] == (6, 0.99) and c[:2] in SWEEP)]


@pytest.mark.parametrize("orig,new,W,rolloff", NEW_CASES)
def test_host_build_within_the_bounds_for_other_parameters(sim, orig, new, W, rolloff):
    """Upsampling pairs, other filter widths and rolloffs, every tile_out from 1 024 down to 64, the table of 22 051 phases and
    filters of 2 to 1 551 taps. 44 100 -> 22 051 builds its plan in 0.1 s on every call of the host build, so it runs the four
    offset pairs of the GPU suite instead of all sixteen."""
    info, _, _ = rr.sim_plan(sim, orig, new, W, rolloff)
    assert info["tile_out"] == rr.TILE_OUT.get((orig, new, W, rolloff), 1024)
    sweep(sim, orig, new, W, rolloff, rr.sweep_frames(info, orig, new), rr.OFFSETS if info["n"] > 10000 else ALL16, wide=True)


def test_sweeps_reach_every_tile_size_and_chain_count(sim):
    """What the sweeps above run, computed from the restated tile cut (rr.tile_counts) and not by the header: plans of every
    tile_out, and tiles whose work items run 1, 2, 3 and 4 chains (compute_tile's four cases), on the four offset pairs the
    GPU suite uses as well and on its lengths, those above the filter's width."""
    tiles, paths, gpu_paths = set(), set(), set()
    for orig, new, W, rolloff in [(a, b, 6, 0.99) for a, b in SWEEP] + NEW_CASES:
        info, _, _ = rr.sim_plan(sim, orig, new, W, rolloff)
        tiles.add(info["tile_out"])
        Ts = rr.sweep_frames(info, orig, new) if (orig, new, W, rolloff) in NEW_CASES else rr.boundary_frames(info, orig, new)
        for T in Ts:
            for rows in (1, 5):
                for out_off, _ in rr.OFFSETS:
                    here = rr.chain_paths(info["tile_out"], rows, rr.out_frames(orig, new, T), out_off)
                    paths |= here
                    if T > info["width"] and (orig, new, W, rolloff) in rr.CASES:
                        gpu_paths |= here
    assert tiles == {1024, 512, 256, 128, 64}
    assert paths == {1, 2, 3, 4} and gpu_paths == {1, 2, 3, 4}
    # the cut itself, on rows cut by hand
    assert rr.tile_counts(64, 130, 0) == [64, 64, 2] and rr.tile_counts(64, 130, 3) == [61, 64, 5] and rr.tile_counts(64, 61, 3) == [61]


# ---- 2b. impulses: the index arithmetic, exactly -------------------------------------------------------------------------
IMPULSE_PLANS = [(a, b, 6, 0.99) for a, b in SWEEP] + NEW_CASES + [(3, 1, 6, 1.0)]


@pytest.mark.parametrize("orig,new,W,rolloff", IMPULSE_PLANS)
def test_impulses_come_out_as_single_table_entries(sim, orig, new, W, rolloff):
    """x = 1.0 (and -0.5) at places 2 * width + o + 1 apart, +0.0 elsewhere: every output is exactly one table entry (times
    -0.5) or +0.0, at the place the definition y[j * n + i] = sum_k H[i][k] x[j * o + k - width] gives it, compared as uint32
    over the whole sentinel-filled buffer. A window start off by one, a tap dropped at a window's end, an input off by one
    at a tile seam or a staged zero in the wrong place moves or loses an entry; the bounds cannot see that, this can."""
    info, h32, first = rr.sim_plan(sim, orig, new, W, rolloff)
    for amp in (1.0, -0.5):
        x, offsets = rr.impulse_rows(info, orig, new, W, rolloff, amp)
        want = rr.impulse_expected(h32, first, offsets, x.shape[1], orig, new, W, rolloff, amp)
        assert rr.out_frames(orig, new, x.shape[1]) >= 3 * info["tile_out"] and np.count_nonzero(want) > 0
        for out_off, in_off in ((0, 0), (3, 1)):
            img, lead, stride, frames = run_sim(sim, orig, new, x, in_off, out_off, guard=1, W=W, rolloff=rolloff)
            image = rr.expected_image(want, img.size, lead, stride)
            if not np.array_equal(img, image):
                bad = np.nonzero(img != image)[0]
                r, m = divmod(int(bad[0]) - lead, stride)
                raise AssertionError("amplitude %g offsets %d/%d: row %d (impulses from %d on) column %d is %#x, not %#x (%d differ)"
                                     % (amp, in_off, out_off, r, offsets[min(r, len(offsets) - 1)], m, img[bad[0]], image[bad[0]], len(bad)))


# ---- 2c. values outside the audio range ----------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", [(44100, 16000), (2, 3)])
def test_denormals_huge_values_signed_zeros_and_non_finite_inputs(sim, orig, new):
    """rr.special_rows through the host build (what the GPU suite holds the device to): denormal and huge inputs stay within
    the running bound, whose underflow term is what the denormal row needs; -0.0 inputs give the bits +0.0 inputs give; an
    infinity and a NaN reach the outputs whose window holds them and no other."""
    info, h32, first = rr.sim_plan(sim, orig, new)
    x = rr.special_rows(np.random.default_rng(orig), 3001)
    img, lead, stride, frames = run_sim(sim, orig, new, x, 1, 3)
    y = np.stack([img[lead + r * stride: lead + r * stride + frames] for r in range(len(x))]).view(np.float32)
    assert np.array_equal(img, rr.expected_image(y, img.size, lead, stride))
    ref = rr.resample64(x[:2], orig, new, h=h32, first=first)
    err = np.abs(y[:2].astype(np.float64) - ref)
    assert (err <= rr.running_bound(h32, first, x[:2], orig, new)).all()
    assert (np.abs(y[0][y[0] != 0]) < 2.0 ** -126).sum() > 100 and np.isfinite(y[1]).all() and np.abs(y[1]).max() > 1e37
    plus = x.copy()
    plus[2] = np.where(x[2] == 0, np.float32(0.0), x[2])
    assert np.signbit(x[2][x[2] == 0]).all() and not np.signbit(plus[2][plus[2] == 0]).any()
    img2, _, _, _ = run_sim(sim, orig, new, plus, 1, 3)
    assert np.array_equal(img2[lead + 2 * stride:][:frames], y[2].view(np.uint32))
    # the window of output m is the inputs j * o + first[i] - width + [0, taps): non-finite exactly where it holds a non-finite input
    m = np.arange(frames)
    lo = (m // info["n"]) * info["o"] + first[m % info["n"]] - info["width"]
    hit = np.zeros(frames, bool)
    for at in (len(x[3]) // 3, 2 * len(x[3]) // 3):
        hit |= (lo <= at) & (at < lo + info["taps"])
    assert np.isfinite(y[3][~hit]).all() and np.array_equal(y[3][~hit].view(np.uint32), y[4][~hit].view(np.uint32))
    assert hit.any() and not np.isfinite(y[3][hit]).any()  # a zero tap times an infinity is a NaN


# ---- 3. and 4. the restatement against the truth ----------------------------------------------------------------------
@pytest.mark.parametrize("freq,orig,new", [(1000, 44100, 16000), (1000, 44100, 48000), (5000, 48000, 44100), (3000, 16000, 44100)])
def test_restatement_resamples_a_sine(freq, orig, new):
    T = 4000
    x = np.sin(2 * np.pi * freq * np.arange(T) / orig)
    y = rr.resample64(x, orig, new)
    want = np.sin(2 * np.pi * freq * np.arange(len(y)) / new)
    cut = len(y) // 10
    err = np.abs(y - want)[cut:-cut].max()
    print("%d Hz %d -> %d: %.2e" % (freq, orig, new, err))
    assert err <= 2.5e-3


@pytest.mark.parametrize("orig,new", rr.PAIRS)
def test_constant_input_stays_constant(sim, orig, new):
    """The phases' DC gains are 1.00004 .. 1.00088: away from the edges a constant comes out within 1e-3 of itself."""
    info, h32, first = rr.sim_plan(sim, orig, new)
    T = 40 * info["width"] + 100
    x = np.ones((1, T), np.float32)
    img, lead, stride, frames = run_sim(sim, orig, new, x)
    y = img[lead:lead + frames].view(np.float32)
    edge = frames // 10 + 1
    assert np.abs(y[edge:-edge] - 1.0).max() <= 1e-3
    if info["n"] * (2 * info["width"] + info["o"]) <= 2_000_000:
        assert np.abs(rr.resample64(x, orig, new)[0, edge:-edge] - 1.0).max() <= 1e-3


# ---- 5. arguments and names -------------------------------------------------------------------------------------------
def test_plans_that_cannot_be_built(sim):
    info = np.zeros(5, np.uint32)
    for orig, new, W, rolloff in [(0, 16000, 6, 0.99), (44100, 0, 6, 0.99), (44100, 44100, 6, 0.99), (44100, 16000, 0, 0.99),
                                  (44100, 16000, 6, 0.0), (44100, 16000, 6, -0.5), (44100, 16000, 6, 1.01), (44100, 16000, 6, float("nan")),
                                  (4_000_000, 1, 6, 0.99),                      # 64 outputs do not fit the staging buffer
                                  (3_999_999, 4_000_000, 6, 0.99)]:             # the table is above its cap
        assert sim.resample_sim_plan(orig, new, W, rolloff, info.ctypes.data, None, 0, None, 0) == -2, (orig, new, W, rolloff)
    assert sim.resample_sim_plan(44100, 16000, 6, 1.0, info.ctypes.data, None, 0, None, 0) == 0
    h = np.zeros(4, np.float32)
    assert sim.resample_sim_plan(44100, 16000, 6, 0.99, info.ctypes.data, h.ctypes.data, 4, None, 0) == -2  # capacity


def test_argument_checks(sim):
    T, rows = 100, 3
    frames = rr.out_frames(3, 2, T)
    src = aligned(rows * T + 8, 0)
    dst = aligned(rows * frames + 8, rr.SENTINEL)
    I, O = src.ctypes.data, dst.ctypes.data
    run = lambda *a: sim.resample_sim_run(3, 2, 6, 0.99, *a, 0)  # noqa: E731
    bad = [
        (None, T, rows, T, O, frames), (I, T, rows, T, None, frames),     # NULL buffers with work to do
        (I + 2, T, rows, T, O, frames), (I, T, rows, T, O + 1, frames),   # a base off its 4 bytes
        (I, T - 1, rows, T, O, frames), (I, T, rows, T, O, frames - 1),   # a stride below its row
        (I, 1 << 62, rows, T, O, frames), (I, T, rows, T, O, 1 << 62),    # products that overflow
        (I, 1 << 63, 1, 1 << 63, O, 1 << 63),
    ]
    for a in bad:
        assert run(*a) == -2, a
    assert np.all(dst == rr.SENTINEL)
    assert run(None, 0, 0, T, None, 0) == 0 and run(None, 0, rows, 0, None, 0) == 0  # no work: nothing is touched
    assert run(I, T, 0, T, O, frames) == 0 and run(I, T, rows, 0, O, frames) == 0
    assert np.all(dst == rr.SENTINEL)
    assert run(I, T, rows, T, O, frames) == 0
    assert not dst[:rows * frames].any() and np.all(dst[rows * frames:] == rr.SENTINEL)
    assert sim.resample_sim_out_frames(44100, 16000, 44100) == 16000 and sim.resample_sim_out_frames(44100, 16000, 1) == 1
    assert sim.resample_sim_out_frames(2, 3, (1 << 64) - 1) == 0


def test_entries_reject_before_any_hip_call(pkg):
    """The library itself, on a machine without a GPU: what is refused before the first HIP call."""
    L = pkg.lib()
    rs = ctypes.c_void_p()
    for orig, new, W, rolloff in [(44100, 44100, 6, 0.99), (0, 8000, 6, 0.99), (8000, 0, 6, 0.99), (44100, 16000, 0, 0.99),
                                  (44100, 16000, 6, 0.0), (44100, 16000, 6, 1.5), (4_000_000, 1, 6, 0.99)]:
        assert L.alacgpu_resampler_create(0, orig, new, W, rolloff, ctypes.byref(rs)) == -2 and not rs.value
        assert b"no resampling plan" in L.alacgpu_last_error()
    assert L.alacgpu_resampler_create(0, 44100, 16000, 6, 0.99, None) == -2
    assert L.alacgpu_resample_device(None, 16, 4, 1, 4, 32, 4, 1) == -2
    assert L.alacgpu_resampler_plan(None, None, None, 0, None, 0) == -2
    assert L.alacgpu_resampler_last_ms(None, None) == -2 and L.alacgpu_resampler_synchronize(None) == -2
    assert L.alacgpu_resample_out_frames(None, 100) == 0 and not L.alacgpu_resampler_stream(None)
    L.alacgpu_resampler_destroy(None)
    with pytest.raises(ValueError):
        pkg.NewResampler(44100, 44100)
    assert pkg.resample(np.zeros((2, 5), np.float32), 8000, 8000).shape == (2, 5)  # equal rates: the input, no GPU needed
    with pytest.raises(ValueError):
        pkg.resample(np.zeros((2, 5), np.float64), 8000, 16000)


def test_new_names_in_library_header_and_binding(pkg):
    L = pkg.lib()
    text = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in pkg._EXPORTS, name
    assert "alacgpu_resample_info" in text
    for name in ("Resampler", "NewResampler", "resample"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert pkg.lib().alacgpu_version() == b"alacgpu 0.7.0 gfx950"
