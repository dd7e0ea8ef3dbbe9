"""The resampler on the CPU: csrc/alac_resample.h built with g++ (tests/host_sim/resample_sim.cpp), tile for tile and work
item for work item what the gfx950 kernel of k_resample.hip runs, against the numpy float64 restatement of
tests/resample_ref.py.

* the plan (o, n, width, the float32 window table, the window starts) against the full double table, for every pair the plan
  must accept;
* a sweep over ratios, row counts, lengths around the filter width and the tile boundaries, and every input and output
  base offset of 0..3 elements with odd row strides: the WHOLE sentinel-filled output buffer is compared, the sentinel outside
  the rows' columns [0, out_frames), inside them the float32 dot-product bound against the restatement run on the plan's own
  table; once more with the input ending at an inaccessible page;
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
@pytest.mark.parametrize("orig,new", SWEEP)
def test_host_build_within_the_bound_over_the_whole_buffer(sim, orig, new):
    info, h32, first = rr.sim_plan(sim, orig, new)
    rng = np.random.default_rng(orig * 7 + new)
    worst = 0.0
    for rows in (1, 5):
        for T in rr.boundary_frames(info, orig, new):
            x = rr.signal(rng, rows, T)
            ref = rr.resample64(x, orig, new, h=h32, first=first)
            lim = rr.bound(h32, first, x, orig, new)
            images = set()
            for in_off in range(4):
                for out_off in range(4):
                    img, lead, stride, frames = run_sim(sim, orig, new, x, in_off, out_off, guard=int(in_off == 1))
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
                    with np.errstate(divide="ignore", invalid="ignore"):
                        worst = max(worst, float(np.nanmax(np.where(lim > 0, err / lim, 0.0))))
            assert len(images) == 1, "the values depend on the alignment"
    print("%d -> %d: worst error / bound %.3f" % (orig, new, worst))


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
