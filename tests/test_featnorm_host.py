"""The feature normalisation pass on the CPU: csrc/alac_featnorm.h built with g++, contraction off
(tests/host_sim/featnorm_sim.cpp), launch for launch, workgroup for workgroup and work item for work item what the gfx950 kernels
of k_featnorm.hip run, against tests/featnorm_ref.py's numpy restatement bit for bit and against float64 within bounds computed
from the data.

* every mode of fr.MODES at the bins 1, 23, 80, 129 and at the wide bins 193, 257, 513, 1025, 4096 (fr.WIDE_BINS: tile_frames 32,
  32, 16, 8 and 2), the frames 1, tile_frames - 1, tile_frames, tile_frames + 1 and 2 * tile_frames + 3, six rows with the lengths
  0, 1, a middle value, frames, -5 and frames + 7, in both layouts, which give the same bits; nothing is cut at the wide bins;
* the means and variances against float64 within fr.mean_bound / fr.var_bound, no free tolerance, at the same
  bins;
* rows and lines padded apart, every base offset, in place, one layout in and the other out; NaN and Inf in the padding and in
  the gaps; canaries around and between everything that is written;
* the affine step and the clamp against the plain numpy expressions; what is refused, by the host build, by the library before
  any HIP call, by the Python class and by the C++ mirror; the structs' sizes; kaldi_frame_counts against the Kaldi pass's own
  frame count; the stand-alone program that the sanitizer runs use; the new names."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import featnorm_ref as fr
from tests import host_build
from tests import kaldi_ref as kr

F32 = np.float32
ROWS = 6


@pytest.fixture(scope="module")
def sim():
    return fr.build_featnorm_sim()


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------
def test_plan_of_every_bin_count(sim):
    """tile_frames is a power of two <= 64, the largest whose image fits, and 64 up to 192 bins; the LDS of every plan stays
    within 51 200 bytes; the bounds of bins"""
    for bins in list(range(1, 300)) + [511, 512, 1023, 2048, 4095, 4096]:
        rc, pl = fr.sim_plan(sim, bins)
        tf = pl["tile_frames"]
        assert rc == 0 and tf == fr.tile_frames_of(bins) and tf & (tf - 1) == 0 and 1 <= tf <= 64
        assert pl["lds_bytes"] == 4 * (((bins * (tf | 1) + 3) & ~3) + 256) <= 51200
        assert tf == 64 or 4 * (bins * (2 * tf | 1) + 256) > 51200
        assert (tf == 64) == (bins <= 192)
    assert fr.sim_plan(sim, 4096)[1]["tile_frames"] == 2
    for bins in (0, 4097, 2 ** 31):
        assert fr.sim_plan(sim, bins)[0] == -2


# ---- 2. bit for bit against the numpy restatement, both layouts ----------------------------------------------------------
@pytest.mark.parametrize("bins", fr.BINS + fr.WIDE_BINS)
@pytest.mark.parametrize("mode", list(fr.MODES))
def test_bits_against_the_reference(sim, mode, bins):
    """The yardstick of tests/test_gpu_featnorm.py: the host build's output and stats [rows][2][bins] are numpy's, at the wide bins
    too, where the device runs other tiles and more than one finishing block"""
    tf = fr.tile_frames_of(bins)
    args = fr.mode_args(mode, bins)
    rng = np.random.default_rng(1000 + bins)
    for frames in fr.frames_of(tf):
        if frames < 1:
            continue
        x = fr.features(rng, ROWS, frames, bins)
        lengths = fr.lengths_of(frames)
        want, want_stats = fr.reference(x, lengths, **args)
        got = {}
        for layout in ("frames", "bins"):
            y, stats = fr.host_values(sim, x, lengths, layout, **args)
            assert fr.same_bits(y, want), "%s, %d frames, layout %s: output" % (mode, frames, layout)
            assert fr.same_bits(stats, want_stats), "%s, %d frames, layout %s: stats" % (mode, frames, layout)
            got[layout] = y
        assert fr.same_bits(got["frames"], got["bins"])
        # a row's result does not depend on the rows around it
        alone, _ = fr.host_values(sim, x[2:3], lengths[2:3], "frames", **args)
        assert fr.same_bits(alone[0], want[2])
        # no lengths: every frame is valid
        full, _ = fr.host_values(sim, x[:2], None, "bins", **args)
        assert fr.same_bits(full, fr.reference(x[:2], None, **args)[0])


# ---- 3. against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", fr.BINS + fr.WIDE_BINS)
def test_mean_and_variance_within_the_float64_bounds(sim, bins):
    """|m - m64| <= gamma(tile_frames + K) sum|x| / n and the variance's analogue (fr.var_bound), per row and bin, from the data"""
    tf = fr.tile_frames_of(bins)
    rng = np.random.default_rng(2000 + bins)
    worst = [0.0, 0.0]
    for frames in fr.frames_of(tf) + (5 * tf + 1,):
        if frames < 1:
            continue
        x = fr.features(rng, ROWS, frames, bins)
        lengths = fr.lengths_of(frames)
        _, stats = fr.host_values(sim, x, lengths, "frames", stat="mean_var", var_floor=1e-30)
        for r, n in enumerate(fr.clamp_lengths(lengths, ROWS, frames)):
            if n == 0:
                continue
            v = x[r, :n]
            v64 = v.astype(np.float64)
            m64 = v64.sum(axis=0) / n
            lim = fr.mean_bound(v, tf)
            err = np.abs(stats[r, 0].astype(np.float64) - m64)
            assert (err <= lim).all(), (frames, r, (err / lim).max())
            worst[0] = max(worst[0], float((err / np.maximum(lim, 1e-300)).max()))
            var64 = ((v64 - m64) ** 2).sum(axis=0) / n
            var32 = fr.chunk_sum((v - stats[r, 0]) * (v - stats[r, 0]), tf) / F32(n)  # what rstd was made of, bit for bit (section 2)
            lim = fr.var_bound(v, stats[r, 0], tf)
            err = np.abs(var32.astype(np.float64) - var64)
            assert (err <= lim).all(), (frames, r, (err / lim).max())
            if n > 1:
                worst[1] = max(worst[1], float((err / lim).max()))
                # and rstd is one division and one root of it
                want = F32(1.0) / np.sqrt(np.where(var32 < F32(1e-30), F32(1e-30), var32))
                assert fr.same_bits(stats[r, 1], want)
    print("bins %d: largest error / bound: mean %.3f, variance %.3f" % (bins, worst[0], worst[1]))


# ---- 4. strides, gaps, canaries, non-finite padding, in place ------------------------------------------------------------
CANARY = F32(-12345.5)


def run_over_buffers(sim, x, lengths, in_layout, out_layout, args, row_gap, inner_gap, lead, poison, in_place=False):
    """x laid out with gaps -> (the output view, stats); asserts that nothing but the output's elements changed"""
    rows, frames, bins = x.shape
    clean = x.copy()
    xin = x.copy()
    if poison is not None:
        for r, n in enumerate(fr.clamp_lengths(lengths, rows, frames)):
            xin[r, n:] = poison
    buf, view, st = fr.lay_out(xin, in_layout, row_gap, inner_gap, lead, fill=CANARY if in_place or poison is None else poison)
    if in_place:
        obuf, oview, ost = buf, view, st
    else:
        obuf, oview, ost = fr.lay_out(np.zeros_like(x), out_layout, row_gap + 1, inner_gap + 2, (lead + 1) % 4, fill=CANARY)
    before = buf.copy()
    stats = np.full((rows, 2, bins), CANARY, F32)
    rc = fr.host_run(sim, bins, view.ctypes.data, st, rows, frames, lengths, oview.ctypes.data, ost, stats, **args)
    assert rc == 0
    olead = (oview.ctypes.data - obuf.ctypes.data) // 4
    rest = fr.outside(obuf, lambda b: fr.view_like(b, olead, x.shape, ost))
    assert rest.size and (rest.view(np.uint32) == CANARY.view(np.uint32)).all(), "an element outside the output was written"
    if not in_place:
        assert np.array_equal(buf.view(np.uint32), before.view(np.uint32)), "the input changed"
    want, want_stats = fr.reference(clean, lengths, **args)
    assert fr.same_bits(oview, want) and fr.same_bits(stats, want_stats)


@pytest.mark.parametrize("bins", fr.BINS)
@pytest.mark.parametrize("mode", ["mean_var", "whisper", "mean_affine", "none_pad"])
def test_gaps_offsets_and_poisoned_padding(sim, mode, bins):
    """Rows a row_gap apart and lines an inner_gap apart at the four base offsets, one layout in and either out, the padded frames
    and every gap of the input NaN or Inf: the result is the clean input's, and nothing around or between the rows is written"""
    tf = fr.tile_frames_of(bins)
    args = fr.mode_args(mode, bins)
    rng = np.random.default_rng(3000 + bins)
    frames = 2 * tf + 3
    x = fr.features(rng, ROWS, frames, bins)
    lengths = fr.lengths_of(frames)
    k = 0
    for in_layout in ("frames", "bins"):
        for out_layout in ("frames", "bins"):
            for lead in range(4):
                poison = (F32(np.nan), F32(np.inf), F32(-np.inf), None)[k % 4]
                k += 1
                run_over_buffers(sim, x, lengths, in_layout, out_layout, args, row_gap=(0, 5, 1, 7)[lead], inner_gap=(0, 3, 1, 2)[lead],
                                 lead=lead, poison=poison)


@pytest.mark.parametrize("bins", fr.BINS)
@pytest.mark.parametrize("mode", ["mean", "mean_var", "max", "affine"])
def test_in_place(sim, mode, bins):
    tf = fr.tile_frames_of(bins)
    args = fr.mode_args(mode, bins)
    rng = np.random.default_rng(4000 + bins)
    for frames in (tf + 1, 2 * tf + 3):
        x = fr.features(rng, ROWS, frames, bins)
        for layout in ("frames", "bins"):
            for lead, gap in ((0, 0), (3, 5)):
                run_over_buffers(sim, x, fr.lengths_of(frames), layout, layout, args, gap, gap, lead, None, in_place=True)


def test_one_frame_and_one_bin_take_either_stride(sim):
    """The stride of an axis of one element is free: [rows, F, 1] with strides (F, 1, 1), [rows, 1, bins] with a frame stride of 1"""
    rng = np.random.default_rng(5)
    x = fr.features(rng, 3, 70, 1)
    want, _ = fr.reference(x, [70, 3, 0], "mean")
    for st in ((70, 1, 1), (70, 1, 70), (70, 1, 99)):
        flat, out = np.ascontiguousarray(x.reshape(-1)), np.zeros(3 * 70, F32)
        assert fr.host_run(sim, 1, flat.ctypes.data, st, 3, 70, [70, 3, 0], out.ctypes.data, st, stat="mean") == 0
        assert fr.same_bits(out.reshape(3, 70, 1), want)
    x = fr.features(rng, 3, 1, 23)
    want, _ = fr.reference(x, [1, 0, 1], "max", range_=1.0)
    for st in ((23, 1, 1), (23, 23, 1), (23, 5, 1)):
        flat, out = np.ascontiguousarray(x.reshape(-1)), np.zeros(3 * 23, F32)
        assert fr.host_run(sim, 23, flat.ctypes.data, st, 3, 1, [1, 0, 1], out.ctypes.data, st, stat="max", range_=1.0) == 0
        assert fr.same_bits(out.reshape(3, 1, 23), want)


# ---- 5. against the plain numpy expressions ------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", fr.BINS)
def test_affine_and_clamp_are_numpys(sim, bins):
    rng = np.random.default_rng(6000 + bins)
    frames = 2 * fr.tile_frames_of(bins) + 3
    x = fr.features(rng, 2, frames, bins)
    shift, scale = rng.uniform(-10, 2, bins).astype(F32), rng.uniform(0.2, 3, bins).astype(F32)
    y, _ = fr.host_values(sim, x, None, "frames", stat="none", shift=shift, scale=scale)
    assert fr.same_bits(y, (x - shift) * scale)
    y, _ = fr.host_values(sim, x, None, "bins", stat="none", scale=scale)
    assert fr.same_bits(y, x * scale)
    y, _ = fr.host_values(sim, x, None, "bins", stat="none")
    assert fr.same_bits(y, x)
    for rng_ in (0.0, 0.5, 8.0):
        y, stats = fr.host_values(sim, x, None, "frames", stat="max", range_=rng_)
        M = x.max(axis=(1, 2), keepdims=True)
        assert fr.same_bits(y, np.maximum(x, M - F32(rng_))) and fr.same_bits(stats[:, 0, 0], M.reshape(-1))
        assert not stats[:, 0, 1:].any() and not stats[:, 1].any() and (rng_ != 0.0 or (y == M).all())
    # Whisper's (max(x, M - 8) + 4) / 4
    y, _ = fr.host_values(sim, x, None, "bins", stat="max", range_=8.0, shift=np.full(bins, -4, F32), scale=np.full(bins, 0.25, F32))
    assert fr.same_bits(y, (np.maximum(x, x.max(axis=(1, 2), keepdims=True) - F32(8.0)) + F32(4.0)) / F32(4.0))


def test_max_ignores_nan_and_orders_zeros(sim):
    x = np.array([[[-0.0, 0.0], [np.nan, -3.0]], [[np.nan, np.nan], [np.nan, np.nan]]], F32)
    y, stats = fr.host_values(sim, x, None, "frames", stat="max", range_=1.0)
    assert stats[0, 0, 0] == 0.0 and not np.signbit(stats[0, 0, 0]) and stats[1, 0, 0] == -np.inf
    assert np.isnan(y[0, 1, 0]) and y[0, 1, 1] == -1.0 and np.isnan(y[1]).all()


# ---- 6. what is refused --------------------------------------------------------------------------------------------------
def test_refusals_of_the_host_build(sim):
    x = np.zeros(4 * 10 * 8 + 64, F32)
    out = np.full(x.shape, CANARY, F32)

    def run(strides=(80, 8, 1), ostrides=(80, 8, 1), rows=4, frames=10, bins=8, inp=x, outp=out, **kw):
        return fr.host_run(sim, bins, None if inp is None else inp.ctypes.data, strides, rows, frames, None,
                           None if outp is None else outp.ctypes.data, ostrides, **kw)

    assert run() == 0
    for bad in (dict(bins=0), dict(bins=4097), dict(var_floor=0.0), dict(var_floor=-1.0), dict(var_floor=float("nan")),
                dict(stat="max", range_=-1.0), dict(stat="max", range_=float("nan")), dict(inp=None), dict(outp=None),
                dict(strides=(80, 8, 2)), dict(ostrides=(160, 16, 2)), dict(strides=(79, 8, 1)), dict(ostrides=(79, 8, 1)),
                dict(strides=(80, 7, 1)), dict(strides=(80, 1, 9)), dict(strides=(79, 1, 10)), dict(strides=(2 ** 62, 8, 1))):
        out[...] = CANARY
        assert run(**bad) == -2, bad
        assert (out == CANARY).all()
    assert run(stat="mean", range_=-1.0) == 0, "range is read with stat max only"
    assert fr.STATS["max"] == 3 and sim.featnorm_sim_run(8, 4, 1e-20, 0.0, 0.0, None, None, x.ctypes.data, 80, 8, 1, 4, 10, None,
                                                         out.ctypes.data, 80, 8, 1, None) == -2, "an unknown stat"
    out[...] = CANARY
    assert run(rows=0) == 0 and run(frames=0) == 0 and run(rows=0, inp=None, outp=None) == 0 and (out == CANARY).all()


def test_refusals_of_the_library_and_its_mirrors(pkg):
    """alacgpu_norm_create refuses before any HIP call (this runs without a GPU), and so do the Python class, the functional entry
    and the C++ mirror; a NULL handle is refused by every entry"""
    pkg.build()
    L = pkg.lib()
    h = ctypes.c_void_p()
    for cfg in (pkg.NormConfig(0, 1, 1e-20, 0, 0), pkg.NormConfig(4097, 1, 1e-20, 0, 0), pkg.NormConfig(80, 4, 1e-20, 0, 0),
                pkg.NormConfig(80, 3, 1e-20, -1.0, 0), pkg.NormConfig(80, 3, 1e-20, float("nan"), 0), pkg.NormConfig(80, 1, 0.0, 0, 0),
                pkg.NormConfig(80, 0, -1.0, 0, 0)):
        assert L.alacgpu_norm_create(0, ctypes.byref(cfg), None, None, ctypes.byref(h)) == -2 and not h
        assert b"no normalisation plan" in L.alacgpu_last_error()
    assert L.alacgpu_norm_create(0, None, None, None, ctypes.byref(h)) == -2
    assert L.alacgpu_norm_create(0, ctypes.byref(pkg.NormConfig(80, 1, 1e-20, 0, 0)), None, None, None) == -2
    ms = ctypes.c_float()
    assert L.alacgpu_norm_device(None, 16, 80, 8, 1, 1, 10, None, 16, 80, 8, 1, None, 1) == -2
    assert L.alacgpu_norm_last_ms(None, ctypes.byref(ms)) == -2 and L.alacgpu_norm_synchronize(None) == -2
    assert L.alacgpu_norm_plan(None, ctypes.byref(pkg.NormInfo()), None, 0, None, 0) == -2
    assert L.alacgpu_norm_out_frames(None, 7) == 0 and not L.alacgpu_norm_stream(None)
    L.alacgpu_norm_destroy(None)
    for kw in (dict(bins=0), dict(bins=4097), dict(bins=80, stat="std"), dict(bins=80, stat=2), dict(bins=80, stat="max"),
               dict(bins=80, stat="max", range=-1.0), dict(bins=80, var_floor=0.0), dict(bins=80, shift=[1.0, 2.0]),
               dict(bins=80.5), dict(bins=True)):
        with pytest.raises(ValueError):
            pkg.NewFeatureNorm(**kw)
    S = fr.build_featnorm_shim(pkg)
    sizes = np.zeros(3, np.uint64)
    S.featnorm_shim_sizes(sizes.ctypes.data)
    assert ctypes.sizeof(pkg.NormConfig) == sizes[0] == 20 and ctypes.sizeof(pkg.NormInfo) == sizes[1] == 40
    assert pkg.NormInfo.scratch_bytes.offset == sizes[2] == 24
    assert S.featnorm_shim_create(ctypes.byref(pkg.NormConfig(0, 1, 1e-20, 0, 0)), None, 0, None, 0) == -6
    assert b"no normalisation plan" in S.featnorm_shim_last_error()
    three = np.zeros(3, F32)
    assert S.featnorm_shim_create(ctypes.byref(pkg.NormConfig(80, 1, 1e-20, 0, 0)), three.ctypes.data, 3, None, 0) == -6
    assert b"one float per bin" in S.featnorm_shim_last_error()


# ---- 7. kaldi_frame_counts -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,h", [(400, 160), (1200, 480)])
@pytest.mark.parametrize("snip", [True, False])
def test_frame_counts_are_the_kaldi_passes(pkg, W, h, snip):
    """Every length from 0 to 3 W against the Kaldi pass's formula (kr.out_frames), and that formula against alacfb::out_frames_of,
    which alacgpu_fbank_out_frames returns, around every value at which the count changes near W (each such call builds a plan);
    tests/test_gpu_featnorm.py asks a handle for every value"""
    import torch
    S = kr.build_fbank_sim()
    cfg = kr.Cfg(W * 40, W, h, snip=snip)
    T = np.arange(0, 3 * W + 1)
    want = np.array([kr.out_frames(cfg, int(t)) for t in T], np.int64)
    for t in (0, 1, W - 1, W, W + 1, W + h - 1, W + h, W + h + 1, 2 * W, 3 * W - 1, 3 * W):
        assert kr.sim_out_frames(S, cfg, t) == want[t]
    for lengths in (torch.from_numpy(T.astype(np.int32)), torch.from_numpy(T), T.tolist()):
        got = pkg.kaldi_frame_counts(lengths, W, h, snip_edges=snip)
        assert got.dtype is torch.int32 and np.array_equal(got.numpy(), want)
    with pytest.raises(ValueError):
        pkg.kaldi_frame_counts(torch.zeros(3), W, h)
    with pytest.raises(ValueError):
        pkg.kaldi_frame_counts(torch.zeros(3, dtype=torch.int32), W, 0)


# ---- 8. the stand-alone program ------------------------------------------------------------------------------------------
def test_standalone_program_builds_and_runs(tmp_path):
    """tests/host_sim/featnorm_san_main.cpp, the program with its own main over featnorm_sim.cpp's functions that DESIGN.md §16
    runs under the sanitizers on a CPU: here it is built plainly and run once, so that it stays in step with the header"""
    exe = str(tmp_path / "featnorm_san")
    host_build.compile("featnorm_san_main.cpp", exe,
                       ["-O1", "-ffp-contract=off", "-fwrapv", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count("-> 0,") == 4 * 4 * 2 * 2 and "nan" not in r.stdout.lower()


# ---- 9. the names --------------------------------------------------------------------------------------------------------
def test_names_in_library_and_binding(pkg):
    import inspect
    for name in ("NormConfig", "FeatureNorm", "NewFeatureNorm", "normalize_features", "kaldi_frame_counts", "load_features"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("create", "destroy", "stream", "synchronize", "last_ms", "out_frames", "device", "plan"):
        assert "alacgpu_norm_" + name in pkg._EXPORTS
    assert issubclass(pkg.FeatureNorm, pkg._RowPass)
    assert list(inspect.signature(pkg.NewFeatureNorm).parameters) == ["bins", "stat", "shift", "scale", "var_floor", "range", "pad_value",
                                                                     "device"]
    assert list(inspect.signature(pkg.FeatureNorm.__call__).parameters) == ["self", "feats", "lengths", "layout", "out", "return_stats"]
    par = inspect.signature(pkg.load_features).parameters
    assert list(par)[:8] == ["sources", "frame_offsets", "num_frames", "sample_rate", "kind", "norm", "channel", "transform"]
    assert par["sample_rate"].default == 16000 and par["norm"].default == "mean" and par["kind"].default == "fbank"
    mk = open(os.path.join(fr.ROOT, "saprobe-alac_amd", "csrc", "Makefile")).read()
    assert "k_featnorm" in mk.split("UNITS =")[1].split("\n")[0] and "build/k_featnorm.o: alac_featnorm.h" in mk
    assert b"alacgpu 0.7.0 gfx950" == pkg.lib().alacgpu_version()
