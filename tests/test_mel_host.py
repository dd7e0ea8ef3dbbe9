"""The spectrogram pass on the CPU: csrc/alac_mel.h built with g++, contraction off (tests/host_sim/mel_sim.cpp), tile for tile
and work item for work item what the gfx950 kernel of k_mel.hip runs, against the numpy float64 restatement of tests/mel_ref.py.

* the restatement itself, and the header's frame count, against torch.stft in float64;
* the plan (dimensions, window starts, the float32 tables) against the restatement;
* the host build over whole sentinel-filled buffers, every base offset, odd strides, a bin stride above F, NaN between the input
  rows and the input ending at an inaccessible page: the sentinel outside [rows, bins, F], inside it the derived ceiling of the
  float32 chains against the restatement run on the plan's own tables;
* mr.EDGE_CASES, the parameter sets at which the header takes another path (dft_blocks<4>, hop > n_fft, the DFT loop's tail, ...);
* impulses, which come out as single table entries: a batch of rows, one impulse each, at every n of a frame;
* the arguments the entries reject, whisper_log_mel's post-processing, and the new names in library, header and binding.

The library's own plan needs a handle, so it is held against the host build's in tests/test_gpu_mel.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import mel_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alacgpu_mel_create", "alacgpu_mel_destroy", "alacgpu_mel_stream", "alacgpu_mel_synchronize", "alacgpu_mel_last_ms",
         "alacgpu_mel_out_frames", "alacgpu_mel_device", "alacgpu_mel_plan"]


@pytest.fixture(scope="module")
def sim():
    return mr.build_mel_sim()


# ---- 1. the restatement ------------------------------------------------------------------------------------------------
STFT_CASES = [(400, 160, 400, True), (16, 4, 12, True), (1024, 256, 1024, True), (15, 4, 9, True), (3, 1, 3, True), (2, 1, 2, True),
              (6, 2, 6, False), (64, 24, 48, False), (16, 37, 16, True), (16, 37, 16, False), (30, 7, 11, True), (8, 3, 1, True),
              (2047, 1024, 2047, True)]


@pytest.mark.parametrize("N,h,W,center", STFT_CASES)
def test_restatement_against_torch_stft(sim, N, h, W, center):
    """Two lengths: 5 max(N, h) + 37, and the multiple of h below it, where an odd N's frame count differs from 1 + T / h. The
    host build's frame count is torch's too."""
    import torch
    cfg = mr.Cfg(16000, N, h, W, center=center)
    rng = np.random.default_rng(N)
    T0 = 5 * max(N, h) + 37
    for T in (T0, T0 // h * h):
        x = rng.uniform(-1, 1, (2, T))
        got = mr.power64(cfg, x)
        win = torch.hann_window(W, periodic=True, dtype=torch.float64)
        X = torch.stft(torch.from_numpy(x), N, hop_length=h, win_length=W, window=win, center=center, pad_mode="reflect",
                       return_complex=True)
        want = (X.abs() ** 2).numpy()
        F = 1 + (T - N % 2) // h if center else 1 + (T - N) // h
        assert got.shape == want.shape == (2, N // 2 + 1, F) and mr.out_frames(cfg, T) == F
        assert mr.sim_out_frames(sim, cfg, T) == want.shape[2], "the header's frame count is not torch.stft's"
        assert T % h or N % 2 == 0 or not center or F == T // h, "an odd n_fft has no frame at T itself"
        err = np.abs(got - want).max() / want.max()
        print("N %d hop %d W %d T %d: %.3g of the largest bin" % (N, h, W, T, err))
        assert err <= 1e-6


def test_restatement_fbanks_against_closed_forms():
    """The triangles: every filter peaks at or below 1 (2 / width with the slaney norm) and the peaks walk up the bins."""
    cfg = mr.CASES["htk128"]
    fb = mr.fbanks(cfg)
    assert fb.shape == (201, 128) and fb.min() == 0.0 and fb.max() <= 1.0
    empty = np.nonzero(~fb.any(axis=0))[0]
    print("filters without a weight:", empty)
    assert len(empty) == 4, "n_mels 128 at n_fft 400 has four filters without a weight"
    top = fb.argmax(axis=0)[fb.any(axis=0)]
    assert (np.diff(top) >= 0).all() and top[-1] >= 195, "the peaks walk up the bins to f_max"
    sl = mr.fbanks(mr.CASES["whisper80"])
    assert sl.shape == (201, 80) and sl.any(axis=0).all() and 0.0 < sl.max() < 0.03


# ---- 2. the plan -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mr.CASES) + ["power", "short_window"] + list(mr.EDGE_CASES))
def test_plan_against_the_restatement(sim, name):
    cfg = mr.CASES.get(name) or {"power": mr.Cfg(16000, 400, 160), "short_window": mr.Cfg(8000, 30, 7, 11, n_mels=4)}.get(name)
    plan = mr.sim_plan(sim, cfg or mr.EDGE_CASES[name][0])
    assert plan is not None, "no plan"
    if cfg is None:
        cfg, tf = mr.EDGE_CASES[name]
        assert plan["tile_frames"] == tf
    N, W, K = cfg.n_fft, cfg.win_length, cfg.K
    assert (plan["n_fft"], plan["win_length"], plan["hop_length"], plan["n_freqs"], plan["bins"]) == (N, W, cfg.hop_length, K, cfg.bins)
    tf = plan["tile_frames"]
    assert tf in (4, 8, 16, 32, 64) and plan["lds_bytes"] <= 4 * sim.mel_sim_lds_floats()
    want = mr.basis(N, W)
    got = plan["basis"]
    assert got.shape == want.shape
    # within one float32 ulp of the double value (libm's and numpy's cos may differ in the last double bit)
    assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).all()
    zero = mr.window(N, W) == 0.0  # outside the window, and the periodic Hann's sample 0 (win_length 1 is [1.0]: none inside)
    assert zero[(N - W) // 2] == (W > 1) and zero.sum() == (N - W + 1 if W > 1 else N - W)
    assert not got[:, :, zero].view(np.uint32).any(), "a window zero is not +0.0 in the table"
    assert not got[1, 0].view(np.uint32).any(), "sin(0) is not +0.0"
    if cfg.n_mels is None:
        assert plan["n_mels"] == 0 and plan["taps"] == 0
        return
    fb = mr.fbanks(cfg)
    first, taps, fbw = mr.windows_of(fb.astype(np.float32))
    assert plan["n_mels"] == cfg.n_mels and plan["taps"] == taps and np.array_equal(plan["first"], first)
    assert (np.abs(plan["fb"].astype(np.float64) - fbw) <= np.spacing(np.abs(fbw))).all()
    assert np.array_equal(plan["fb"] == 0.0, fbw == 0.0) and not plan["fb"][fbw == 0.0].view(np.uint32).any()
    dense = mr.dense_fb(plan, K)
    assert np.array_equal(dense == 0.0, fb.astype(np.float32) == 0.0), "a weight outside its triangle"


def test_tile_frames_follow_the_lds_budget(sim):
    for cfg, tf in ((mr.CASES["tiny"], 64), (mr.CASES["whisper80"], 32), (mr.CASES["n1024"], 16), (mr.Cfg(48000, 2048, 2048), 4),
                    (mr.Cfg(48000, 2048, 5000), 4), (mr.Cfg(48000, 2048, 512, n_mels=64), 8)) + tuple(mr.EDGE_CASES.values()):
        assert mr.sim_plan(sim, cfg)["tile_frames"] == tf
    assert mr.sim_plan(sim, mr.EDGE_CASES["n2046u"][0])["lds_bytes"] == 60608


# ---- 3. the host build against the restatement ------------------------------------------------------------------------
def check_image(cfg, plan, x, img, lay, what):
    """The whole buffer: the sentinel outside [rows, bins, F], inside it the ceilings of mr.bounds."""
    got = mr.values_of(img, lay, cfg, x.shape[0], x.shape[1], what)
    return mr.ceiling_share(cfg, plan, x, got, what)


def lengths(cfg, tf):
    """T for F = tile_frames - 1, tile_frames, tile_frames + 1 and 1 (where a row that short has frames), and the shortest row"""
    Ts = {mr.length_for(cfg, F) for F in (tf - 1, tf, tf + 1, 1)}
    Ts.add(cfg.n_fft // 2 + 1 if cfg.center else cfg.n_fft)
    return sorted(Ts)


@pytest.mark.parametrize("name", ["tiny", "uncentred", "whisper80"])
def test_host_build_against_the_restatement(sim, name):
    cfg = mr.CASES[name]
    plan = mr.sim_plan(sim, cfg)
    rng = np.random.default_rng(len(name))
    small = cfg.n_fft <= 64
    worst = 0.0
    for cfg_, plan_ in ((cfg, plan), (cfg.with_(n_mels=None, mel_scale=None, norm=None), None)):
        plan_ = plan_ or mr.sim_plan(sim, cfg_)
        for rows in (1, 5) if small else (2,):
            for T in lengths(cfg, plan["tile_frames"]) if small else [mr.length_for(cfg, plan["tile_frames"] + 1), cfg.n_fft // 2 + 1]:
                x = mr.signal(rng, rows, T)
                assert mr.sim_out_frames(sim, cfg_, T) == mr.out_frames(cfg_, T) > 0
                for out_off, in_off in mr.OFFSETS if small else mr.OFFSETS[1:2]:
                    for bin_pad in (0, 3) if small else (3,):
                        img, lay = mr.sim_image(sim, cfg_, x, in_off, out_off, bin_pad, guard=1)
                        worst = max(worst, check_image(cfg_, plan_, x, img, lay, "%s rows %d T %d offsets %d/%d pad %d"
                                                       % (name, rows, T, in_off, out_off, bin_pad)))
    print("%s: at most %.1f %% of the ceiling" % (name, 100 * worst))


def test_hop_above_n_fft_and_odd_sizes(sim):
    """hop > n_fft (the frames are staged one behind the other), an odd n_fft, K even (n_fft 6), win_length 1"""
    rng = np.random.default_rng(3)
    for cfg in (mr.Cfg(8000, 16, 37, 16, n_mels=3), mr.Cfg(8000, 15, 4, 9), mr.Cfg(8000, 6, 2, 6, n_mels=2, center=False),
                mr.Cfg(8000, 8, 3, 1)):
        plan = mr.sim_plan(sim, cfg)
        for T in (cfg.n_fft, 200, 64 * cfg.hop_length + 5):
            x = mr.signal(rng, 3, T)
            for out_off, in_off in mr.OFFSETS[:2]:
                img, lay = mr.sim_image(sim, cfg, x, in_off, out_off, 1, guard=1)
                check_image(cfg, plan, x, img, lay, "n_fft %d hop %d T %d" % (cfg.n_fft, cfg.hop_length, T))


@pytest.mark.parametrize("name", list(mr.EDGE_CASES))
def test_edge_cases_against_the_restatement(sim, name):
    """mr.EDGE_CASES, each at the tile_frames the table gives: rows 1 and 3; F = tile_frames + 1, the shortest row and F =
    tile_frames; up to n_fft 128 every offset pair of mr.OFFSETS with bin strides F and F + 3, above it one pair and the first
    two lengths."""
    cfg, tf = mr.EDGE_CASES[name]
    plan = mr.sim_plan(sim, cfg)
    assert plan["tile_frames"] == tf
    rng = np.random.default_rng(len(name) + cfg.n_fft)
    small = name in mr.SMALL_EDGES
    worst = 0.0
    for rows in (1, 3):
        for T in mr.edge_lengths(cfg, tf):
            x = mr.signal(rng, rows, T)
            assert mr.sim_out_frames(sim, cfg, T) == mr.out_frames(cfg, T) > 0
            for out_off, in_off in mr.OFFSETS if small else mr.OFFSETS[1:2]:
                for bin_pad in (0, 3) if small else (3,):
                    img, lay = mr.sim_image(sim, cfg, x, in_off, out_off, bin_pad, guard=1)
                    worst = max(worst, check_image(cfg, plan, x, img, lay, "%s rows %d T %d offsets %d/%d pad %d"
                                                   % (name, rows, T, in_off, out_off, bin_pad)))
    print("%s: tile_frames %d, at most %.1f %% of the ceiling" % (name, tf, 100 * worst))


@pytest.mark.parametrize("name", mr.IMPULSE_CASES)
def test_impulse_at_every_n(sim, name):
    """One launch over a batch of rows, row r of +0.0 with 1.0 at js[r]: every frame that reads js[r] holds fmaf(S, S, C * C) of
    the table's entries under it, every other power is +0.0, the whole buffer compared as uint32. A frame's n that the DFT loop
    dropped, staged from a neighbouring index or took from another row shows here even where the window is 1e-6 there, which
    the ceilings let pass."""
    cfg, tf, T, js = mr.impulse_batch(name)
    plan = mr.sim_plan(sim, cfg)
    assert plan["tile_frames"] == tf
    want, twice, silent = mr.impulse_image(cfg, plan["basis"], T, js)
    if cfg.n_fft < 2048:  # the positions of the large cases lie inside the row, away from both margins
        assert (twice > 0) == (cfg.center and cfg.n_fft >= 3), "the reflected margin shows an impulse twice"
    if name == "hop37":
        assert silent > 0, "no impulse lies between two frames"
    x = mr.impulse_rows(T, js)
    img, lay = mr.sim_image(sim, cfg, x, 1, 2, 1)
    bad = np.nonzero(img != mr.expected_image(want, img.size, lay[5], lay[3], lay[4]))[0]
    assert not len(bad), "%s: %d words differ, the first in the row of the impulse at %d" % (name, len(bad), js[(bad[0] - lay[5]) // lay[3]])


def test_impulses_come_out_as_single_table_entries(sim):
    """x = delta at j: re[k] and im[k] of a frame are the table's entries under j, the power fmaf(S, S, C * C) of them exactly; an
    impulse inside the reflected margin is seen twice by the first frames, one near the end twice by the last."""
    cfg = mr.CASES["tiny"].with_(n_mels=None, mel_scale=None, norm=None)
    plan = mr.sim_plan(sim, cfg)
    T = 100
    for j, amp, margin in ((40, 1.0, False), (3, 1.0, True), (97, -0.5, True)):
        x = np.zeros((1, T), np.float32)
        x[0, j] = amp
        img, lay = mr.sim_image(sim, cfg, x, 1, 2)
        F = mr.out_frames(cfg, T)
        got = mr.rows_of(img, 1, cfg.K, F, lay[5], lay[3], lay[4])[0]
        want, twice = mr.impulse_expected(cfg, plan["basis"], T, j, amp)
        assert (twice > 0) == margin and np.count_nonzero(want) > 0
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "impulse at %d" % j


def test_log_modes_on_the_host(sim):
    """libm against float64: logf within 1 ulp and log10f within 2 (what glibc documents for them), db within 3 (log10f's 2, ten
    times an error being ten times as many of the product's own ulps at worst 2.5, and the product's rounding); values at or below
    the floor give float(s log(floor)) exactly. The device's own log is measured and bounded in tests/test_gpu_mel.py."""
    rng = np.random.default_rng(9)
    base = mr.CASES["tiny"]
    x = mr.signal(rng, 3, 150)
    x[1, 20:120] = 0.0  # frames of silence: at the floor
    P = None
    for log in (None, "ln", "log10", "db"):
        for floor in (1e-10, 1e-3):
            cfg = base.with_(log=log, floor=floor)
            img, lay = mr.sim_image(sim, cfg, x, 0, 0)
            got = mr.rows_of(img, 3, cfg.bins, mr.out_frames(cfg, 150), lay[5], lay[3], lay[4])
            if log is None:
                P = got
                continue
            want = mr.log64(cfg, P)
            low = P <= np.float32(floor)
            assert low.any() and (~low).any()
            assert np.array_equal(got[low], want[low].astype(np.float32))
            assert mr.ulps32(got[~low], want[~low]).max() <= {"ln": 1.0, "log10": 2.0, "db": 3.0}[log]


# ---- 4. refusals -------------------------------------------------------------------------------------------------------
BAD = [dict(n_fft=1), dict(n_fft=2049), dict(win_length=401), dict(win_length=0), dict(hop_length=0), dict(f_min=8000.0),
       dict(f_min=9000.0), dict(f_min=-1.0), dict(n_mels=0), dict(floor=0.0), dict(floor=-1.0), dict(floor=1e-60),
       dict(sample_rate=0), dict(f_max=float("nan"))]


def test_plans_refused(sim, pkg):
    good = mr.CASES["whisper80"]
    assert mr.sim_plan(sim, good) is not None
    L = pkg.lib()
    for kw in BAD:
        cfg = good.with_(**kw)
        assert mr.sim_plan(sim, cfg) is None, kw
        if "n_mels" not in kw:
            with pytest.raises(ValueError, match="no spectrogram plan"):
                pkg.NewMelSpectrogram(**cfg.kwargs())
    with pytest.raises(ValueError):
        pkg.NewMelSpectrogram(16000, n_mels=0)
    w, d = good.words()
    for at, v in ((5, 2), (6, 2), (7, 3), (8, 4)):  # center, norm, mel_scale, log outside their values
        ww = w.copy()
        ww[at] = v
        info = np.zeros(9, np.uint32)
        assert sim.mel_sim_plan(ww.ctypes.data, d.ctypes.data, info.ctypes.data, None, 0, None, 0, None, 0) == -2
        c = pkg.MelConfig(*[int(u) for u in ww[:4]], d[0], d[1], int(ww[4]), int(ww[5]), int(ww[6]), int(ww[7]), int(ww[8]), 0, d[2])
        h = ctypes.c_void_p()
        assert L.alacgpu_mel_create(0, ctypes.byref(c), ctypes.byref(h)) == -2 and not h.value
        assert b"no spectrogram plan" in L.alacgpu_last_error()
    for kw in (dict(mel_scale="bark"), dict(norm="l2"), dict(log="log2"), dict(n_fft=400.5), dict(hop_length=-1)):
        with pytest.raises(ValueError):
            pkg.NewMelSpectrogram(16000, **kw)
    # no mel scale: n_mels and norm must be 0
    ww = w.copy()
    ww[7] = 0
    info = np.zeros(9, np.uint32)
    assert sim.mel_sim_plan(ww.ctypes.data, d.ctypes.data, info.ctypes.data, None, 0, None, 0, None, 0) == -2
    # NULLs and the entries on a NULL handle: before any HIP call
    h = ctypes.c_void_p()
    assert L.alacgpu_mel_create(0, None, ctypes.byref(h)) == -2 and L.alacgpu_mel_create(0, ctypes.byref(pkg.MelConfig()), None) == -2
    assert L.alacgpu_mel_device(None, 16, 4, 1, 4, 32, 4, 4, 1) == -2
    assert L.alacgpu_mel_plan(None, None, None, 0, None, 0, None, 0) == -2
    assert L.alacgpu_mel_last_ms(None, None) == -2 and L.alacgpu_mel_synchronize(None) == -2
    assert L.alacgpu_mel_out_frames(None, 1000) == 0 and not L.alacgpu_mel_stream(None)
    L.alacgpu_mel_destroy(None)
    for bad in (np.zeros((2, 500), np.float64), [0.0] * 500):
        with pytest.raises(ValueError):
            pkg.mel_spectrogram(bad, 16000)


def test_pass_arguments_refused(sim):
    cfg = mr.CASES["tiny"]
    rows, T = 2, 40
    F, bins = mr.out_frames(cfg, T), cfg.bins
    src = mr.aligned(rows * T + 8, 0)
    dst = mr.aligned(rows * bins * F + 8, mr.SENTINEL)
    I, O = src.ctypes.data, dst.ctypes.data
    w, d = cfg.words()
    run = lambda *a: sim.mel_sim_run(w.ctypes.data, d.ctypes.data, *a, 0)  # noqa: E731
    bad = [
        (None, T, rows, T, O, bins * F, F), (I, T, rows, T, None, bins * F, F),           # NULL buffers with work to do
        (I + 2, T, rows, T, O, bins * F, F), (I, T, rows, T, O + 1, bins * F, F),         # a base off its 4 bytes
        (I, T - 1, rows, T, O, bins * F, F), (I, T, rows, T, O, bins * F, F - 1),         # strides below what they span
        (I, T, rows, T, O, bins * F - 1, F), (I, T, rows, T, O, bins * (F + 1) - 2, F + 1),
        (I, 1 << 62, rows, T, O, bins * F, F), (I, T, rows, T, O, 1 << 62, F),            # products that overflow
        (I, T, rows, T, O, 1 << 63, 1 << 62), (I, 1 << 63, 1, 1 << 62, O, 1 << 63, 1 << 62),
    ]
    for a in bad:
        assert run(*a) == -2, a
    assert np.all(dst == mr.SENTINEL)
    assert run(None, 0, 0, T, None, 0, 0) == 0 and run(None, 0, rows, 8, None, 0, 0) == 0  # no rows, no frames: nothing is touched
    assert run(I, T, rows, cfg.n_fft // 2, O, bins * F, F) == 0
    assert np.all(dst == mr.SENTINEL)
    assert run(I, T, rows, T, O, bins * F, F) == 0
    assert not dst[:rows * bins * F].any() and np.all(dst[rows * bins * F:] == mr.SENTINEL)
    for c, T_, F_ in ((cfg, 8, 0), (cfg, 9, 3), (cfg, 1 << 62, 0), (mr.CASES["uncentred"], 63, 0), (mr.CASES["uncentred"], 64, 1),
                      (mr.CASES["uncentred"], 88, 2)):
        assert mr.sim_out_frames(sim, c, T_) == F_


# ---- 5. whisper's post-processing, and the names ------------------------------------------------------------------------
def test_whisper_post_processing(pkg):
    import torch
    rng = np.random.default_rng(4)
    x = rng.uniform(-10.0, 2.0, (3, 80, 26)).astype(np.float32)
    x[1, :, -1] = 50.0  # the dropped frame does not set the maximum
    got = pkg.whisper_post(torch.from_numpy(x)).numpy()
    want = mr.whisper_post(x)
    assert got.shape == (3, 80, 25) and np.array_equal(got, want)
    for r in range(3):
        top = x[r, :, :-1].max()
        assert got[r].max() == (top + np.float32(4)) / np.float32(4) and got[r].min() >= (top - 8 + 4) / 4 - 1e-6
    one = pkg.whisper_post(torch.from_numpy(x[0])).numpy()
    assert np.array_equal(one, want[0])


def test_new_names_in_library_header_and_binding(pkg):
    L = pkg.lib()
    text = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in pkg._EXPORTS, name
    assert "alacgpu_mel_config" in text and "alacgpu_mel_info" in text
    for name in ("MelSpectrogram", "NewMelSpectrogram", "mel_spectrogram", "spectrogram", "whisper_log_mel"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert ctypes.sizeof(pkg.MelConfig) == 64 and pkg.MelConfig.floor.offset == 56
    assert pkg.lib().alacgpu_version() == b"alacgpu 0.7.0 gfx950"
