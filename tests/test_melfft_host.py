"""The spectrogram pass with transform="fft" on the CPU: csrc/alac_melfft.h built with g++, contraction off
(tests/host_sim/melfft_sim.cpp), tile for tile and work item for work item what the gfx950 kernel of k_melfft.hip runs, against
the numpy float64 restatement of tests/melfft_ref.py (np.fft.rfft over the float32 window) within the derived ceilings.

* the plan: radices, tables, LDS, tile_frames, per accepted size; the sizes that have no plan;
* the host build over whole sentinel-filled buffers at every case of fr.FFT_CASES (each radix alone, every pair, repeated ones,
  no pass at all, short windows, hop > n_fft, the sizes at which the transform buffer holds fewer frames than the tile);
* impulses; the FFT result against the direct pass's host build; the stand-alone program that the sanitizer runs use;
* the new names in library source, header and binding.

The library's own plan needs a handle, so it is held against the host build's in tests/test_gpu_melfft.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import host_build
from tests import mel_ref as mr
from tests import melfft_ref as fr

ROOT = fr.ROOT


@pytest.fixture(scope="module")
def sim():
    return fr.build_melfft_sim()


@pytest.fixture(scope="module")
def direct_sim():
    return mr.build_mel_sim()


# ---- 1. the plan -------------------------------------------------------------------------------------------------------
ACCEPTED = [n for n in range(2, 2049) if fr.size_ok(n)]


def check_plan(cfg, pl):
    N, M = cfg.n_fft, cfg.n_fft // 2
    assert pl["transform"] == 1
    assert int(np.prod(pl["radix"], dtype=np.int64)) == M and all(r in (2, 3, 4, 5) for r in pl["radix"]) and pl["n_passes"] == len(pl["radix"])
    assert pl["radix"] == sorted(pl["radix"], key=lambda r: {5: 0, 3: 1, 4: 2, 2: 3}[r]) and pl["radix"].count(2) <= 1
    tf, batch = pl["tile_frames"], pl["batch_frames"]
    assert tf >= 4 and tf & (tf - 1) == 0 and tf <= 64 and batch >= 1 and tf % batch == 0 and (batch == tf or tf == 4)
    assert pl["lds_bytes"] <= 65536
    assert pl["pitch"] % 2 == 1 and pl["pitch"] >= M + ((M - 1) >> 4)
    a = (tf - 1) * cfg.hop_length + N + 3 if cfg.hop_length <= N else tf * N
    a = (max(a, (cfg.n_mels or 0) * tf) + 3) // 4 * 4
    assert pl["lds_bytes"] == 4 * (a + (tf * (cfg.K | 1) + 3) // 4 * 4 + 2 * batch * pl["pitch"])
    assert pl["window"].shape == (N,)
    w64 = fr.window64(N, cfg.win_length)
    assert (np.abs(pl["window"].astype(np.float64) - w64) <= np.spacing(np.abs(w64).astype(np.float32))).all()
    off = (N - cfg.win_length) // 2
    outside = np.concatenate([pl["window"][:off], pl["window"][off + cfg.win_length:]])
    assert not outside.view(np.uint32).any(), "the window's zeros are +0.0"
    t64 = fr.twiddle64(N, pl["radix"])
    assert pl["twiddle"].shape == t64.shape
    ulp = np.spacing(np.maximum(np.abs(t64).astype(np.float32), np.float32(2.0 ** -126))).astype(np.float64)
    assert (np.abs(pl["twiddle"].astype(np.float64) - t64) <= ulp).all(), "a twiddle is more than one float32 ulp off"
    assert pl["twiddle"][0] == -0.5 and not pl["twiddle"][6:8].view(np.uint32).any()


def test_every_accepted_size_has_a_plan(sim):
    """Every even n_fft in [2, 2048] whose half is 2^a 3^b 5^c, at hop n_fft / 4, n_fft and above n_fft (the largest staging),
    with and without a mel stage: a plan of at least four frames within 64 KB, and everything check_plan asks."""
    assert len(ACCEPTED) == 87 and ACCEPTED[:6] == [2, 4, 6, 8, 10, 12] and ACCEPTED[-1] == 2048
    frames = {}
    for N in ACCEPTED:
        for hop, mels in ((max(1, N // 4), 128 if N >= 256 else None), (N, None), (N + 3, None)):
            cfg = mr.Cfg(48000, N, hop, N, n_mels=mels)
            pl = fr.sim_plan(sim, cfg)
            assert pl is not None, "no plan for n_fft %d hop %d" % (N, hop)
            check_plan(cfg, pl)
            frames[(N, hop)] = (pl["tile_frames"], pl["batch_frames"])
    assert frames[(2048, 512)] == (4, 4) and frames[(2048, 2048)] == (4, 1) and frames[(400, 100)][0] >= 16


@pytest.mark.parametrize("name", list(fr.FFT_CASES))
def test_plan_of_the_cases(sim, name):
    cfg, tf, batch, radix = fr.FFT_CASES[name]
    pl = fr.sim_plan(sim, cfg)
    check_plan(cfg, pl)
    assert (pl["tile_frames"], pl["batch_frames"], pl["radix"]) == (tf, batch, radix)
    if cfg.n_mels is not None:  # the filterbank is the direct plan's
        first, taps, fbw = mr.windows_of(mr.fbanks(cfg).astype(np.float32))
        assert taps == pl["taps"] and np.array_equal(first, pl["first"])
        ulp = np.spacing(np.maximum(np.abs(fbw), np.float32(2.0 ** -126)))  # libm's and numpy's log, exp may differ in the last bit
        assert (np.abs(pl["fb"].astype(np.float64) - fbw) <= ulp).all() and np.array_equal(pl["fb"] == 0, fbw == 0)


@pytest.mark.parametrize("N", [15, 14, 22, 2046, 2047, 0, 1, 2050, 4096])
def test_sizes_without_a_plan(sim, direct_sim, N):
    """Odd n_fft and an n_fft whose half has a prime factor above 5 have no FFT plan; the direct transform still takes them."""
    cfg = mr.Cfg(16000, N, max(1, N // 4), max(1, N))
    assert not fr.size_ok(N) and fr.sim_plan(sim, cfg) is None
    assert (mr.sim_plan(direct_sim, cfg) is not None) == (2 <= N <= 2048)


def test_refusals_in_the_library_source():
    """What needs a handle runs in tests/test_gpu_melfft.py; here: the entry refuses a transform above 1 and a size without a plan
    before it plans or touches HIP, with a message that names the rule, and nothing falls back to the direct transform."""
    src = open(os.path.join(ROOT, "saprobe-alac_amd", "csrc", "k_mel.hip")).read()
    body = src[src.index("int alacgpu_mel_create("):src.index("void alacgpu_mel_destroy(")]
    host = open(os.path.join(ROOT, "saprobe-alac_amd", "csrc", "alac_host.h")).read()
    assert "hipSetDevice" in host[host.index("void open(int dev)"):host.index("void upload(")] and "hip" not in body[:body.index("r->open(")]
    assert body.index("config->transform > ALACGPU_MEL_TRANSFORM_FFT") < body.index("size_ok(") < body.index("r->open(device)")  # the first HIP call
    assert "2^a 3^b 5^c" in body
    hdr = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    cfg = hdr[hdr.index("typedef struct alacgpu_mel_config"):hdr.index("} alacgpu_mel_config;")]
    assert re.search(r"uint32_t log;[^\n]*\n\s*uint32_t transform;[^\n]*\n\s*double floor;", cfg), "transform takes reserved0's place"
    assert "ALACGPU_MEL_TRANSFORM_DIRECT = 0, ALACGPU_MEL_TRANSFORM_FFT = 1" in hdr and "alacgpu_mel_fft_plan(" in hdr
    assert 'alacgpu 0.7.0' in open(os.path.join(ROOT, "saprobe-alac_amd", "csrc", "alacgpu.hip")).read()


# ---- 2. the host build against the restatement -------------------------------------------------------------------------
def run_case(sim, name, rng):
    cfg, tf = fr.FFT_CASES[name][:2]
    pl = fr.sim_plan(sim, cfg)
    assert pl["tile_frames"] == tf
    runs = fr.runs_of(name)
    Fs = {mr.out_frames(cfg, T) for _, T, _ in runs}
    assert {tf - 1, tf, tf + 1} <= Fs and {r for r, _, _ in runs} == {1, 3}
    assert {o for _, _, o in runs} == set(fr.offsets(cfg))
    worst = 0.0
    for k, (rows, T, (out_off, in_off)) in enumerate(runs):
        x = mr.signal(rng, rows, T)
        img, lay = fr.sim_image(sim, cfg, x, in_off, out_off, bin_pad=k % 3, guard=1)
        got = mr.values_of(img, lay, cfg, rows, T, "%s rows %d T %d" % (name, rows, T))
        worst = max(worst, fr.share(cfg, pl, x, got, "%s rows %d T %d offsets %d/%d" % (name, rows, T, in_off, out_off)))
    return worst


@pytest.mark.parametrize("name", list(fr.FFT_CASES))
def test_host_build_within_the_ceilings(sim, name):
    """Every case: rows 1 and 3, F = tile_frames - 1, tile_frames, tile_frames + 1, 1 and the shortest row, every base offset of
    mr.OFFSETS up to n_fft 128 and two above, sentinel-filled whole buffers, the input ending at an inaccessible page."""
    worst = run_case(sim, name, np.random.default_rng(len(name) + fr.FFT_CASES[name][0].n_fft))
    print("CEILING_SHARE host %s %.4f" % (name, worst))
    assert 0 < worst <= 1.0


@pytest.mark.parametrize("name", fr.IMPULSE_CASES)
def test_impulses(sim, name):
    """Rows of +0.0 with 1.0 at j: every bin of the frames that hold j within the ceiling of w32[n]^2 (the squared modulus of their
    complex sum where the reflected margins show j twice); the frames that do not hold j are +0.0 exactly. The ceiling is relative
    to the frame's own norm, w32[n] here, so a sample dropped or misplaced at a window's edge shows."""
    cfg, T, js = fr.impulse_batch(name)
    pl = fr.sim_plan(sim, cfg)
    x = mr.impulse_rows(T, js)
    img, lay = fr.sim_image(sim, cfg, x, 1, 2)
    got = mr.values_of(img, lay, cfg, len(js), T, name)
    fr.share(cfg, pl, x, got, name)
    v = mr.frames_of(cfg, x) * pl["window"].astype(np.float64)  # [R, F, N]
    empty = ~(v != 0).any(axis=2)  # frames without the impulse under a weight that is not zero
    assert empty.any() and (~empty).any()
    assert not got.transpose(0, 2, 1)[empty].view(np.uint32).any(), "a frame that does not hold the impulse is not +0.0"
    twice = ((mr.frames_of(cfg, x) != 0).sum(axis=2) >= 2).any()
    assert twice == (cfg.center and 4 <= cfg.n_fft <= 32), "the reflected margin shows an impulse twice (n_fft 2 reads x[1], x[0])"


@pytest.mark.parametrize("name", ["n16", "whisper", "n2048h512"])
def test_fft_against_the_direct_pass(sim, direct_sim, name):
    """The two transforms' host builds on the same input differ by no more than the sum of their ceilings."""
    cfg, tf = fr.FFT_CASES[name][:2]
    rng = np.random.default_rng(7)
    x = mr.signal(rng, 3, mr.length_for(cfg, tf + 2))
    img, lay = fr.sim_image(sim, cfg, x)
    a = mr.values_of(img, lay, cfg, 3, x.shape[1], name)
    img, lay = mr.sim_image(direct_sim, cfg, x)
    b = mr.values_of(img, lay, cfg, 3, x.shape[1], name)
    dplan = mr.sim_plan(direct_sim, cfg)
    _, lim_fft = fr.reference(cfg, x, fr.sim_plan(sim, cfg))
    dense = mr.dense_fb(dplan, cfg.K)
    _, lim_direct = mr.bounds(cfg, x, dplan["basis"], dense, dplan["taps"])
    diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
    assert (diff <= lim_fft + lim_direct).all() and diff.max() > 0, "the two transforms are not the same function"


# ---- 3. the stand-alone program ----------------------------------------------------------------------------------------
def test_standalone_program_builds_and_runs(tmp_path):
    """tests/host_sim/melfft_san_main.cpp, the program with its own main over melfft_sim.cpp's functions that DESIGN.md §14a runs
    under the sanitizers on a CPU: here it is built plainly and run once, so that it stays in step with the header. Three parameter
    sets, the input ending at the buffer's last element and at an inaccessible page, the LDS image exactly the plan's size."""
    exe = str(tmp_path / "melfft_san")
    host_build.compile("melfft_san_main.cpp", exe,
                       ["-O1", "-ffp-contract=off", "-fwrapv", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count("-> 0,") == 6 and "nan" not in r.stdout.lower()


# ---- 4. the names ------------------------------------------------------------------------------------------------------
def test_names_in_library_and_binding():
    import importlib
    import inspect
    pkg = importlib.import_module("saprobe-alac_amd")
    assert "alacgpu_mel_fft_plan" in pkg._EXPORTS
    assert [k for k, _ in pkg.MelConfig._fields_][11] == "transform"
    assert ctypes.sizeof(pkg.MelConfig) == 64 and ctypes.sizeof(pkg.MelFftInfo) == 64
    for fn in (pkg.MelSpectrogram.__init__, pkg.NewMelSpectrogram, pkg.mel_spectrogram, pkg.spectrogram, pkg.whisper_log_mel):
        par = inspect.signature(fn).parameters
        assert par["transform"].kind is inspect.Parameter.KEYWORD_ONLY and par["transform"].default == "direct"
        assert list(par)[-1] == "transform" and list(par)[-2] == "device"
    for bad in ("FFT", "", None, 1, "stockham"):
        with pytest.raises(ValueError):
            pkg._mel_config(16000, 400, None, None, 0.0, None, 80, True, None, "htk", None, 1e-10, bad)
    assert pkg._mel_config(16000, 400, None, None, 0.0, None, 80, True, None, "htk", None, 1e-10).transform == 0
    assert pkg._mel_config(16000, 400, None, None, 0.0, None, 80, True, None, "htk", None, 1e-10, "fft").transform == 1
    assert hasattr(pkg.MelSpectrogram, "fft_plan")
