"""The Kaldi feature pass with transform="fft" on the CPU: csrc/alac_fbankfft.h built with g++, contraction off
(tests/host_sim/fbankfft_sim.cpp), tile for tile, phase for phase and work item for work item what the gfx950 kernel of
k_fbankfft.hip runs, against tests/kaldi_ref.py's step-by-step float64 restatement within the ceilings that tests/kaldifft_ref.py
derives.

* the plan of every accepted size: radices, ws, twiddles, LDS, tile_frames and batch_frames, the tables it shares with the direct
  plan bit for bit; the sizes that have no FFT plan while the direct plan exists;
* the host build over whole sentinel-filled buffers at every case of kf.FFT_CASES, every base offset, odd strides, a frame stride
  above cols, the input ending at an inaccessible page;
* impulses; the FFT build against the direct build; the energy column bit for bit the direct build's; a constant row, which is
  exactly +0.0; the logs and MFCC within kr.check_logged's bounds; other float values; the column arrangement;
* the stand-alone program that the sanitizer runs use; the new names in library source, header and binding.

The library's own plan needs a handle, so it is held against the host build's in tests/test_gpu_fbankfft.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import host_build
from tests import kaldi_ref as kr
from tests import kaldifft_ref as kf
from tests import melfft_ref as fr

ROOT = kf.ROOT


@pytest.fixture(scope="module")
def sim():
    return kf.build_fbankfft_sim()


@pytest.fixture(scope="module")
def direct_sim():
    return kr.build_fbank_sim()


# ---- 1. the plan -------------------------------------------------------------------------------------------------------
ACCEPTED = [n for n in range(2, 2049) if fr.size_ok(n)]


def check_plan(cfg, pl, direct=None):
    N, W, M = cfg.N, cfg.W, cfg.N // 2
    assert pl["transform"] == 1 and (pl["n_fft"], pl["frame_length"], pl["n_freqs"]) == (N, W, cfg.K)
    assert int(np.prod(pl["radix"], dtype=np.int64)) == M and all(r in (2, 3, 4, 5) for r in pl["radix"])
    assert pl["n_passes"] == len(pl["radix"]) and pl["radix"] == kf.radices_of(N)
    tf, batch = pl["tile_frames"], pl["batch_frames"]
    assert tf >= 4 and tf & (tf - 1) == 0 and tf <= 64 and batch >= 1 and tf % batch == 0 and (batch == tf or tf == 4)
    assert pl["lds_bytes"] <= 65536
    assert (tf, batch, pl["lds_bytes"]) == kf.lds_rule(cfg)[:2] + (4 * kf.lds_rule(cfg)[2],), "the LDS formula"
    assert pl["pitch"] % 2 == 1 and pl["pitch"] >= M + ((M - 1) >> 4)
    # the places: staging, power tile, energies, cepstral tile, sums, transform buffer, one behind the other
    assert pl["a_floats"] % 4 == 0 and pl["p_floats"] == (tf * (cfg.K | 1) + 3) // 4 * 4
    assert pl["e_off"] == pl["a_floats"] + pl["p_floats"] and pl["c_off"] == pl["e_off"] + (tf if cfg.energy else 0)
    assert pl["s_off"] == pl["c_off"] + cfg.ceps * tf and pl["b_off"] == pl["s_off"] + (256 if cfg.dc else 0)
    assert pl["b_off"] % 2 == 0 and 4 * (pl["b_off"] + 2 * batch * pl["pitch"]) == pl["lds_bytes"]
    assert pl["parts"] * tf == 256
    # ws = float(scale * win), +0.0 where that is 0 and from W on
    ws = pl["window"]
    assert ws.shape == (N,)
    sw = cfg.scale * kr.window(cfg)
    ulp = np.spacing(np.maximum(np.abs(sw).astype(np.float32), np.float32(2.0 ** -126))).astype(np.float64)
    assert (np.abs(ws[:W].astype(np.float64) - sw) <= ulp).all(), "ws is more than one float32 ulp off"
    assert not ws[:W][sw == 0.0].view(np.uint32).any() and not ws[W:].view(np.uint32).any(), "the window's zeros are +0.0"
    t64 = fr.twiddle64(N, pl["radix"])
    assert pl["twiddle"].shape == t64.shape
    ulp = np.spacing(np.maximum(np.abs(t64).astype(np.float32), np.float32(2.0 ** -126))).astype(np.float64)
    assert (np.abs(pl["twiddle"].astype(np.float64) - t64) <= ulp).all(), "a twiddle is more than one float32 ulp off"
    if direct is not None:
        assert pl["taps"] == direct["taps"] and pl["cols"] == direct["cols"]
        for k in kf.TABLES:
            assert np.array_equal(pl[k].view(np.uint32), direct[k].view(np.uint32)), k + " is not the direct plan's"


def test_every_accepted_size_has_a_plan(sim, direct_sim):
    """Without rounding, every even W = N in [2, 2048] whose half is 2^a 3^b 5^c, at shift N / 4, N and N + 3 (the largest
    staging): a plan of at least four frames within 64 KB and everything check_plan asks; at shift N / 4 the filterbank is the
    direct plan's bit for bit. With rounding, every W in [2, 2048] has a plan, of the power of two."""
    assert len(ACCEPTED) == 87
    frames = {}
    for N in ACCEPTED:
        for hop in (max(1, N // 4), N, N + 3):
            cfg = kr.Cfg(48000, N, hop, mels=64 if N >= 256 else 5, pow2=False, energy=N % 3 == 0)
            pl = kf.sim_plan(sim, cfg)
            assert pl is not None, "no plan for W = N = %d, shift %d" % (N, hop)
            check_plan(cfg, pl, kr.sim_plan(direct_sim, cfg) if hop < N and N <= 512 else None)
            frames[(N, hop)] = (pl["tile_frames"], pl["batch_frames"])
    assert frames[(2048, 512)] == (4, 2) and frames[(2048, 2048)] == (4, 1) and frames[(400, 100)] == (16, 16)
    for W in range(2, 2049):
        cfg = kr.Cfg(48000, W, max(1, W // 3), mels=5)
        pl = kf.sim_plan(sim, cfg)
        assert pl is not None and pl["n_fft"] == cfg.N and pl["lds_bytes"] <= 65536 and pl["tile_frames"] >= 4, W


@pytest.mark.parametrize("name", list(kf.FFT_CASES))
def test_plan_of_the_cases(sim, direct_sim, name):
    """The case's plan and its unlogged twin's: check_plan, the tile and the radices the case table says, and fbw / first / dct /
    lifter bit for bit the direct plan's"""
    cfg, tf, batch, radix = kf.FFT_CASES[name]
    for c in (cfg, cfg.prelog()):
        pl = kf.sim_plan(sim, c)
        check_plan(c, pl, kr.sim_plan(direct_sim, c))
        assert (pl["tile_frames"], pl["batch_frames"], pl["radix"]) == (tf, batch, radix)
    if name in kf.PINNED:
        assert (tf, batch, radix) == kf.PINNED[name]


@pytest.mark.parametrize("cfg", kf.REFUSED + [kr.Cfg(8000, 2046, 512, pow2=False), kr.Cfg(8000, 2047, 512, pow2=False)],
                         ids=lambda c: "W%d" % c.W)
def test_sizes_without_an_fft_plan(sim, direct_sim, cfg):
    """W = 1 (N = 1), and without rounding an odd N or one whose half has a prime factor above 5: no FFT plan, while the direct
    plan for the same configuration exists; with rounding the same W has one (but W = 1)."""
    assert not fr.size_ok(cfg.N) and kf.sim_plan(sim, cfg) is None
    assert kr.sim_plan(direct_sim, cfg) is not None
    assert (kf.sim_plan(sim, cfg.with_(pow2=True)) is not None) == (cfg.W > 1)


def test_what_the_direct_plan_refuses_is_refused(sim):
    """dither, vtln_warp, use_power, raw_energy, a frame length above 2048, no mel bins: no FFT plan either"""
    for refused in (dict(dither=1.0), dict(vtln=1.1), dict(use_power=0), dict(raw_energy=0)):
        cfg = kr.W10.with_(energy=True)
        assert kf.sim_plan(sim, cfg, **refused) is None and kf.sim_plan(sim, cfg) is not None
    for cfg in (kr.Cfg(8000, 2049, 4), kr.Cfg(8000, 0, 4), kr.Cfg(8000, 8, 0), kr.W10.with_(mels=0), kr.W10.with_(scale=0.0)):
        assert kf.sim_plan(sim, cfg) is None


def test_refusals_in_the_library_source():
    """What needs a handle runs in tests/test_gpu_fbankfft.py; here: the entry refuses a transform above 1 and a size without a
    plan before it plans or touches HIP, with a message that names the rule, and nothing falls back to the direct transform."""
    src = open(os.path.join(ROOT, "saprobe-alac_amd", "csrc", "k_fbank.hip")).read()
    body = src[src.index("int alacgpu_fbank_create_transform("):src.index("void alacgpu_fbank_destroy(")]
    assert "hip" not in body[:body.index("r->open(")]
    assert body.index("transform > ALACGPU_FBANK_TRANSFORM_FFT") < body.index("size_ok(") < body.index("r->open(device)")
    assert "2^a 3^b 5^c" in body
    one = src[src.index("int alacgpu_fbank_create("):src.index("int alacgpu_fbank_create_transform(")]
    assert "alacgpu_fbank_create_transform(device, config, ALACGPU_FBANK_TRANSFORM_DIRECT, out)" in one
    hdr = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    assert "ALACGPU_FBANK_TRANSFORM_DIRECT = 0, ALACGPU_FBANK_TRANSFORM_FFT = 1" in hdr and "alacgpu_fbank_fft_plan(" in hdr
    assert 'alacgpu 0.7.0' in open(os.path.join(ROOT, "saprobe-alac_amd", "csrc", "alacgpu.hip")).read()


# ---- 2. the host build against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(kf.FFT_CASES))
def test_host_build_within_the_ceilings(sim, name):
    """Every case over kf.case_runs (F = tile_frames - 1, tile_frames, tile_frames + 1 and 1, rows 1 and 3), each at every base
    offset of kr.OFFSETS (two for the large cases) with odd strides, the frame stride cols, cols + 1 .. cols + 3 in turn, whole
    sentinel-filled buffers, the input ending at an inaccessible page: with nothing logged against kr.features64 within
    kf.reference's ceiling, the same bits at every offset; then the case's own pass (log fbank, log energy, MFCC) against the
    float64 of the build's own unlogged values within kr.check_logged's bounds; the layout bins is the transpose, bit for bit."""
    cfg, tf = kf.FFT_CASES[name][:2]
    pre = cfg.prelog()
    pl = kf.sim_plan(sim, pre)
    offs = kr.OFFSETS if name in kf.SMALL else [kr.OFFSETS[1], kr.OFFSETS[3]]
    worst = worst_log = 0.0
    seen = set()
    for k, rows, T, x in kf.case_runs(name):
        seen.add((kr.out_frames(cfg, T), rows))
        y = None
        for j, (out_off, in_off) in enumerate(offs):
            what = "%s rows %d T %d offsets %d/%d" % (name, rows, T, in_off, out_off)
            img, lay = kf.sim_image(sim, pre, x, in_off, out_off, j, guard=1)
            got = kr.values_of(img, lay, pre, rows, T, what)
            assert y is None or kr.same_bits(got, y), what + ": the values depend on where the buffers lie"
            y = got
        worst = max(worst, kf.share(pre, pl, x, y, what))
        img, lay = kf.sim_image(sim, cfg, x, 2, 1, 3)
        worst_log = max(worst_log, kr.check_logged(cfg, kr.values_of(img, lay, cfg, rows, T, what), y, what))
        b = pre.with_(layout="bins")
        img, lay = kf.sim_image(sim, b, x, 1, 3, 3, guard=1)
        assert kr.same_bits(kr.values_of(img, lay, b, rows, T, what), y), what + " layout bins"
    assert {f for f, _ in seen} >= {tf - 1, tf, tf + 1} and {r for _, r in seen} == {1, 3}
    print("CEILING_SHARE host %s %.4f logged %.3f" % (name, worst, worst_log))
    assert worst <= 1.0 and (worst > 0 or cfg.N == 2)  # N 2 has the DC bin alone, which no mel filter weighs


@pytest.mark.parametrize("name", kf.IMPULSE_CASES)
def test_impulses(sim, name):
    """No DC removal, nothing logged: rows of +0.0 with 1.0 at j, every j of the first 3 W and last 2 W samples, in the case's own
    frame mode. Within the ceiling of the float64 result (relative to the frame's own norm, so a sample dropped or misplaced
    shows); the frames that do not read j are exactly +0.0 in every mel column. The impulse at a frame's n = 0 exercises v[-1] =
    v[0]: there y[0] = (1 - c) and y[1] = -c, not 1 and -c."""
    cfg, T, js = kf.impulse_batch(name)
    pl = kf.sim_plan(sim, cfg)
    x = np.zeros((len(js), T), np.float32)
    x[np.arange(len(js)), js] = 1.0
    img, lay = kf.sim_image(sim, cfg, x, 1, 2, 1)
    got = kr.values_of(img, lay, cfg, len(js), T, name)
    kf.share(cfg, pl, x, got, name)
    idx = kr.frame_index(cfg, T)  # [F, W]
    reads = (idx[None, :, :] == np.array(js)[:, None, None]).any(axis=2)  # [R, F]
    assert reads.any() and (~reads).any() and (idx[:, 0][None, :] == np.array(js)[:, None]).any()
    assert not got[~reads].view(np.uint32).any(), "a frame that does not read the impulse is not +0.0"
    if cfg.N > 2:
        assert got[reads].any()


@pytest.mark.parametrize("name", ["w10", "asr", "k48"])
def test_fft_against_the_direct_build(sim, direct_sim, name):
    """The two transforms' host builds on the same input differ by no more than the sum of their ceilings"""
    cfg, tf = kf.FFT_CASES[name][:2]
    pre = cfg.prelog()
    x = kr.signal(np.random.default_rng(7), 3, kr.length_for(cfg, tf + 2), 0.3)
    a = kf.host_values(sim, pre, x)
    b = kr.host_values(direct_sim, pre, x)
    _, lim_fft = kf.reference(pre, kf.sim_plan(sim, pre), x)
    _, lim_direct = kr.prelog_bounds(pre, kr.sim_plan(direct_sim, pre), x)
    diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
    assert (diff <= lim_fft + lim_direct).all() and diff.max() > 0, "the two transforms are not the same function"


@pytest.mark.parametrize("name", [k for k, c in kf.FFT_CASES.items() if c[0].energy])
def test_energy_column_is_the_direct_builds(sim, direct_sim, name):
    """The energy column of an FFT pass, logged and not: bit for bit the direct build's"""
    cfg, tf = kf.FFT_CASES[name][:2]
    x = kr.signal(np.random.default_rng(11), 3, kr.length_for(cfg, tf + 1), 0.3)
    for c in (cfg, cfg.prelog()):
        col = (c.cols - 1) if c.htk else 0
        a, b = kf.host_values(sim, c, x), kr.host_values(direct_sim, c, x)
        assert kr.same_bits(a[..., col], b[..., col]) and len(np.unique(a[..., col])) > tf


def test_constant_row(sim):
    """A row of constant 0.5 with DC removal at scale 1 and 32768: every unlogged mel column and the energy are +0.0, as Kaldi has
    them (the direct transform's folded tables leave their rounding: kr.check_constant), the logged ones float32(ln 2^-23)"""
    kf.check_constant(lambda cfg, x: kf.host_values(sim, cfg, x), None)


def test_column_arrangement(sim):
    print("sqrt(2) C0 on the host build: largest error / bound %.3f" % kr.check_arrangement(lambda cfg, x: kf.host_values(sim, cfg, x)))


@pytest.mark.parametrize("name", kr.SPECIAL_CASES)
def test_other_float_values(sim, name):
    """Zeros, denormals, 1e30, -0.0, an infinity and a NaN (mr.special_rows): kr.check_special_unlogged and, for the case's own
    logging pass, kr.check_special_logged. Only the frames that read the non-finite sample are non-finite."""
    cfg, T, x = kr.special_input(name)
    assert name in kf.FFT_CASES
    P = kf.host_values(sim, cfg.prelog(), x)
    kr.check_special_unlogged(cfg.prelog(), T, x, P)
    kr.check_special_logged(cfg, kf.host_values(sim, cfg, x), P, name)


@pytest.mark.parametrize("name", ["mfcc13", "mfcc_e_htk", "mfcc_htk"])
def test_silence_through_mfcc(sim, name):
    kr.check_silence_mfcc(lambda cfg, x: kf.host_values(sim, cfg, x), name)


# ---- 3. the stand-alone program ----------------------------------------------------------------------------------------
def test_standalone_program_builds_and_runs(tmp_path):
    """tests/host_sim/fbankfft_san_main.cpp, the program with its own main over fbankfft_sim.cpp's functions that DESIGN.md §15b
    runs under the sanitizers on a CPU: here it is built plainly and run once, so that it stays in step with the header. Three
    parameter sets (W odd below N; asr; full with one frame in the transform buffer), the input ending at the buffer's last
    element and at an inaccessible page, the LDS image exactly the plan's size."""
    exe = str(tmp_path / "fbankfft_san")
    host_build.compile("fbankfft_san_main.cpp", exe,
                       ["-O1", "-ffp-contract=off", "-fwrapv", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count("-> 0,") == 6 and "nan" not in r.stdout.lower() and "batch 1," in r.stdout


# ---- 4. the names ------------------------------------------------------------------------------------------------------
def test_names_in_library_and_binding():
    import importlib
    import inspect
    pkg = importlib.import_module("saprobe-alac_amd")
    assert "alacgpu_fbank_fft_plan" in pkg._EXPORTS and "alacgpu_fbank_create_transform" in pkg._EXPORTS
    assert ctypes.sizeof(pkg.FbankConfig) == 136 and ctypes.sizeof(pkg.FbankFftInfo) == 64
    for fn in (pkg.KaldiFeatures.__init__, pkg.kaldi_fbank, pkg.kaldi_mfcc):
        par = inspect.signature(fn).parameters
        assert par["transform"].kind is inspect.Parameter.KEYWORD_ONLY and par["transform"].default == "direct"
        assert list(par)[-1] == "transform" and list(par)[-2] == "device"
    for bad in ("FFT", "", None, 1, "stockham"):
        with pytest.raises(ValueError):
            pkg._fbank_transform(bad)
    assert pkg._fbank_transform("direct") == 0 and pkg._fbank_transform("fft") == 1
    assert hasattr(pkg.KaldiFeatures, "fft_plan")
    mk = open(os.path.join(ROOT, "saprobe-alac_amd", "csrc", "Makefile")).read()
    assert "k_fbankfft" in mk.split("UNITS =")[1].split("\n")[0] and "build/k_fbankfft.o: alac_fbankfft.h" in mk
