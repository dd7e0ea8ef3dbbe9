"""The spectrogram pass with transform="fft" on the device (k_melfft.hip: alac_melfft_rows) against the host build of the same
header (tests/host_sim/melfft_sim.cpp), bit for bit up to the log, and the same device output against the numpy float64
restatement of tests/melfft_ref.py within the derived ceilings; the log, the special inputs, the entries, the refusals."""
import ctypes

import numpy as np
import pytest

from tests import mel_ref as mr
from tests import melfft_ref as fr
from tests.test_gpu_mel import LOG_ULPS, assert_same_image, device_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture(scope="module")
def sim():
    return fr.build_melfft_sim()


def new_fft(pkg, cfg):
    return pkg.NewMelSpectrogram(transform="fft", **cfg.kwargs())


def host_values(S, cfg, x):
    img, lay = fr.sim_image(S, cfg, x)
    return mr.rows_of(img, x.shape[0], cfg.bins, mr.out_frames(cfg, x.shape[1]), lay[5], lay[3], lay[4])


def same_fft_plan(lib_plan, lib_fft, want):
    return (all(lib_fft[k] == want[k] for k in fr.FFT_INFO) and lib_fft["radix"] == want["radix"]
            and all(np.array_equal(lib_fft[k].view(np.uint32), want[k].view(np.uint32)) for k in ("window", "twiddle"))
            and all(np.array_equal(lib_plan[k].view(np.uint32), want[k].view(np.uint32)) for k in ("fb", "first"))
            and lib_plan["tile_frames"] == want["tile_frames"] and lib_plan["lds_bytes"] == want["lds_bytes"] and lib_plan["basis"].size == 0)


@pytest.mark.parametrize("name", list(fr.FFT_CASES))
def test_device_equals_the_host_build_bit_for_bit(torch, pkg, sim, name):
    """Every case of fr.FFT_CASES: rows 1 and 3, F = tile_frames - 1, tile_frames, tile_frames + 1, 1 and the shortest row, every
    base offset of mr.OFFSETS up to n_fft 128 and two above; the whole sentinel-filled buffer equals the host build's, and the
    device's values lie within the ceilings of the restatement."""
    cfg, tf, batch, radix = fr.FFT_CASES[name]
    want = fr.sim_plan(sim, cfg)
    rng = np.random.default_rng(len(name) + cfg.n_fft)
    worst = 0.0
    with new_fft(pkg, cfg) as ms:
        plan, fft = ms.plan(), ms.fft_plan()
        assert same_fft_plan(plan, fft, want), "the library's plan is not the host build's"
        assert (fft["tile_frames"], fft["batch_frames"], fft["radix"]) == (tf, batch, radix)
        for k, (rows, T, (out_off, in_off)) in enumerate(fr.runs_of(name)):
            assert ms.out_frames(T) == mr.out_frames(cfg, T) > 0
            x = mr.signal(rng, rows, T)
            y = host_values(sim, cfg, x)
            img, lay = device_image(torch, ms, cfg, x, in_off, out_off, k % 3)
            what = "%s rows %d T %d offsets %d/%d" % (name, rows, T, in_off, out_off)
            assert_same_image(img, mr.expected_image(y, img.size, lay[5], lay[3], lay[4]), what, lay)
            got = mr.values_of(img, lay, cfg, rows, T, what)
            worst = max(worst, fr.share(cfg, want, x, got, what))
        assert ms.last_ms() > 0
    print("CEILING_SHARE device %s %.4f" % (name, worst))


@pytest.mark.parametrize("name", fr.IMPULSE_CASES)
def test_device_impulses(torch, pkg, sim, name):
    cfg, T, js = fr.impulse_batch(name)
    x = mr.impulse_rows(T, js)
    y = host_values(sim, cfg, x)
    with new_fft(pkg, cfg) as ms:
        img, lay = device_image(torch, ms, cfg, x, 1, 2)
    assert_same_image(img, mr.expected_image(y, img.size, lay[5], lay[3], lay[4]), name, lay)
    fr.share(cfg, fr.sim_plan(sim, cfg), x, mr.values_of(img, lay, cfg, len(js), T, name), name)


@pytest.mark.parametrize("name", ["n16", "whisper", "n2048h2048"])
def test_other_float_values(torch, pkg, sim, name):
    """Zeros, denormals, values whose powers overflow to inf, -0.0, an infinity and a NaN (mr.special_rows): non-finite words where
    the host build has them, a NaN where it has a NaN, every other word equal; the frames that do not cover the infinity or the NaN
    are finite: frames do not share a transform."""
    base = fr.FFT_CASES[name][0]
    for cfg in (base, mr.power_only(base)) if base.n_mels is not None else (base,):
        with new_fft(pkg, cfg) as ms:
            tf = ms.fft_plan()["tile_frames"]
            T = mr.length_for(cfg, tf + 2)
            x = mr.special_rows(np.random.default_rng(tf), T)
            y = host_values(sim, cfg, x)
            assert not y[0].view(np.uint32).any(), "zeros give +0.0"
            assert np.isfinite(y[1]).all() and np.isfinite(y[3]).all() and not np.isfinite(y[2]).all()
            for r, at in ((4, T // 3), (5, 2 * T // 3)):
                f = np.arange(y.shape[2]) * cfg.hop_length - (cfg.n_fft // 2 if cfg.center else 0)
                clear = (f > at) | (f + cfg.n_fft <= at)  # frames that do not read sample `at`
                assert clear.any() and (~clear).any() and np.isfinite(y[r][:, clear]).all() and not np.isfinite(y[r][:, ~clear]).all()
            for out_off, in_off in ((0, 0), (1, 3)):
                img, lay = device_image(torch, ms, cfg, x, in_off, out_off, 2)
                want = mr.expected_image(y, img.size, lay[5], lay[3], lay[4])
                nan = np.isnan(want.view(np.float32))
                assert nan.any() and np.isnan(img.view(np.float32)[nan]).all(), "a NaN of the host build is none on the device"
                inf = np.isinf(want.view(np.float32))
                assert np.array_equal(np.isinf(img.view(np.float32)), inf)
                assert_same_image(np.where(nan, 0, img), np.where(nan, 0, want), "%s bins %d offsets %d/%d" % (name, cfg.bins, in_off, out_off), lay)


def log_inputs(cfg, tf):
    rng = np.random.default_rng(17)
    T = mr.length_for(cfg, tf + 3)
    x = mr.signal(rng, 4, T)
    x[2] = (rng.uniform(-1, 1, T) * 1e-4).astype(np.float32)
    x[2, T // 4: T // 2] = 0.0  # frames of silence: at the floor
    return x


@pytest.mark.parametrize("name", ["n16", "whisper"])
def test_log_modes(torch, pkg, sim, name):
    """With P the device's own power, held to the host build bit for bit, every mode against float64 s log(max(P, floor)): within
    the bounds tests/test_gpu_mel.py uses for the same code (twice the 2.23 / 2.14 / 3.10 ulps of DESIGN.md §14), and float(s
    log(floor)) exactly for P at or below the floor."""
    worst = {}
    for base in (fr.FFT_CASES[name][0], mr.power_only(fr.FFT_CASES[name][0])):
        P = None
        for log, floor in ((None, 1e-10), ("ln", 1e-10), ("log10", 1e-10), ("db", 1e-10), ("log10", 1e-3), ("db", 0.5)):
            cfg = base.with_(log=log, floor=floor)
            with new_fft(pkg, cfg) as ms:
                if P is None:
                    x = log_inputs(cfg, ms.fft_plan()["tile_frames"])
                img, lay = device_image(torch, ms, cfg, x, 1, 2, 1)
            got = mr.values_of(img, lay, cfg, x.shape[0], x.shape[1], "log %s" % log)
            if log is None:
                P = got
                assert np.array_equal(P.view(np.uint32), host_values(sim, cfg, x).view(np.uint32))
                continue
            want = mr.log64(cfg, P)
            low = P <= np.float32(floor)
            assert low.any() and (~low).any()
            assert np.array_equal(got[low], want[low].astype(np.float32)), "log %s floor %g: at the floor" % (log, floor)
            u = float(mr.ulps32(got[~low], want[~low]).max())
            worst[log] = max(worst.get(log, 0.0), u)
    print("LOG_ULPS fft %s: %s" % (name, {k: round(v, 3) for k, v in worst.items()}))
    for log, u in worst.items():
        assert u <= LOG_ULPS[log], "log %s: %.3f ulps, bound %.3f" % (log, u, LOG_ULPS[log])


def test_pass_without_sync(torch, pkg, sim):
    cfg, tf = fr.FFT_CASES["whisper"][:2]
    x = mr.signal(np.random.default_rng(3), 5, mr.length_for(cfg, 3 * tf + 1))
    y = host_values(sim, cfg, x)
    with new_fft(pkg, cfg) as ms:
        img, lay = device_image(torch, ms, cfg, x, 2, 1, 0, sync=False)
        assert ms.last_ms() > 0
    assert_same_image(img, mr.expected_image(y, img.size, lay[5], lay[3], lay[4]), "sync=False", lay)


def test_small_inputs_and_no_work(torch, pkg):
    """tests/test_gpu_mel.py's test on an FFT handle: calls without work, which touch nothing, and what the entry refuses before a
    launch."""
    cfg = mr.CASES["tiny"]
    with new_fft(pkg, cfg) as ms:
        assert ms.fft_plan()["transform"] == 1 and ms.out_frames(40) == 11 and cfg.bins == 5 and ms.out_frames(8) == 0
        buf = torch.full((1024,), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        B = buf.data_ptr()
        ms.mel_device(B, 40, 0, 40, B + 2048, 55, 11)       # no rows
        ms.mel_device(B, 40, 2, 8, B + 2048, 55, 11)        # rows of n_fft / 2 samples: no frame
        ms.mel_device(None, 0, 0, 0, None, 0, 0)
        ms.synchronize()
        assert bool((buf == 7.0).all().item())
        for bad in [(None, 40, 2, 40, B + 2048, 55, 11), (B, 40, 2, 40, None, 55, 11), (B + 2, 40, 2, 40, B + 2048, 55, 11),
                    (B, 40, 2, 40, B + 2049, 55, 11), (B, 39, 2, 40, B + 2048, 55, 11), (B, 40, 2, 40, B + 2048, 55, 10),
                    (B, 40, 2, 40, B + 2048, 54, 11), (B, 1 << 62, 2, 40, B + 2048, 55, 11), (B, 40, 2, 40, B + 2048, 1 << 62, 11)]:
            with pytest.raises(ValueError):
                ms.mel_device(*bad)
        ms.synchronize()
        assert bool((buf == 7.0).all().item())
        ms.mel_device(B, 40, 2, 40, B + 2048, 55, 11)       # and the same call with everything in order does write
        assert not bool((buf[512:512 + 110] == 7.0).any().item()) and bool((buf[:512] == 7.0).all().item())
        assert bool((buf[512 + 110:] == 7.0).all().item())


def test_python_entries(torch, pkg, sim):
    """mel_spectrogram, spectrogram and whisper_log_mel with transform="fft" give the host build's bits; the cache keeps a direct
    and an FFT handle of one parameter set apart; transform="direct" gives the bits of a call without the keyword."""
    cfg = fr.FFT_CASES["whisper"][0]
    x = mr.signal(np.random.default_rng(5), 2, 1700)
    kw = {k: v for k, v in cfg.kwargs().items() if k != "sample_rate"}
    y = host_values(sim, cfg, x)
    xd = torch.from_numpy(x).to("cuda:0")
    def key(transform):  # the cache's key of this parameter set: (device, every field of the configuration)
        c = pkg._mel_config(cfg.sample_rate, transform=transform, **kw)
        return (0,) + tuple(getattr(c, k) for k, _ in pkg.MelConfig._fields_)

    others = set(pkg._MELS) - {key("direct"), key("fft")}  # another test of this process may have cached the direct handle
    fft = pkg.mel_spectrogram(xd, cfg.sample_rate, transform="fft", **kw)
    plain = pkg.mel_spectrogram(xd, cfg.sample_rate, **kw)
    direct = pkg.mel_spectrogram(xd, cfg.sample_rate, transform="direct", **kw)
    assert key("direct") != key("fft") and set(pkg._MELS) == others | {key("direct"), key("fft")}, "one handle per transform"
    h_direct, h_fft = pkg._MELS[key("direct")], pkg._MELS[key("fft")]
    assert h_direct is not h_fft and h_direct.fft_plan()["transform"] == 0 and h_fft.fft_plan()["transform"] == 1
    assert pkg.mel_spectrogram(x, cfg.sample_rate, transform="fft", **kw).shape == y.shape
    assert set(pkg._MELS) == others | {key("direct"), key("fft")} and pkg._MELS[key("fft")] is h_fft, "the handles are reused"
    assert np.array_equal(fft.cpu().numpy().view(np.uint32), y.view(np.uint32))
    assert torch.equal(plain, direct) and not torch.equal(plain, fft)
    assert float((plain - fft).abs().max()) <= 1e-3 * float(plain.max())
    pc = mr.power_only(cfg)
    sp = pkg.spectrogram(xd, cfg.sample_rate, 400, 400, 160, transform="fft")
    assert np.array_equal(sp.cpu().numpy().view(np.uint32), host_values(sim, pc, x).view(np.uint32))
    wl = pkg.whisper_log_mel(xd, transform="fft")
    wd = pkg.whisper_log_mel(xd)
    assert wl.shape == wd.shape == (2, 80, 10) and float((wl - wd).abs().max()) < 1e-4
    with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:  # a direct handle reports no FFT
        d = ms.fft_plan()
        assert d["transform"] == 0 and d["n_passes"] == 0 and d["radix"] == [] and d["window"].size == 0 and d["twiddle"].size == 0
        assert d["tile_frames"] == ms.plan()["tile_frames"] and d["lds_bytes"] == ms.plan()["lds_bytes"] and ms.plan()["basis"].size > 0
        assert ms.transform == "direct"
    with pytest.raises(ValueError):
        pkg.mel_spectrogram(xd, cfg.sample_rate, transform="FFT", **kw)


@pytest.mark.parametrize("N", [15, 14, 22, 2046, 2047])
def test_sizes_the_fft_refuses(torch, pkg, N):
    """ValueError with a message that names the rule; a direct handle for the same n_fft still builds and runs."""
    with pytest.raises(ValueError, match=r"2\^a 3\^b 5\^c"):
        pkg.NewMelSpectrogram(16000, N, n_mels=None, transform="fft")
    with pytest.raises(ValueError, match=r"2\^a 3\^b 5\^c"):
        pkg.spectrogram(np.zeros(4096, np.float32), 16000, N, transform="fft")
    with pkg.NewMelSpectrogram(16000, N, n_mels=None) as ms:
        assert ms(torch.zeros(4096)).shape == (N // 2 + 1, ms.out_frames(4096))


def test_transform_above_one_through_the_c_abi(torch, pkg):
    c = pkg._mel_config(16000, 400, None, None, 0.0, None, 80, True, None, "htk", None, 1e-10)
    for value, rc_want in ((2, -2), (0xFFFFFFFF, -2), (1, 0), (0, 0)):
        c.transform = value
        h = ctypes.c_void_p()
        rc = pkg.lib().alacgpu_mel_create(0, ctypes.byref(c), ctypes.byref(h))
        assert rc == rc_want and bool(h) == (rc == 0)
        if rc:
            assert b"transform" in pkg.lib().alacgpu_last_error()
        else:
            info = pkg.MelFftInfo()
            assert pkg.lib().alacgpu_mel_fft_plan(h, ctypes.byref(info), None, 0, None, 0) == 0 and info.transform == value
            small = np.zeros(3, np.float32)
            if value:  # a capacity below the table is refused
                assert pkg.lib().alacgpu_mel_fft_plan(h, ctypes.byref(info), small.ctypes.data, small.size, None, 0) == -2
            pkg.lib().alacgpu_mel_destroy(h)
    assert pkg.lib().alacgpu_mel_fft_plan(None, None, None, 0, None, 0) == -2


def test_cpp_entry(torch, pkg, sim):
    """host/mel_spectrogram.hpp: MelConfig's transform member defaults to direct; set to fft, FftPlan() is the host build's plan and
    MelDevice gives its bits; a refused size is std::invalid_argument."""
    S = fr.build_melfft_shim(pkg)
    cfg = mr.Cfg(16000, 400, 160, 400, n_mels=40)  # MelConfig's defaults: htk, f_max = sample_rate / 2
    want = fr.sim_plan(sim, cfg)
    x = mr.signal(np.random.default_rng(9), 2, 2000)
    y = host_values(sim, cfg, x)
    F = y.shape[2]
    dev = torch.device("cuda:0")
    d_in = torch.from_numpy(x).to(dev)
    d_out = torch.zeros((2, 40, F), dtype=torch.float32, device=dev)
    info = np.zeros(16, np.uint32)
    win = np.zeros(400, np.float32)
    tw = np.zeros(want["twiddle"].size, np.float32)
    torch.cuda.synchronize()

    def run(n_fft, transform):
        return S.melfft_shim_run(16000, n_fft, n_fft, 160, 40, 1, transform, d_in.data_ptr(), 2000, 2, 2000, d_out.data_ptr(), 40 * F, F,
                                 info.ctypes.data, win.ctypes.data, win.size, tw.ctypes.data, tw.size)

    assert run(400, 1) == 0, S.melfft_shim_last_error()
    assert list(info[:6]) == [want[k] for k in fr.FFT_INFO] and list(info[6:6 + info[5]]) == want["radix"]
    assert np.array_equal(win.view(np.uint32), want["window"].view(np.uint32)) and np.array_equal(tw.view(np.uint32), want["twiddle"].view(np.uint32))
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), y.view(np.uint32))
    assert run(400, 0) == 0 and info[0] == 0 and info[5] == 0 and info[14] == 0
    assert not np.array_equal(d_out.cpu().numpy().view(np.uint32), y.view(np.uint32))
    assert run(398, 1) == -6 and b"2^a 3^b 5^c" in S.melfft_shim_last_error()
    assert run(400, 2) == -6
