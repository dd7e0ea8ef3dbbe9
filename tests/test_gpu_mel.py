"""alacgpu_mel_device on the GPU: bit for bit what the host build of the same header (tests/host_sim/mel_sim.cpp) writes, over
whole sentinel-filled buffers with NaN between the input rows, mr.EDGE_CASES also within the derived ceilings against the
float64 restatement; impulses, which come out as single table entries; zeros, denormals,
huge values, -0.0, an infinity and a NaN; the log modes against float64 in float32 ulps; the Python entries over it
(mel_spectrogram, spectrogram, whisper_log_mel, the pass behind load_clips); and host/mel_spectrogram.hpp through
tests/host_sim/mel_shim.cpp.

The values of the host build do not depend on where the buffers lie (tests/test_mel_host.py runs it at every offset), so it runs
once per (parameters, rows, length) here and the device is held to its values at every offset.

No test provokes a fault: the arguments the entry refuses are refused on the host, before a launch."""
import ctypes

import numpy as np
import pytest

from tests import clip_ref as cr
from tests import m4a
from tests import mel_ref as mr

pytestmark = pytest.mark.gpu

# The device's log against float64 s log(max(P, floor)) over the inputs of test_log_modes, in float32 ulps of the result: the
# largest measured on an MI355X (ln 2.226, log10 2.141, db 3.103, each over the power spectrogram of n_fft 400; the host build's
# libm gives 0.72, 1.67 and 2.03 on the same inputs). The bound is twice that, and at least 1: the margin covers inputs the
# sample missed.
LOG_ULPS_MEASURED = {"ln": 2.226, "log10": 2.141, "db": 3.103}
LOG_ULPS = {k: max(1.0, 2.0 * v) for k, v in LOG_ULPS_MEASURED.items()}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture(scope="module")
def sim():
    return mr.build_mel_sim()


def device_image(torch, ms, cfg, x, in_off=0, out_off=0, bin_pad=0, sync=True):
    rows, T = x.shape
    F = mr.out_frames(cfg, T)
    lay = mr.layout(rows, T, cfg.bins, F, in_off, out_off, bin_pad)
    in_stride, in_lead, in_elems, row_stride, bin_stride, out_lead, out_elems = lay
    dev = torch.device("cuda:0")
    host = np.full(in_elems, np.nan, np.float32)  # NaN between the rows: a read outside a row's [0, T) shows
    for r in range(rows):
        host[in_lead + r * in_stride: in_lead + r * in_stride + T] = x[r]
    src = torch.from_numpy(host).to(dev)
    buf = torch.full((out_elems,), mr.SENTINEL - (1 << 32), dtype=torch.int32, device=dev)
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    ms.mel_device(src.data_ptr() + 4 * in_lead, in_stride, rows, T, buf.data_ptr() + 4 * out_lead, row_stride, bin_stride, sync=sync)
    if not sync:
        ms.synchronize()
    return buf.cpu().numpy().view(np.uint32), lay


def host_values(S, cfg, x):
    """[rows, bins, F] float32 of the host build"""
    img, lay = mr.sim_image(S, cfg, x)
    return mr.rows_of(img, x.shape[0], cfg.bins, mr.out_frames(cfg, x.shape[1]), lay[5], lay[3], lay[4])


def assert_same_image(img, want, what, lay):
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError("%s: element %d of the buffer (rows start at %d, row stride %d, bin stride %d): got %#x, want %#x (%d "
                             "differ)" % (what, bad[0], lay[5], lay[3], lay[4], img[bad[0]], want[bad[0]], len(bad)))


def same_plan(a, b):
    return all(a[k] == b[k] for k in mr.INFO) and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
                                                      for k in ("basis", "fb", "first"))


@pytest.mark.parametrize("name", list(mr.CASES))
def test_device_equals_the_host_build_bit_for_bit(torch, pkg, sim, name):
    """mr.CASES with and without the mel stage, log off: rows 1 and 5; F = tile_frames - 1, tile_frames, tile_frames + 1, 1 where a
    row can be that short, and the shortest row there is (n_fft / 2 + 1 centred); the four offset pairs of mr.OFFSETS, the last
    three with a bin stride of F + 3. Above n_fft 64 five rows run at tile_frames + 1 only, and the power spectrogram alone at
    that length: the host build is what takes the time."""
    mel_cfg = mr.CASES[name]
    rng = np.random.default_rng(len(name))
    small = mel_cfg.n_fft <= 64
    for cfg in (mel_cfg, mel_cfg.with_(n_mels=None, mel_scale=None, norm=None)):
        with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
            plan = ms.plan()
            assert same_plan(plan, mr.sim_plan(sim, cfg)), "the library's plan is not the host build's"
            with pytest.raises(ValueError):
                ms.last_ms()  # no pass yet on this handle
            tf = plan["tile_frames"]
            shortest = cfg.n_fft // 2 + 1 if cfg.center else cfg.n_fft
            Ts = sorted({mr.length_for(cfg, F) for F in (tf - 1, tf, tf + 1, 1)} | {shortest})
            Fs = {mr.out_frames(cfg, T) for T in Ts}
            assert {tf - 1, tf, tf + 1} <= Fs and (1 in Fs or cfg.hop_length <= cfg.n_fft // 2)
            if not small and cfg.n_mels is None:
                Ts = [mr.length_for(cfg, tf + 1)]
            for T in Ts:
                F = mr.out_frames(cfg, T)
                assert ms.out_frames(T) == F > 0
                for rows in (1, 5) if small or F == tf + 1 else (1,):
                    x = mr.signal(rng, rows, T)
                    y = host_values(sim, cfg, x)
                    for k, (out_off, in_off) in enumerate(mr.OFFSETS):
                        img, lay = device_image(torch, ms, cfg, x, in_off, out_off, 3 if k else 0)
                        assert_same_image(img, mr.expected_image(y, img.size, lay[5], lay[3], lay[4]),
                                          "%s bins %d rows %d T %d offsets %d/%d" % (name, cfg.bins, rows, T, in_off, out_off), lay)
            assert ms.last_ms() > 0
            assert ms.out_frames(shortest - 1) == 0


@pytest.mark.parametrize("name", list(mr.EDGE_CASES))
def test_edge_cases_on_the_device(torch, pkg, sim, name):
    """mr.EDGE_CASES, each at the tile_frames its table gives (dft_blocks<4>, tile_frames 8, hop > n_fft, the DFT loop's tail, n_fft
    below 4, even K, odd n_fft, 60 608 bytes of LDS): the library's plan is the host build's; rows 1 and 3 at F = tile_frames + 1,
    the shortest row and (up to n_fft 128) F = tile_frames, the device's whole buffer bit for bit the host build's at the four
    offset pairs of mr.OFFSETS (two above n_fft 128); and the device's own values within the ceilings of mr.bounds against the
    float64 restatement, which does not come from the header."""
    cfg, tf = mr.EDGE_CASES[name]
    small = name in mr.SMALL_EDGES
    rng = np.random.default_rng(len(name) + cfg.n_fft)
    worst = 0.0
    with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
        plan = ms.plan()
        assert plan["tile_frames"] == tf
        assert same_plan(plan, mr.sim_plan(sim, cfg)), "the library's plan is not the host build's"
        for rows in (1, 3):
            for T in mr.edge_lengths(cfg, tf):
                assert ms.out_frames(T) == mr.out_frames(cfg, T) > 0
                x = mr.signal(rng, rows, T)
                y = host_values(sim, cfg, x)
                for k, (out_off, in_off) in enumerate(mr.OFFSETS if small else mr.OFFSETS[:2]):
                    what = "%s rows %d T %d offsets %d/%d" % (name, rows, T, in_off, out_off)
                    img, lay = device_image(torch, ms, cfg, x, in_off, out_off, 3 if k else 0)
                    if k == 0:
                        worst = max(worst, mr.ceiling_share(cfg, plan, x, mr.values_of(img, lay, cfg, rows, T, what), what))
                    assert_same_image(img, mr.expected_image(y, img.size, lay[5], lay[3], lay[4]), what, lay)
    print("%s: tile_frames %d, at most %.1f %% of the ceiling" % (name, tf, 100 * worst))


@pytest.mark.parametrize("name", mr.IMPULSE_CASES)
def test_device_impulse_at_every_n(torch, pkg, name):
    """One launch over a batch of rows, row r of +0.0 with 1.0 at js[r] (mr.impulse_batch: every j of the first 3 n_fft and the last
    2 n_fft samples; at n_fft 2048 the n of one frame at the window's edges and its middle): every power is fmaf(S, S, C * C) of the
    handle's own table entries under the impulse, or of their sum where the reflected margin shows it twice, and +0.0 elsewhere;
    the whole buffer compared as uint32. The expectation needs the table alone, not the header."""
    cfg, tf, T, js = mr.impulse_batch(name)
    with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
        plan = ms.plan()
        assert plan["tile_frames"] == tf
        want, twice, silent = mr.impulse_image(cfg, plan["basis"], T, js)
        if cfg.n_fft < 2048:  # the positions of the large cases lie inside the row, away from both margins
            assert (twice > 0) == (cfg.center and cfg.n_fft >= 3), "the reflected margin shows an impulse twice"
        if name == "hop37":
            assert silent > 0, "no impulse lies between two frames"
        img, lay = device_image(torch, ms, cfg, mr.impulse_rows(T, js), 1, 2, 1)
    assert_same_image(img, mr.expected_image(want, img.size, lay[5], lay[3], lay[4]), "%s: impulses at %d positions" % (name, len(js)), lay)


@pytest.mark.parametrize("name", ["tiny", "band"])
def test_log_modes_on_other_float_values(torch, pkg, name):
    """ln and db over mr.special_rows, against the device's own output P with the log off: +inf where P is +inf, a NaN where P is
    one, float32(s log(floor)) exactly where P is at or below the floor (the zeros and the denormals), within LOG_ULPS of float64 s
    log(P) everywhere else."""
    base = mr.CASES[name] if name in mr.CASES else mr.EDGE_CASES[name][0]
    T = mr.length_for(base, 64 + 2)
    x = mr.special_rows(np.random.default_rng(31), T)
    P = None
    for log in (None, "ln", "db"):
        cfg = base.with_(log=log, floor=1e-10)
        with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
            assert ms.plan()["tile_frames"] == 64
            img, lay = device_image(torch, ms, cfg, x, 3, 1, 2)
        got = mr.values_of(img, lay, cfg, 6, T, "log %s" % log)
        if log is None:
            P = got
            inf, nan = np.isposinf(P), np.isnan(P)
            low = P <= np.float32(1e-10)
            rest = ~(inf | nan | low)
            assert inf.any() and nan.any() and low[:2].all() and rest.any() and not (P[~nan] < 0).any()
            continue
        s = 10.0 if log == "db" else 1.0
        fl = float(np.float32(1e-10))
        assert np.isposinf(got[inf]).all(), "log %s of +inf" % log
        assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any(), "log %s of a NaN" % log
        at_floor = np.float32(s * (np.log(fl) if log == "ln" else np.log10(fl)))
        assert np.array_equal(got[low].view(np.uint32), np.full(low.sum(), at_floor, np.float32).view(np.uint32)), "log %s at the floor" % log
        u = float(mr.ulps32(got[rest], mr.log64(cfg, P[rest].astype(np.float64))).max())
        print("%s log %s: %.3f ulps over %d values" % (name, log, u, rest.sum()))
        assert u <= LOG_ULPS[log], "log %s: %.3f ulps, bound %.3f" % (log, u, LOG_ULPS[log])


def test_pass_without_sync(torch, pkg, sim):
    """mel_device(..., sync=False) and then synchronize(): the image of sync=True, and the pass has a time."""
    cfg = mr.CASES["tiny"]
    x = mr.signal(np.random.default_rng(5), 3, mr.length_for(cfg, 64 + 5))
    with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
        want, lay = device_image(torch, ms, cfg, x, 1, 2, 1, sync=True)
    with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
        img, _ = device_image(torch, ms, cfg, x, 1, 2, 1, sync=False)
        assert ms.last_ms() > 0
    assert_same_image(img, want, "sync=False", lay)
    y = host_values(sim, cfg, x)
    assert_same_image(img, mr.expected_image(y, img.size, lay[5], lay[3], lay[4]), "sync=False against the host build", lay)


def test_frame_count_at_odd_n_fft(torch, pkg):
    """An odd n_fft, centred: torch.stft pads n_fft / 2 on each side, so F = 1 + (T - 1) / hop: 28 frames at n_fft 15, hop 4, T 112,
    not 29; and out_frames of the handle is the restatement's at every T up to 4 n_fft."""
    x = torch.from_numpy(np.random.default_rng(15).uniform(-1, 1, (2, 112)).astype(np.float32)).to("cuda:0")
    assert tuple(pkg.mel_spectrogram(x, 8000, n_fft=15, hop_length=4, n_mels=4).shape) == (2, 4, 28)
    assert tuple(pkg.spectrogram(x, 8000, 15, hop_length=4).shape) == (2, 8, 28)
    assert tuple(pkg.spectrogram(x, 8000, 16, hop_length=4).shape) == (2, 9, 29)
    for name in ("n15", "n3", "n2047", "tiny"):
        cfg = mr.CASES[name] if name in mr.CASES else mr.EDGE_CASES[name][0]
        with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
            for T in range(0, 4 * cfg.n_fft):
                assert ms.out_frames(T) == mr.out_frames(cfg, T), "%s T %d" % (name, T)
            if cfg.n_fft % 2:
                T = 3 * cfg.hop_length * cfg.n_fft
                assert ms.out_frames(T) == T // cfg.hop_length


@pytest.mark.parametrize("name", ["tiny", "whisper80", "uncentred"])
def test_device_impulses_come_out_as_single_table_entries(torch, pkg, name):
    """x = delta (and -0.5 delta) at j: every power is fmaf(S, S, C * C) of the handle's own table entries under j, or of the sum
    of two where the reflected margin shows j twice; the whole buffer compared as uint32, over more than two tiles."""
    cfg = mr.CASES[name].with_(n_mels=None, mel_scale=None, norm=None)
    with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
        plan = ms.plan()
        T = mr.length_for(cfg, 2 * plan["tile_frames"] + 3)
        seen_twice = 0
        for j, amp in ((cfg.n_fft // 8 + 3, 1.0), (T // 2 + 1, -0.5), (T - cfg.n_fft // 2 + 1, 1.0)):
            x = np.zeros((1, T), np.float32)
            x[0, j] = amp
            want, twice = mr.impulse_expected(cfg, plan["basis"], T, j, amp)
            assert np.count_nonzero(want) > 0
            seen_twice += twice
            for out_off, in_off in ((0, 0), (3, 1)):
                img, lay = device_image(torch, ms, cfg, x, in_off, out_off, 1)
                assert_same_image(img, mr.expected_image(want[None], img.size, lay[5], lay[3], lay[4]),
                                  "impulse %g at %d offsets %d/%d" % (amp, j, in_off, out_off), lay)
        assert (seen_twice > 0) == cfg.center


@pytest.mark.parametrize("name", ["tiny", "whisper80"])
def test_other_float_values(torch, pkg, sim, name):
    """Zeros, denormals, values whose powers overflow to inf, -0.0, an infinity and a NaN (mr.special_rows): where the host build has
    a NaN the device has one too, whatever its payload, and every other word is equal; the frames that do not cover the infinity
    or the NaN are finite."""
    for cfg in (mr.CASES[name], mr.CASES[name].with_(n_mels=None, mel_scale=None, norm=None)):
        with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
            tf = ms.plan()["tile_frames"]
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
                assert_same_image(np.where(nan, 0, img), np.where(nan, 0, want), "%s bins %d offsets %d/%d" % (name, cfg.bins, in_off, out_off), lay)


def log_inputs(cfg, tf):
    rng = np.random.default_rng(17)
    T = mr.length_for(cfg, tf + 3)
    x = mr.signal(rng, 4, T)
    x[2] = (rng.uniform(-1, 1, T) * 1e-4).astype(np.float32)
    x[2, T // 4: T // 2] = 0.0  # frames of silence: at the floor
    return x


@pytest.mark.parametrize("name", ["tiny", "whisper80"])
def test_log_modes(torch, pkg, sim, name):
    """With P the device's own mel power, held to the host build bit for bit, every mode against float64 s log(max(P, floor)):
    within LOG_ULPS float32 ulps of the result, and float(s log(floor)) exactly for P at or below the floor. The power
    spectrogram's log likewise."""
    worst = {}
    for base in (mr.CASES[name], mr.CASES[name].with_(n_mels=None, mel_scale=None, norm=None)):
        P = None
        for log, floor in ((None, 1e-10), ("ln", 1e-10), ("log10", 1e-10), ("db", 1e-10), ("log10", 1e-3), ("db", 0.5)):
            cfg = base.with_(log=log, floor=floor)
            with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
                if P is None:
                    x = log_inputs(cfg, ms.plan()["tile_frames"])
                img, lay = device_image(torch, ms, cfg, x, 1, 2, 1)
            got = mr.rows_of(img, x.shape[0], cfg.bins, mr.out_frames(cfg, x.shape[1]), lay[5], lay[3], lay[4])
            assert_same_image(img, mr.expected_image(got, img.size, lay[5], lay[3], lay[4]), "log %s: outside the output" % log, lay)
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
            print("%s bins %d log %s floor %g: %.3f ulps" % (name, cfg.bins, log, floor, u))
    print("LOG_ULPS_MEASURED %s: %s" % (name, {k: round(v, 3) for k, v in worst.items()}))
    for log, u in worst.items():
        assert u <= LOG_ULPS[log], "log %s: %.3f ulps, bound %.3f" % (log, u, LOG_ULPS[log])


def test_small_inputs_and_no_work(torch, pkg):
    """Calls without work, which touch nothing, and what the entry refuses before a launch."""
    cfg = mr.CASES["tiny"]
    with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
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


def test_python_entries(torch, pkg, sim):
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.uniform(-1, 1, (3, 2, 1500)).astype(np.float32)).to("cuda:0")
    kw = dict(n_fft=400, hop_length=160, n_mels=80, mel_scale="slaney", norm="slaney")
    keys = set(pkg._MELS)
    before = len(keys)
    y = pkg.mel_spectrogram(x, 16000, **kw)
    F = 1 + 1500 // 160
    assert tuple(y.shape) == (3, 2, 80, F) and y.is_cuda and y.dtype is torch.float32
    new = [k for k in pkg._MELS if k not in keys]
    assert len(new) == 1
    handle = pkg._MELS[new[0]]
    for a in range(3):
        for c in range(2):
            assert torch.equal(pkg.mel_spectrogram(x[a, c], 16000, **kw), y[a, c])
    assert len(pkg._MELS) == before + 1 and pkg._MELS[new[0]] is handle  # the handle of a parameter set is built once and kept
    cfg = mr.Cfg(16000, 400, 160, 400, n_mels=80, mel_scale="slaney", norm="slaney")
    rows = x.cpu().numpy().reshape(6, 1500)
    assert np.array_equal(y.cpu().numpy().reshape(6, 80, F).view(np.uint32), host_values(sim, cfg, rows).view(np.uint32))
    # a non-contiguous input, a CPU tensor and a numpy array
    t = x.transpose(0, 1)
    assert not t.is_contiguous() and torch.equal(pkg.mel_spectrogram(t, 16000, **kw), y.transpose(0, 1))
    assert torch.equal(pkg.mel_spectrogram(x.cpu(), 16000, **kw), y) and torch.equal(pkg.mel_spectrogram(x.cpu().numpy(), 16000, **kw), y)
    # another parameter set is another handle; log modes on top of the same power
    ylog = pkg.mel_spectrogram(x, 16000, log="db", floor=1e-5, **kw)
    assert len(pkg._MELS) == before + 2
    want = mr.log64(cfg.with_(log="db", floor=1e-5), y.cpu().numpy())
    assert mr.ulps32(ylog.cpu().numpy(), want).max() <= LOG_ULPS["db"]
    # spectrogram: the power itself, the mel stage applied by hand within its chain's ceiling
    p = pkg.spectrogram(x, 16000, 400, hop_length=160)
    assert tuple(p.shape) == (3, 2, 201, F)
    pcfg = cfg.with_(n_mels=None, mel_scale=None, norm=None)
    assert np.array_equal(p.cpu().numpy().reshape(6, 201, F).view(np.uint32), host_values(sim, pcfg, rows).view(np.uint32))
    d = pkg.spectrogram(x, 16000)  # torchaudio's defaults: win_length n_fft, hop win_length / 2
    assert tuple(d.shape) == (3, 2, 201, 1 + 1500 // 200)
    for bad in (x.double(), x.to(torch.int32), x.cpu().numpy().astype(np.float64)):
        with pytest.raises(ValueError):
            pkg.mel_spectrogram(bad, 16000)
    with pytest.raises(ValueError):
        pkg.mel_spectrogram(x[..., :200], 16000)  # T <= n_fft / 2: no frame
    with pytest.raises(ValueError):
        pkg.mel_spectrogram(x, 16000, n_mels=0)


def test_whisper_log_mel(torch, pkg, sim):
    """[2, 4000] of noise against the restatement on the handle's own tables with numpy's post-processing. An element's log10 is off
    by at most dmel / (mel ln 10) (the chains' ceiling) + LOG_ULPS ulps of itself; the clamp against (the maximum) - 8 passes on at
    most the largest of those in the row, and (x + 4) / 4 a quarter of it plus two roundings at magnitudes below 4."""
    rng = np.random.default_rng(23)
    x = rng.uniform(-1, 1, (2, 4000)).astype(np.float32)
    got = pkg.whisper_log_mel(torch.from_numpy(x).to("cuda:0"))
    assert tuple(got.shape) == (2, 80, 25) and got.is_cuda
    assert torch.equal(got, pkg.whisper_log_mel(x)) and torch.equal(got[1], pkg.whisper_log_mel(x[1]))
    cfg = mr.Cfg(16000, 400, 160, 400, n_mels=80, mel_scale="slaney", norm="slaney", f_max=8000.0, log="log10")
    with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
        plan = ms.plan()
    dense = mr.dense_fb(plan, 201)
    mel = mr.mel64(cfg, x, plan["basis"], dense)
    _, dmel = mr.bounds(cfg, x, plan["basis"], dense, plan["taps"])
    assert mel.min() > 1e-6, "noise keeps every filter far above the floor"
    lg = np.log10(mel)
    e = dmel / (mel * np.log(10.0)) + LOG_ULPS["log10"] * np.spacing(np.abs(lg).astype(np.float32))
    tol = e.max(axis=(1, 2), keepdims=True) / 4 + 2 * 2.0 ** -22
    want = lg[..., :-1]
    want = (np.maximum(want, want.max(axis=(1, 2), keepdims=True) - 8.0) + 4.0) / 4.0
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print("whisper_log_mel: error %.3g, tolerance %.3g" % (err.max(), tol.min()))
    assert (err <= tol).all()
    # and the torch post-processing is numpy's on the pass's own output
    raw = pkg.mel_spectrogram(x, 16000, 400, 400, 160, 0.0, 8000.0, 80, True, "slaney", "slaney", "log10", 1e-10)
    assert np.array_equal(got.cpu().numpy(), mr.whisper_post(raw.cpu().numpy()))
    assert tuple(pkg.whisper_log_mel(x, n_mels=128).shape) == (2, 128, 25)


FL = 256


@pytest.fixture(scope="module")
def files(oracle, synth, tmp_path_factory):
    """Two small 16-bit stereo files, at 44 100 and at 16 000 Hz -> paths"""
    d = tmp_path_factory.mktemp("mel")
    made = []
    for name, rate, seed in (("a44", 44100, 1), ("b16", 16000, 2)):
        cfg = oracle.make_config(FL, 16, 2, sample_rate=rate)
        path = d / (name + ".m4a")
        path.write_bytes(m4a.write_m4a(cfg, cr.file_packets(oracle, synth, cfg, 12, seed)))
        made.append(str(path))
    return made


def test_mel_of_loaded_clips(torch, pkg, files):
    """mel_spectrogram(load_clips(..., sample_rate=16000)[0], 16000, ...) is the pass over the same tensor through the raw-pointer
    entry."""
    L = 1200
    clips, lengths, rate = pkg.load_clips(files, [100, 7], L, sample_rate=16000)
    assert rate == 16000 and tuple(clips.shape) == (2, 2, L) and bool(clips.any().item())
    kw = dict(n_fft=400, hop_length=160, n_mels=64, log="log10")
    got = pkg.mel_spectrogram(clips, 16000, **kw)
    F = 1 + L // 160
    assert tuple(got.shape) == (2, 2, 64, F)
    out = torch.full((4, 64, F + 2), -7.0, dtype=torch.float32, device="cuda:0")
    flat = clips.contiguous().reshape(4, L)
    torch.cuda.synchronize()
    with pkg.NewMelSpectrogram(16000, **kw) as ms:
        ms.mel_device(flat.data_ptr(), L, 4, L, out.data_ptr(), 64 * (F + 2), F + 2, sync=True)
    assert torch.equal(out[:, :, :F].view(torch.int32), got.reshape(4, 64, F).view(torch.int32)) and bool((out[:, :, F:] == -7.0).all())


def test_cpp_mel_spectrogram(torch, pkg):
    """host/mel_spectrogram.hpp (alac::MelSpectrogram: OutFrames, Plan, MelDevice, LastMs) through the ctypes shim: the bits and the
    plan of the Python handle, and std::invalid_argument where no plan exists or the pass refuses its arguments."""
    L = mr.build_mel_shim(pkg)
    cfg = mr.Cfg(22050, 128, 40, 100, n_mels=20, mel_scale="slaney", norm="slaney", f_min=30.0, f_max=9000.0, log="ln", floor=1e-6)
    rows, T = 3, 700
    x = torch.from_numpy(mr.signal(np.random.default_rng(8), rows, T)).to("cuda:0")
    with pkg.NewMelSpectrogram(**cfg.kwargs()) as ms:
        plan = ms.plan()
        want = ms(x)
    F = want.shape[2]
    out = torch.full((rows, 20, F + 1), -7.0, dtype=torch.float32, device="cuda:0")
    of, msec = ctypes.c_uint64(0), ctypes.c_float(-1.0)
    info = np.zeros(9, np.uint32)
    basis, fb, first = np.zeros_like(plan["basis"]), np.zeros_like(plan["fb"]), np.zeros_like(plan["first"])
    torch.cuda.synchronize()

    def run(n_fft, out_bin_stride):
        return L.mel_shim_run(22050, n_fft, 100, 40, 30.0, 9000.0, 20, 1, 1, 2, 1, 1e-6, x.data_ptr(), T, rows, T, out.data_ptr(),
                              20 * (F + 1), out_bin_stride, ctypes.byref(of), info.ctypes.data, basis.ctypes.data, basis.size,
                              fb.ctypes.data, fb.size, first.ctypes.data, first.size, ctypes.byref(msec))

    assert run(128, F + 1) == 0, L.mel_shim_last_error()
    assert of.value == F == mr.out_frames(cfg, T) and msec.value > 0
    assert [int(v) for v in info] == [plan[k] for k in mr.INFO]
    assert all(np.array_equal(a.view(np.uint32), plan[k].view(np.uint32)) for a, k in ((basis, "basis"), (fb, "fb"), (first, "first")))
    assert torch.equal(out[:, :, :F].view(torch.int32), want.view(torch.int32)) and bool((out[:, :, F] == -7.0).all())
    assert run(99, F + 1) == -6 and b"no spectrogram plan" in L.mel_shim_last_error()  # win_length above n_fft
    assert run(128, F - 1) == -6 and b"stride" in L.mel_shim_last_error()
    assert torch.equal(out[:, :, :F].view(torch.int32), want.view(torch.int32)) and bool((out[:, :, F] == -7.0).all())
