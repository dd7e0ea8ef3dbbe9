"""alacgpu_fbank_device on a handle with transform = fft, on the GPU. With nothing logged the device's whole sentinel-filled buffer
is bit for bit what the host build of the same header (tests/host_sim/fbankfft_sim.cpp) writes, in every case of kf.FFT_CASES, and
within the ceilings that tests/kaldifft_ref.py derives against the step-by-step float64 restatement. The logging passes (log fbank,
log energy, MFCC) are held to the float64 of the device's own unlogged values within kr.check_logged's bounds. Then the column
arrangement, other float values, the constant row (exactly +0.0), sync=False, both layouts, kaldi_fbank / kaldi_mfcc with
transform="fft" and their cache, fft_plan() and the C entries, host/kaldi_features.hpp through a shim of its own, calls without
work and every refusal of the device entry, the handle's lifecycle, the kernel's second launch and one far stride.

Every test here needs the transform keyword: on a library without it they fail with TypeError.

No test provokes a fault: the arguments the entry refuses are refused on the host, before a launch."""
import ctypes

import numpy as np
import pytest

from tests import far_buffers as fb
from tests import kaldi_ref as kr
from tests import kaldifft_ref as kf
from tests import mel_ref as mr

pytestmark = pytest.mark.gpu

FFT = dict(transform="fft")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture(scope="module")
def sim():
    return kf.build_fbankfft_sim()


def device_image(torch, h, cfg, x, in_off=0, out_off=0, pad=0, sync=True):
    rows, T = x.shape
    lay = kr.layout(cfg, rows, T, in_off, out_off, pad)
    in_stride, in_lead, in_elems, row_stride, inner, out_lead, out_elems = lay
    dev = torch.device("cuda:0")
    host = np.full(in_elems, np.nan, np.float32)  # NaN between the rows: a read outside a row's [0, T) shows
    for r in range(rows):
        host[in_lead + r * in_stride: in_lead + r * in_stride + T] = x[r]
    src = torch.from_numpy(host).to(dev)
    buf = torch.full((out_elems,), mr.SENTINEL - (1 << 32), dtype=torch.int32, device=dev)
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    h.features_device(src.data_ptr() + 4 * in_lead, in_stride, rows, T, buf.data_ptr() + 4 * out_lead, row_stride, inner, sync=sync)
    if not sync:
        h.synchronize()
    return buf.cpu().numpy().view(np.uint32), lay


def device_values(torch, pkg, cfg, x, in_off=1, out_off=2, pad=1):
    """[rows, F, cols] float32 of a fresh FFT handle's pass, everything outside the output checked to be the sentinel"""
    with pkg.NewKaldiFeatures(**cfg.kwargs(), **FFT) as h:
        img, lay = device_image(torch, h, cfg, x, in_off, out_off, pad)
    return kr.values_of(img, lay, cfg, x.shape[0], x.shape[1], "device pass")


def assert_same_image(img, want, what, lay):
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError("%s: element %d of the buffer (rows start at %d, row stride %d, inner stride %d): got %#x, want %#x (%d "
                             "differ)" % (what, bad[0], lay[5], lay[3], lay[4], img[bad[0]], want[bad[0]], len(bad)))


@pytest.mark.parametrize("name", list(kf.FFT_CASES))
def test_device_equals_the_host_build_and_logs_within_bounds(torch, pkg, sim, name):
    """Every case at F = tile_frames - 1, tile_frames, tile_frames + 1 and 1; rows 1 and 3. Unlogged: the library's plan is the
    host build's, the whole buffer bit for bit the host build's at the offset pairs (all but the first with a frame stride of cols
    + 3; one of them with sync=False), in the layout bins at F = tile_frames + 1, and the values within kf.reference's ceiling. Then
    the case's own pass against the float64 of those values (kr.check_logged)."""
    cfg, tf, batch, radix = kf.FFT_CASES[name]
    small = name in kf.SMALL
    pre_cfg = cfg.prelog()
    worst = worst_log = 0.0
    with pkg.NewKaldiFeatures(**pre_cfg.kwargs(), **FFT) as pre_h, pkg.NewKaldiFeatures(**cfg.kwargs(), **FFT) as h, \
            pkg.NewKaldiFeatures(**pre_cfg.with_(layout="bins").kwargs(), **FFT) as bins_h:
        plan = kf.handle_plan(pre_h)
        assert (plan["tile_frames"], plan["batch_frames"], plan["radix"]) == (tf, batch, radix)
        assert kf.same_plan(plan, kf.sim_plan(sim, pre_cfg)) and kf.same_plan(kf.handle_plan(h), kf.sim_plan(sim, cfg)), \
            "the library's plan is not the host build's"
        with pytest.raises(ValueError):
            h.last_ms()  # no pass yet on this handle
        for k, rows, T, x in kf.case_runs(name):  # the CPU suite's inputs: the shares are the same numbers
            assert h.out_frames(T) == kr.out_frames(cfg, T) > 0
            what = "%s rows %d T %d" % (name, rows, T)
            y = kf.host_values(sim, pre_cfg, x)
            for j, (out_off, in_off) in enumerate(kr.OFFSETS if small else kr.OFFSETS[:2]):
                img, lay = device_image(torch, pre_h, pre_cfg, x, in_off, out_off, 3 if j else 0, sync=j != 1)
                assert_same_image(img, kr.image_of(pre_cfg, y, img.size, lay), "%s offsets %d/%d" % (what, in_off, out_off), lay)
            worst = max(worst, kf.share(pre_cfg, plan, x, y, what))
            if k == 2:
                b = pre_cfg.with_(layout="bins")
                img, lay = device_image(torch, bins_h, b, x, 1, 3, 3)
                assert_same_image(img, kr.image_of(b, y, img.size, lay), what + " layout bins", lay)
            img, lay = device_image(torch, h, cfg, x, 2, 1, 3)
            got = kr.values_of(img, lay, cfg, rows, T, what)
            worst_log = max(worst_log, kr.check_logged(cfg, got, y, what))
        assert h.last_ms() > 0 and h.out_frames(cfg.W - 1) == 0
    print("CEILING_SHARE device %s %.4f logged %.3f%s" % (name, worst, worst_log, " (MFCC)" if cfg.ceps else ""))


def test_column_arrangement(torch, pkg):
    """kr.check_arrangement on an FFT handle: the place of every column and the factor of C0 under htk_compat"""
    share = kr.check_arrangement(lambda cfg, x: device_values(torch, pkg, cfg, x))
    print("sqrt(2) C0 on the device: largest error / bound %.3f" % share)


@pytest.mark.parametrize("name", kr.SPECIAL_CASES)
def test_other_float_values(torch, pkg, sim, name):
    """Zeros, denormals, values whose powers overflow, -0.0, an infinity and a NaN (mr.special_rows). Unlogged: where the host
    build has a NaN the device has one too, whatever its payload, and every other word is equal; kr.check_special_unlogged: only
    the frames that read the non-finite sample are non-finite. Then the case's own logging pass (kr.check_special_logged)."""
    cfg, T, x = kr.special_input(name)
    pre_cfg = cfg.prelog()
    y = kf.host_values(sim, pre_cfg, x)
    with pkg.NewKaldiFeatures(**pre_cfg.kwargs(), **FFT) as h:
        for out_off, in_off in ((0, 0), (1, 3)):
            img, lay = device_image(torch, h, pre_cfg, x, in_off, out_off, 2)
            want = kr.image_of(pre_cfg, y, img.size, lay)
            nan = np.isnan(want.view(np.float32))
            assert nan.any() and np.isnan(img.view(np.float32)[nan]).all(), "a NaN of the host build is none on the device"
            assert_same_image(np.where(nan, 0, img), np.where(nan, 0, want), "%s offsets %d/%d" % (name, in_off, out_off), lay)
    P = kr.values_of(img, lay, pre_cfg, 6, T, name)
    kr.check_special_unlogged(pre_cfg, T, x, P)
    share = kr.check_special_logged(cfg, device_values(torch, pkg, cfg, x, 2, 1, 3), P, name)
    print("%s: largest error / bound of the logs on the device %.3f" % (name, share))


def test_constant_row(torch, pkg, sim):
    """A constant 0.5 with DC removal at scale 1 and 32768 is exactly +0.0 in every unlogged column, float32(ln 2^-23) logged"""
    def run(cfg, x):
        got = device_values(torch, pkg, cfg, x)
        assert kr.same_bits(got, kf.host_values(sim, cfg, x))
        return got
    kf.check_constant(run, None)


def test_python_entries(torch, pkg, sim):
    """kaldi_fbank / kaldi_mfcc with transform="fft": unlogged bit for bit the FFT host build's, logged within the bounds; the
    cache keeps a direct and an FFT handle apart; transform="direct" equals no keyword, bit for bit; other strings are refused"""
    cfg = kr.Cfg(8000, 50, 20, low=23.0)  # 6.25 ms and 2.5 ms at 8 kHz; a low_freq that no other test's cached handle has
    x = kr.signal(np.random.default_rng(21), 6, 1330)
    ms = dict(sample_frequency=8000, frame_length=6.25, frame_shift=2.5, low_freq=23.0)
    pre = kf.host_values(sim, cfg.prelog(), x)
    before = set(pkg._KALDIS)
    for src in (x.reshape(2, 3, -1), torch.from_numpy(x).cuda().reshape(2, 3, -1)):
        got = pkg.kaldi_fbank(src, use_log_fbank=False, transform="fft", **ms)
        assert got.is_cuda and tuple(got.shape) == (2, 3, 65, 23)
        assert np.array_equal(got.cpu().numpy().reshape(pre.shape).view(np.uint32), pre.view(np.uint32))
    assert len(set(pkg._KALDIS) - before) == 1
    plain = pkg.kaldi_fbank(x, use_log_fbank=False, **ms)
    direct = pkg.kaldi_fbank(x, use_log_fbank=False, transform="direct", **ms)
    added = set(pkg._KALDIS) - before
    assert len(added) == 2 and sorted(pkg._KALDIS[k].transform for k in added) == ["direct", "fft"]
    assert torch.equal(plain.view(torch.int32), direct.view(torch.int32))
    assert not torch.equal(plain.view(torch.int32), got.reshape(plain.shape).view(torch.int32)), "the two transforms share a handle"
    got = pkg.kaldi_fbank(x, transform="fft", **ms).cpu().numpy()
    kr.check_logged(cfg, got, pre, "kaldi_fbank fft")
    bins = pkg.kaldi_fbank(x, layout="bins", transform="fft", **ms)
    assert tuple(bins.shape) == (6, 23, 65) and np.array_equal(bins.cpu().numpy().transpose(0, 2, 1), got)
    got = pkg.kaldi_mfcc(torch.from_numpy(x[0]), transform="fft", **ms).cpu().numpy()
    assert got.shape == (65, 13)
    kr.check_logged(cfg.with_(ceps=13), got[None], pre[:1], "kaldi_mfcc fft")
    for bad in ("FFT", "", None, 1):
        with pytest.raises(ValueError):
            pkg.kaldi_fbank(x, transform=bad, **ms)
        with pytest.raises(ValueError):
            pkg.kaldi_mfcc(x, transform=bad, **ms)
    with pytest.raises(ValueError):
        pkg.kaldi_fbank(x, transform="fft", round_to_power_of_two=False, sample_frequency=8000, frame_length=1.75, frame_shift=0.5)  # W 14
    with pytest.raises(ValueError):
        pkg.kaldi_fbank(x, transform="fft", dither=1.0, **ms)


def test_fft_plan_and_the_c_entries(torch, pkg, sim):
    """fft_plan() on both kinds of handle, plan()["basis"] empty on an FFT handle, transform = 2 and the sizes without a plan
    through the C ABI (ALACGPU_E_ARG, a message that names the rule, no handle), capacities below the tables"""
    cfg = kf.FFT_CASES["n30"][0]
    L = pkg.lib()
    with pkg.NewKaldiFeatures(**cfg.kwargs(), **FFT) as h, pkg.NewKaldiFeatures(**cfg.kwargs()) as d:
        assert h.transform == "fft" and d.transform == "direct"
        fp, sp = kf.handle_plan(h), kf.sim_plan(sim, cfg)
        assert kf.same_plan(fp, sp) and fp["radix"] == [5, 3] and fp["transform"] == 1 and fp["window"].shape == (30,)
        assert h.plan()["basis"].shape == (2, 0, 30) and d.plan()["basis"].shape == (2, 16, 30)
        dp = d.fft_plan()
        assert dp["transform"] == 0 and dp["radix"] == [] and dp["n_passes"] == dp["batch_frames"] == dp["pitch"] == 0
        assert dp["window"].size == dp["twiddle"].size == 0
        assert (dp["tile_frames"], dp["lds_bytes"]) == (d.plan()["tile_frames"], d.plan()["lds_bytes"])
        for k in kf.TABLES:
            assert np.array_equal(h.plan()[k].view(np.uint32), d.plan()[k].view(np.uint32)), k
        info = pkg.FbankFftInfo()
        small = np.zeros(3, np.float32)
        assert L.alacgpu_fbank_fft_plan(h._h, ctypes.byref(info), small.ctypes.data, small.size, None, 0) == -2
        assert L.alacgpu_fbank_fft_plan(h._h, ctypes.byref(info), None, 0, small.ctypes.data, small.size) == -2
        assert not small.any()
        basis = np.full(8, 7.0, np.float32)  # an FFT handle copies no basis, whatever the capacity
        pinfo = pkg.FbankInfo()
        assert L.alacgpu_fbank_plan(h._h, ctypes.byref(pinfo), basis.ctypes.data, basis.size, None, 0, None, 0, None, 0, None, 0) == 0
        assert (basis == 7.0).all()
    assert L.alacgpu_fbank_fft_plan(None, None, None, 0, None, 0) == -2
    c = pkg._fbank_config(**{k: v for k, v in zip(
        ("sample_rate", "frame_length", "frame_shift", "num_mel_bins", "num_ceps", "round_to_power_of_two", "snip_edges",
         "remove_dc_offset", "window_type", "use_log_fbank", "use_energy", "raw_energy", "htk_compat", "use_power", "log_energy", "layout",
         "preemphasis_coefficient", "blackman_coeff", "low_freq", "high_freq", "energy_floor", "scale", "cepstral_lifter", "dither",
         "vtln_warp"),
        (8000, 10, 4, 23, 0, True, True, True, "povey", True, False, True, False, True, True, "frames", 0.97, 0.42, 20.0, 0.0, 1.0, 1.0,
         22.0, 0.0, 1.0))})
    for transform in (2, 3, 0xFFFFFFFF):
        out = ctypes.c_void_p(5)
        assert L.alacgpu_fbank_create_transform(0, ctypes.byref(c), transform, ctypes.byref(out)) == -2 and not out.value
        assert b"ALACGPU_FBANK_TRANSFORM_FFT (1)" in L.alacgpu_last_error()
    for value in (0, 1):
        out = ctypes.c_void_p()
        assert L.alacgpu_fbank_create_transform(0, ctypes.byref(c), value, ctypes.byref(out)) == 0 and out.value
        info = pkg.FbankFftInfo()
        assert L.alacgpu_fbank_fft_plan(out, ctypes.byref(info), None, 0, None, 0) == 0 and info.transform == value
        L.alacgpu_fbank_destroy(out)
    for bad in kf.REFUSED:
        with pytest.raises(ValueError, match="2\\^a 3\\^b 5\\^c"):
            pkg.NewKaldiFeatures(**bad.kwargs(), **FFT)
        pkg.NewKaldiFeatures(**bad.kwargs()).close()  # the direct transform takes it
    with pytest.raises(ValueError):
        pkg.NewKaldiFeatures(**cfg.kwargs(), transform="stockham")


def test_cpp_entry(torch, pkg, sim):
    """host/kaldi_features.hpp with a transform: NewKaldiFeatures, Plan (an empty basis), FftPlan, FeaturesDevice, LastMs;
    std::invalid_argument for a size without an FFT plan and for a transform above 1"""
    shim = kf.build_fbankfft_shim(pkg)
    cfg = kf.FFT_CASES["e_last_1"][0].prelog()
    x = kr.signal(np.random.default_rng(2), 3, kr.length_for(cfg, 65))
    T, F = x.shape[1], 65
    y = kf.host_values(sim, cfg, x)
    with pkg.NewKaldiFeatures(**cfg.kwargs(), **FFT) as h:
        c = h.config
        want_info = [h.plan()[k] for k in kr.INFO]
        fp = h.fft_plan()
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros((3, F, cfg.cols), dtype=torch.float32, device="cuda:0")
    frames, info, ms = ctypes.c_uint64(), (ctypes.c_uint32 * 10)(), ctypes.c_float()
    basis, fft_info, sizes = ctypes.c_uint64(9), (ctypes.c_uint32 * 16)(), (ctypes.c_uint64 * 2)()

    def run(transform, inner=cfg.cols):
        torch.cuda.synchronize()
        return shim.fbankfft_shim_run(ctypes.addressof(c), transform, d_in.data_ptr(), T, 3, T, d_out.data_ptr(), F * cfg.cols, inner,
                                      ctypes.addressof(frames), ctypes.addressof(info), ctypes.addressof(basis),
                                      ctypes.addressof(fft_info), ctypes.addressof(sizes), ctypes.addressof(ms))
    assert run(1) == 0, shim.fbankfft_shim_last_error()
    assert frames.value == F and list(info) == want_info and ms.value > 0 and basis.value == 0
    assert list(fft_info)[:6] == [fp[k] for k in kf.FFT_INFO] and list(fft_info)[6:8] == fp["radix"] == [4, 2]
    assert list(sizes) == [fp["window"].size, fp["twiddle"].size]
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), y.view(np.uint32))
    assert run(0) == 0 and basis.value == 2 * 9 * 10 and list(fft_info)[0] == 0 and list(sizes) == [0, 0]  # the default transform
    assert not np.array_equal(d_out.cpu().numpy().view(np.uint32), y.view(np.uint32))
    assert run(2) == -6 and run(1, cfg.cols - 1) == -6
    c.round_to_power_of_two, c.frame_length = 0, 14
    assert run(1) == -6 and b"2^a 3^b 5^c" in shim.fbankfft_shim_last_error()


def test_small_inputs_and_no_work(torch, pkg):
    """Calls without work, which touch nothing, and what the entry refuses before a launch, on an FFT handle"""
    for cfg in (kr.W10, kr.W10.with_(layout="bins")):
        T = 30
        F = kr.out_frames(cfg, T)  # 6 frames of 23
        lines, length = kr.out_shape(cfg, F)
        span = (lines - 1) * length + length
        with pkg.NewKaldiFeatures(**cfg.kwargs(), **FFT) as h:
            buf = torch.full((1024,), 7.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            B = buf.data_ptr()
            O = B + 2048
            h.features_device(B, T, 0, T, O, span, length)            # no rows
            h.features_device(B, T, 2, cfg.W - 1, O, span, length)    # rows shorter than a frame
            h.features_device(None, 0, 0, 0, None, 0, 0)
            h.synchronize()
            assert bool((buf == 7.0).all().item())
            for bad in [(None, T, 2, T, O, span, length), (B, T, 2, T, None, span, length), (B + 2, T, 2, T, O, span, length),
                        (B + 1, T, 2, T, O, span, length), (B, T, 2, T, O + 1, span, length), (B, T, 2, T, O + 2, span, length),
                        (B, T - 1, 2, T, O, span, length), (B, T, 2, T, O, span, length - 1), (B, T, 2, T, O, span - 1, length),
                        (B, 1 << 62, 2, T, O, span, length), (B, T, 2, T, O, 1 << 62, length), (B, T, 2, T, O, 1 << 62, 1 << 62),
                        (B, T, 2, (1 << 61) + 1, O, span, length)]:
                with pytest.raises(ValueError):
                    h.features_device(*bad)
            h.synchronize()
            assert bool((buf == 7.0).all().item()), "a refused call wrote"
            with pytest.raises(ValueError):
                h.last_ms()  # nothing was launched
            h.features_device(B, T, 2, T, O, span, length)  # and the same arguments, in order, are a pass
            assert h.last_ms() > 0 and not bool((buf[512:512 + 2 * span] == 7.0).any().item()) and bool((buf[:512] == 7.0).all().item())
            assert bool((buf[512 + 2 * span:] == 7.0).all().item())


# ---- the lifecycle tests/test_gpu_pass_handles.py asks of the other handles ----------------------------------------------------
ROWS, T64 = 2, 64
KALDI_FRAMES = 1 + (T64 - 16) // 4


def rows_of(torch):
    return torch.from_numpy(np.random.default_rng(64).uniform(-1.0, 1.0, (ROWS, T64)).astype(np.float32)).to("cuda:0")


def assert_closed(h, x):
    assert h.out_frames(T64) == 0
    for call in (h.synchronize, h.last_ms, h.plan, h.fft_plan, lambda: h(x)):
        with pytest.raises(ValueError):
            call()


def test_lifecycle_of_an_fft_handle(torch, pkg):
    def new():
        return pkg.NewKaldiFeatures(16000, 16, 4, num_mel_bins=4, low_freq=20.0, **FFT)
    x = rows_of(torch)
    h = new()
    with pytest.raises(ValueError):
        h.last_ms()  # no pass yet on this handle
    h.features_device(0, T64, 0, T64, 0, 4 * KALDI_FRAMES, 4)
    with pytest.raises(ValueError):
        h.last_ms()  # nothing was launched
    out = h(x)
    assert tuple(out.shape) == (ROWS, KALDI_FRAMES, 4) and out.dtype is torch.float32 and out.device == x.device
    assert h.out_frames(T64) == KALDI_FRAMES and h.last_ms() > 0
    h.synchronize()
    assert bool(torch.isfinite(out).all().item())
    h.close()
    h.close()  # a second close is harmless
    assert_closed(h, x)
    with new() as g:
        assert g.out_frames(T64) > 0
    assert_closed(g, x)  # leaving the with block closed it


def test_the_module_entry_keeps_one_fft_handle_per_parameter_set(torch, pkg):
    def entry(x):
        return pkg.kaldi_fbank(x, 16000, frame_length=1.0, frame_shift=0.25, num_mel_bins=4, low_freq=21.0, **FFT)
    x = rows_of(torch)
    before = set(pkg._KALDIS)
    first = entry(x)
    added = set(pkg._KALDIS) - before
    assert len(added) == 1, "the first call adds exactly one handle"
    handle = pkg._KALDIS[next(iter(added))]
    second = entry(x)
    assert set(pkg._KALDIS) - before == added and pkg._KALDIS[next(iter(added))] is handle, "the second call adds none"
    assert tuple(first.shape) == (ROWS, KALDI_FRAMES, 4) and torch.equal(first.view(torch.int32), second.view(torch.int32))


# ---- the second launch, as tests/test_gpu_tile_slices.py has it for alac_fbank_rows ---------------------------------------------
SLICE = 1 << 22
N_ROWS = SLICE + 4099
LEAD, TAIL = 9, 8


def test_second_launch_of_alac_fbankfft_rows(torch, pkg, sim):
    """N = 2^22 + 4 099 rows of 6 samples, frame length 4, shift 2, one mel bin and the energy column, nothing logged: two frames
    of 2 columns, tile_frames 64, so tiles_per_row = 1, tile = row and the second launch has first_tile = 2^22. Row r is class r % 7
    (2^22 = 2 mod 7); the expectation is the host build's output for the 7 rows (101 MB in, 67 MB out).

    A launch that ignored first_tile would compute rows 0 .. 4 098 again and leave the rows from 2^22 on unwritten (the
    sentinel); one that read from the batch's start would give row 2^22 + j the features of row j, of another class."""
    cfg = kr.Cfg(8000, 4, 2, mels=1, energy=True, log=False, log_energy=False)
    T, F, cols = 6, 2, 2
    rows7 = np.random.default_rng(15).uniform(-1, 1, (7, T)).astype(np.float32)
    rows7[3] = [1.0, -1.0, 1.0, -1.0, 1.0, -1.0]
    want7 = kf.host_values(sim, cfg, rows7)
    assert kr.out_frames(cfg, T) == F and want7.shape == (7, F, cols)
    assert all(len(set(want7[:, 0, c].tolist())) == 7 for c in range(cols)), "the 7 rows are not distinct in both columns"
    x = torch.from_numpy(rows7).to("cuda:0").repeat(-(-N_ROWS // 7), 1)[:N_ROWS].contiguous()
    fill = mr.SENTINEL - (1 << 32)
    elems = N_ROWS * F * cols
    buf = torch.full((LEAD + elems + TAIL,), fill, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with pkg.NewKaldiFeatures(**cfg.kwargs(), **FFT) as h:
        assert h.out_frames(T) == F and h.fft_plan()["tile_frames"] == 64 and h.fft_plan()["radix"] == [2]
        h.features_device(x.data_ptr(), T, N_ROWS, T, buf.data_ptr() + 4 * LEAD, F * cols, cols, sync=True)
    row = torch.from_numpy(np.ascontiguousarray(want7).view(np.int32).reshape(-1)).to("cuda:0")
    body = buf[LEAD:LEAD + elems]
    period = row.numel()
    full = elems // period
    bad = torch.nonzero((body[:full * period].view(full, period) != row).any(dim=1))[:4].flatten().tolist()
    assert not bad, "periods %s of %d elements differ from the expectation" % (bad, period)
    assert torch.equal(body[full * period:], row[:elems - full * period]), "the last, short period differs"
    assert bool((buf[:LEAD] == fill).all()) and bool((buf[LEAD + elems:] == fill).all()), "a sentinel around the tensor is gone"


# ---- one far stride, as tests/test_gpu_far_strides.py::test_kaldi_features_with_far_strides --------------------------------------
def test_fft_features_with_a_far_input_stride(torch, pkg, sim):
    """alacgpu_fbank_device on an FFT handle, w10 with nothing logged, three rows, in_row_stride 2^29 - 101 elements: row 2
    straddles input byte 2^32. [rows][F][cols] is the host build's bit for bit, every other element the sentinel, the input
    unchanged. A 32-bit row * stride * 4 reads row 2 from the NaN in front of row 0. Peak device memory 4 GiB."""
    fb._need_gb(torch, 10)
    cfg = kf.FFT_CASES["w10"][0].prelog()
    R, T = 3, kr.length_for(cfg, 200)
    F = kr.out_frames(cfg, T)
    x = kr.signal(np.random.default_rng(3), R, T, 0.3)
    y = kf.host_values(sim, cfg, x)
    in_stride = (fb.LINE // 8) - 101
    fill = mr.SENTINEL - (1 << 32)
    src = fb.Far(torch, torch.int32, (R - 1) * in_stride + T + 8, 0x7FC00000, lead=5)
    dst = fb.Far(torch, torch.int32, R * F * cfg.cols + 8, fill, lead=6)
    d_x = torch.from_numpy(x.view(np.int32)).to("cuda:0")
    in_rows = [(r, r * in_stride, d_x[r], T) for r in range(R)]
    fb.assert_crosses([r[1] for r in in_rows], [r[3] for r in in_rows], 4, fb.LINE, what="far input stride")
    for _, off, t, _ in in_rows:
        src.place(off, t)
    torch.cuda.synchronize()
    with pkg.NewKaldiFeatures(**cfg.kwargs(), **FFT) as h:
        h.features_device(src.ptr(), in_stride, R, T, dst.ptr(), F * cfg.cols, cfg.cols, sync=True)
    d_y = torch.from_numpy(np.ascontiguousarray(y).view(np.int32)).to("cuda:0")
    out_rows = [(r, r * F * cfg.cols, d_y[r].reshape(-1), F * cfg.cols) for r in range(R)]
    fb.check_footprints(torch, dst, out_rows, "far input stride", unit="row")
    fb.check_footprints(torch, src, in_rows, "far input stride: the input afterwards", unit="row")
