"""alacgpu_fbank_device on the GPU. With nothing logged (use_log_fbank off, the energy column as the sum itself) the device's
whole sentinel-filled buffer is bit for bit what the host build of the same header (tests/host_sim/fbank_sim.cpp) writes, in
every case of kr.CASES, and within the derived ceilings against the step-by-step float64 restatement. The logging passes (log
fbank, log energy, MFCC) are held to the float64 ln (and DCT, lifter) of the device's own bit-checked unlogged values from that
second pass, within twice the 2.23 float32 ulps DESIGN.md §14 measured for this device's logf; values at or below 2^-23 give
ln(2^-23) exactly. Impulses come out as table entries; sync=False, both layouts, the Python entries (kaldi_fbank, kaldi_mfcc)
and host/kaldi_features.hpp through tests/host_sim/fbank_shim.cpp are covered; so are the place of every column and sqrt(2)
C0 under htk_compat from the device's own outputs (kr.check_arrangement), the layout bins of every case with a DCT or an energy
column, samples outside the audio range, silence, a constant row, calls without work and kaldi_fbank behind load_clips.

The values of the host build do not depend on where the buffers lie (tests/test_fbank_host.py runs it at every offset), so it
runs once per (parameters, rows, length) here and the device is held to its values at every offset.

No test provokes a fault: the arguments the entry refuses are refused on the host, before a launch."""
import ctypes

import numpy as np
import pytest

from tests import clip_ref as cr
from tests import kaldi_ref as kr
from tests import m4a
from tests import mel_ref as mr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture(scope="module")
def sim():
    return kr.build_fbank_sim()


def device_image(torch, kf, cfg, x, in_off=0, out_off=0, pad=0, sync=True):
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
    kf.features_device(src.data_ptr() + 4 * in_lead, in_stride, rows, T, buf.data_ptr() + 4 * out_lead, row_stride, inner, sync=sync)
    if not sync:
        kf.synchronize()
    return buf.cpu().numpy().view(np.uint32), lay


def device_values(torch, pkg, cfg, x, in_off=1, out_off=2, pad=1):
    """[rows, F, cols] float32 of a fresh handle's pass, everything outside the output checked to be the sentinel"""
    with pkg.NewKaldiFeatures(**cfg.kwargs()) as kf:
        img, lay = device_image(torch, kf, cfg, x, in_off, out_off, pad)
    return kr.values_of(img, lay, cfg, x.shape[0], x.shape[1], "device pass")


def assert_same_image(img, want, what, lay):
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError("%s: element %d of the buffer (rows start at %d, row stride %d, inner stride %d): got %#x, want %#x (%d "
                             "differ)" % (what, bad[0], lay[5], lay[3], lay[4], img[bad[0]], want[bad[0]], len(bad)))


@pytest.mark.parametrize("name", list(kr.CASES))
def test_device_equals_the_host_build_and_logs_within_bounds(torch, pkg, sim, name):
    """Every case at F = tile_frames - 1, tile_frames, tile_frames + 1 and 1; rows 1 and 3. Unlogged: the library's plan is the
    host build's, the whole buffer bit for bit the host build's at the four offset pairs (the last three with a frame stride of
    cols + 3; one of them with sync=False), in the layout bins at F = tile_frames + 1, and the values within the ceilings of
    kr.prelog_bounds. Then the case's own pass against the float64 of those values (kr.check_logged)."""
    cfg, tf = kr.CASES[name]
    small = name in kr.SMALL
    pre_cfg = cfg.prelog()
    rng = np.random.default_rng(len(name) + cfg.W)
    worst = worst_log = 0.0
    with pkg.NewKaldiFeatures(**pre_cfg.kwargs()) as pre_kf, pkg.NewKaldiFeatures(**cfg.kwargs()) as kf, \
            pkg.NewKaldiFeatures(**pre_cfg.with_(layout="bins").kwargs()) as bins_kf:
        plan = pre_kf.plan()
        assert kf.plan()["tile_frames"] == tf == kr.lds_rule(cfg)[0]
        assert kr.same_plan(plan, kr.sim_plan(sim, pre_cfg)) and kr.same_plan(kf.plan(), kr.sim_plan(sim, cfg)), \
            "the library's plan is not the host build's"
        with pytest.raises(ValueError):
            kf.last_ms()  # no pass yet on this handle
        for k, T in enumerate(kr.case_lengths(cfg, tf)):
            assert kf.out_frames(T) == kr.out_frames(cfg, T) > 0
            for rows in (1, 3) if small or k == 2 else (1,):
                x = kr.signal(rng, rows, T, 0.3 if rows == 3 else 0.0)
                what = "%s rows %d T %d" % (name, rows, T)
                y = kr.host_values(sim, pre_cfg, x)
                for j, (out_off, in_off) in enumerate(kr.OFFSETS if small else kr.OFFSETS[:2]):
                    img, lay = device_image(torch, pre_kf, pre_cfg, x, in_off, out_off, 3 if j else 0, sync=j != 1)
                    assert_same_image(img, kr.image_of(pre_cfg, y, img.size, lay), "%s offsets %d/%d" % (what, in_off, out_off), lay)
                ref, lim = kr.prelog_bounds(pre_cfg, plan, x)
                worst = max(worst, kr.assert_within(y, ref, lim, what))
                if k == 2:
                    b = pre_cfg.with_(layout="bins")
                    img, lay = device_image(torch, bins_kf, b, x, 1, 3, 3)
                    assert_same_image(img, kr.image_of(b, y, img.size, lay), what + " layout bins", lay)
                img, lay = device_image(torch, kf, cfg, x, 2, 1, 3)
                got = kr.values_of(img, lay, cfg, rows, T, what)
                worst_log = max(worst_log, kr.check_logged(cfg, got, y, what))
        assert kf.last_ms() > 0 and kf.out_frames(cfg.W - 1) == 0
    print("%s: largest error / bound on the device: %.3f unlogged (ceilings), %.3f logged%s" %
          (name, worst, worst_log, " (MFCC)" if cfg.ceps else ""))


@pytest.mark.parametrize("name", kr.IMPULSE_CASES)
def test_impulses_are_table_entries(torch, pkg, sim, name):
    """remove_dc_offset off, nothing logged: row r is +0.0 with 1.0 at the r-th position of the first 3 W and the last 2 W samples;
    the device's whole buffer bit for bit what the plan's tables under the impulse give"""
    cfg, T, js = kr.impulse_batch(name)
    x = np.zeros((len(js), T), np.float32)
    x[np.arange(len(js)), js] = 1.0
    with pkg.NewKaldiFeatures(**cfg.kwargs()) as kf:
        plan = kf.plan()
        assert kr.same_plan(plan, kr.sim_plan(sim, cfg))
        want = np.stack([kr.impulse_expected(cfg, plan, T, j)[0] for j in js])
        img, lay = device_image(torch, kf, cfg, x, 3, 1, 3)
    assert_same_image(img, kr.image_of(cfg, want, img.size, lay), name, lay)
    assert want.any()


def test_python_entries(torch, pkg, sim):
    """kaldi_fbank / kaldi_mfcc: torchaudio's keyword names, milliseconds resolved as torchaudio does, [..., T] from CUDA, CPU
    and numpy inputs; unlogged bit for bit the host build's, logged within the bounds; subtract_mean; layout; the refusals"""
    cfg = kr.Cfg(8000, 50, 20)  # 6.25 ms and 2.5 ms at 8 kHz
    rng = np.random.default_rng(21)
    x = kr.signal(rng, 6, 1330)
    ms = dict(sample_frequency=8000, frame_length=6.25, frame_shift=2.5)
    pre = kr.host_values(sim, cfg.prelog(), x)
    for src in (x.reshape(2, 3, -1), torch.from_numpy(x).reshape(2, 3, -1), torch.from_numpy(x).cuda().reshape(2, 3, -1)):
        got = pkg.kaldi_fbank(src, use_log_fbank=False, **ms)
        assert got.is_cuda and tuple(got.shape) == (2, 3, 65, 23)
        assert np.array_equal(got.cpu().numpy().reshape(pre.shape).view(np.uint32), pre.view(np.uint32))
    got = pkg.kaldi_fbank(x, **ms).cpu().numpy()
    kr.check_logged(cfg, got, pre, "kaldi_fbank")
    bins = pkg.kaldi_fbank(x, layout="bins", **ms)
    assert tuple(bins.shape) == (6, 23, 65) and np.array_equal(bins.cpu().numpy().transpose(0, 2, 1), got)
    sub = pkg.kaldi_fbank(x, subtract_mean=True, **ms).cpu().numpy()
    # a float32 mean over F values and one subtraction, whatever the order of the sum: (F + 2) u of the largest value
    want = got.astype(np.float64) - got.astype(np.float64).mean(axis=1, keepdims=True)
    assert np.abs(sub - want).max() <= (got.shape[1] + 2) * kr.U * np.abs(got).max()
    e_cfg = cfg.with_(energy=True, scale=32768.0)
    e_pre = kr.host_values(sim, e_cfg.prelog(), x)
    got = pkg.kaldi_fbank(x, use_energy=True, scale=32768.0, **ms).cpu().numpy()
    assert got.shape == (6, 65, 24)
    kr.check_logged(e_cfg, got, e_pre, "kaldi_fbank with energy")
    m_cfg = cfg.with_(ceps=13)
    got = pkg.kaldi_mfcc(torch.from_numpy(x[0]), **ms).cpu().numpy()
    assert got.shape == (65, 13)
    kr.check_logged(m_cfg, got[None], pre[:1], "kaldi_mfcc")
    for kw in (dict(dither=1.0), dict(vtln_warp=1.1), dict(use_energy=True, raw_energy=False), dict(window_type="hann"),
               dict(layout="time"), dict(num_mel_bins=0)):
        with pytest.raises(ValueError):
            pkg.kaldi_fbank(x, **dict(ms, **kw))
    with pytest.raises(ValueError):
        pkg.kaldi_fbank(x, use_power=False, **ms)
    with pytest.raises(ValueError):
        pkg.kaldi_mfcc(x, num_ceps=24, **ms)
    with pytest.raises(ValueError):
        pkg.kaldi_fbank(x[:, :49], **ms)  # T < W has no frame
    with pytest.raises(ValueError):
        pkg.kaldi_fbank(x.astype(np.float64), **ms)


def test_cpp_entry(torch, pkg, sim):
    """host/kaldi_features.hpp: NewKaldiFeatures, OutFrames, Plan, FeaturesDevice, LastMs; std::invalid_argument for no plan"""
    shim = kr.build_fbank_shim(pkg)
    cfg = kr.CASES["e_last_1"][0].prelog()
    x = kr.signal(np.random.default_rng(2), 3, kr.length_for(cfg, 65))
    T, F = x.shape[1], 65
    y = kr.host_values(sim, cfg, x)
    with pkg.NewKaldiFeatures(**cfg.kwargs()) as kf:
        c = kf.config
        want_info = [kf.plan()[k] for k in kr.INFO]
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros((3, F, cfg.cols), dtype=torch.float32, device="cuda:0")
    frames, info, ms = ctypes.c_uint64(), (ctypes.c_uint32 * 10)(), ctypes.c_float()
    torch.cuda.synchronize()
    rc = shim.fbank_shim_run(ctypes.addressof(c), d_in.data_ptr(), T, 3, T, d_out.data_ptr(), F * cfg.cols, cfg.cols,
                             ctypes.addressof(frames), ctypes.addressof(info), ctypes.addressof(ms))
    assert rc == 0, shim.fbank_shim_last_error()
    assert frames.value == F and list(info) == want_info and ms.value > 0
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), y.view(np.uint32))
    c.dither = 1.0
    assert shim.fbank_shim_run(ctypes.addressof(c), d_in.data_ptr(), T, 3, T, d_out.data_ptr(), F * cfg.cols, cfg.cols,
                               ctypes.addressof(frames), ctypes.addressof(info), ctypes.addressof(ms)) == -6
    c.dither = 0.0
    assert shim.fbank_shim_run(ctypes.addressof(c), d_in.data_ptr(), T, 3, T, d_out.data_ptr(), F * cfg.cols, cfg.cols - 1,
                               ctypes.addressof(frames), ctypes.addressof(info), ctypes.addressof(ms)) == -6


def test_column_arrangement(torch, pkg):
    """kr.check_arrangement on the device: the place of every column and the factor of C0 under htk_compat, without the
    restatement and without the host build"""
    share = kr.check_arrangement(lambda cfg, x: device_values(torch, pkg, cfg, x))
    print("sqrt(2) C0 on the device: largest error / bound %.3f" % share)


@pytest.mark.parametrize("name", [k for k, (c, _) in kr.CASES.items() if c.ceps or c.energy])
def test_layout_bins_of_the_dct_and_energy_passes(torch, pkg, name):
    """Every case with a DCT or an energy column, its own configuration (logs, DCT and all) at F = tile_frames + 1, rows 3: the
    whole image of layout="bins" (offsets 1 / 3, a bin stride of F + 3) is the transpose of the layout frames' output of the same
    parameters, bit for bit, and the sentinel everywhere else. For MFCC this is alacmel::store_tile out of the cepstral tile."""
    cfg, tf = kr.CASES[name]
    x = kr.signal(np.random.default_rng(12), 3, kr.length_for(cfg, tf + 1))
    want = device_values(torch, pkg, cfg, x)
    bins = cfg.with_(layout="bins")
    with pkg.NewKaldiFeatures(**bins.kwargs()) as kf:
        img, lay = device_image(torch, kf, bins, x, 3, 1, 3)
    assert want.shape == (3, tf + 1, cfg.cols) and len(np.unique(want)) > tf + 1  # (with 2048 bins most are at the floor)
    assert_same_image(img, kr.image_of(bins, want, img.size, lay), name + " layout bins", lay)


@pytest.mark.parametrize("name", kr.SPECIAL_CASES)
def test_other_float_values(torch, pkg, sim, name):
    """Zeros, denormals, values whose powers overflow, -0.0, an infinity and a NaN (mr.special_rows). Unlogged: where the host
    build has a NaN the device has one too, whatever its payload, and every other word is equal; kr.check_special_unlogged. Then
    the case's own logging pass against the device's unlogged values (kr.check_special_logged), and the floors of the energy of
    silence."""
    cfg, T, x = kr.special_input(name)
    pre_cfg = cfg.prelog()
    y = kr.host_values(sim, pre_cfg, x)
    with pkg.NewKaldiFeatures(**pre_cfg.kwargs()) as kf:
        for out_off, in_off in ((0, 0), (1, 3)):
            img, lay = device_image(torch, kf, pre_cfg, x, in_off, out_off, 2)
            want = kr.image_of(pre_cfg, y, img.size, lay)
            nan = np.isnan(want.view(np.float32))
            assert nan.any() and np.isnan(img.view(np.float32)[nan]).all(), "a NaN of the host build is none on the device"
            assert_same_image(np.where(nan, 0, img), np.where(nan, 0, want), "%s offsets %d/%d" % (name, in_off, out_off), lay)
    P = kr.values_of(img, lay, pre_cfg, 6, T, name)
    kr.check_special_unlogged(pre_cfg, T, x, P)
    got = device_values(torch, pkg, cfg, x, 2, 1, 3)
    share = kr.check_special_logged(cfg, got, P, name)
    if cfg.energy:
        floor = np.float32(0.0) if cfg.efloor > 0.0 else kr.LOG_EPS32
        assert cfg.efloor in (0.0, 1.0) and (got[0, :, 0].view(np.uint32) == floor.view(np.uint32)).all()
    print("%s: largest error / bound of the logs on the device %.3f" % (name, share))


@pytest.mark.parametrize("name", ["mfcc13", "mfcc_e_htk", "mfcc_htk"])
def test_silence_through_mfcc(torch, pkg, name):
    print("%s: %.3f of the bound on the device" % (name, kr.check_silence_mfcc(lambda cfg, x: device_values(torch, pkg, cfg, x), name)))


def test_constant_row(torch, pkg, sim):
    """What the folded mean removal leaves of a constant 0.5 on the device: within the ceilings, and the host build's bits"""
    def run(cfg, x):
        got = device_values(torch, pkg, cfg, x)
        assert kr.same_bits(got, kr.host_values(sim, cfg, x))
        return got
    left = kr.check_constant(run, lambda cfg: kr.sim_plan(sim, cfg))
    print("constant 0.5 on the device: largest mel value %s" % ", ".join("%.3g at scale %g" % (v, s) for s, v in left.items()))


def test_small_inputs_and_no_work(torch, pkg):
    """Calls without work, which touch nothing, and what the entry refuses before a launch; a plan that does not fit LDS"""
    with pytest.raises(ValueError):
        pkg.NewKaldiFeatures(**kr.NO_LDS.kwargs())
    for cfg in (kr.W10, kr.W10.with_(layout="bins")):
        T = 30
        F, cols = kr.out_frames(cfg, T), cfg.cols  # 6 frames of 23
        lines, length = kr.out_shape(cfg, F)
        span = (lines - 1) * length + length
        with pkg.NewKaldiFeatures(**cfg.kwargs()) as kf:
            buf = torch.full((1024,), 7.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            B = buf.data_ptr()
            O = B + 2048
            kf.features_device(B, T, 0, T, O, span, length)            # no rows
            kf.features_device(B, T, 2, cfg.W - 1, O, span, length)    # rows shorter than a frame
            kf.features_device(None, 0, 0, 0, None, 0, 0)
            kf.synchronize()
            assert bool((buf == 7.0).all().item())
            for bad in [(None, T, 2, T, O, span, length), (B, T, 2, T, None, span, length), (B + 2, T, 2, T, O, span, length),
                        (B + 1, T, 2, T, O, span, length), (B, T, 2, T, O + 1, span, length), (B, T, 2, T, O + 2, span, length),
                        (B, T - 1, 2, T, O, span, length), (B, T, 2, T, O, span, length - 1), (B, T, 2, T, O, span - 1, length),
                        (B, 1 << 62, 2, T, O, span, length), (B, T, 2, T, O, 1 << 62, length), (B, T, 2, T, O, 1 << 62, 1 << 62)]:
                with pytest.raises(ValueError):
                    kf.features_device(*bad)
            kf.synchronize()
            assert bool((buf == 7.0).all().item())
            with pytest.raises(ValueError):
                kf.last_ms()  # nothing was launched
            kf.features_device(B, T, 2, T, O, span, length)  # and the same arguments, in order, are a pass
            assert kf.last_ms() > 0 and not bool((buf[512:512 + 2 * span] == 7.0).any().item()) and bool((buf[:512] == 7.0).all().item())


FL = 256


@pytest.fixture(scope="module")
def files(oracle, synth, tmp_path_factory):
    """Two small 16-bit stereo files, at 44 100 and at 16 000 Hz -> paths"""
    d = tmp_path_factory.mktemp("fbank")
    made = []
    for name, rate, seed in (("a44", 44100, 1), ("b16", 16000, 2)):
        cfg = oracle.make_config(FL, 16, 2, sample_rate=rate)
        path = d / (name + ".m4a")
        path.write_bytes(m4a.write_m4a(cfg, cr.file_packets(oracle, synth, cfg, 12, seed)))
        made.append(str(path))
    return made


def test_fbank_of_loaded_clips(torch, pkg, files):
    """kaldi_fbank(load_clips(..., sample_rate=16000)[0], 16000, ...) is the pass over the same tensor through the raw-pointer
    entry, there into a buffer with a frame stride of cols + 2 whose padding stays untouched."""
    L = 1200
    clips, lengths, rate = pkg.load_clips(files, [100, 7], L, sample_rate=16000)
    assert rate == 16000 and tuple(clips.shape) == (2, 2, L) and bool(clips.any().item())
    got = pkg.kaldi_fbank(clips, 16000, num_mel_bins=40, use_energy=True)
    F, cols = 1 + (L - 400) // 160, 41
    assert tuple(got.shape) == (2, 2, F, cols)
    out = torch.full((4, F, cols + 2), -7.0, dtype=torch.float32, device="cuda:0")
    flat = clips.contiguous().reshape(4, L)
    torch.cuda.synchronize()
    with pkg.NewKaldiFeatures(16000, 400, 160, num_mel_bins=40, use_energy=True) as kf:
        kf.features_device(flat.data_ptr(), L, 4, L, out.data_ptr(), F * (cols + 2), cols + 2, sync=True)
    assert torch.equal(out[:, :, :cols].view(torch.int32), got.reshape(4, F, cols).view(torch.int32))
    assert bool((out[:, :, cols:] == -7.0).all()) and len(torch.unique(got)) > got.numel() // 2
