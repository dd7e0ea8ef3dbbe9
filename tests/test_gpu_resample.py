"""alacgpu_resample_device on the GPU: bit for bit what the host build of the same header (tests/host_sim/resample_sim.cpp)
writes, over whole sentinel-filled buffers, and within the float32 dot-product bound of the numpy float64 restatement
(tests/resample_ref.py) run on the table the handle reports as its own; and the Python entries over it: resample(),
load(sample_rate=) and load_clips(sample_rate=) on files of different rates. The same over other filter widths, rolloffs, upsampling
pairs and every tile_out (rr.CASES) within the running-error bound of the chain; impulses, which come out as single table entries;
denormals, huge values, -0.0, infinities and NaNs; and host/resampler.hpp through tests/host_sim/host_shim.cpp.

No test provokes a fault: the arguments the entry refuses are refused on the host, before a launch."""
import ctypes

import numpy as np
import pytest

from tests import clip_ref as cr
from tests import m4a
from tests import resample_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture(scope="module")
def sim():
    return rr.build_resample_sim()


def host_image(S, orig, new, x, in_off, out_off, W=6, rolloff=0.99):
    """The host build's whole output buffer for the layout of rr.layout (uint32), as tests/test_resample_host.py runs it."""
    rows, T = x.shape
    frames = rr.out_frames(orig, new, T)
    in_stride, in_lead, in_elems, out_stride, out_lead, out_elems = rr.layout(rows, T, frames, in_off, out_off)
    own_in, own_out = np.zeros(in_elems + 8, np.uint32), np.zeros(out_elems + 8, np.uint32)
    src = own_in[(-own_in.ctypes.data // 4) % 4:][:in_elems]
    img = own_out[(-own_out.ctypes.data // 4) % 4:][:out_elems]
    assert src.ctypes.data % 16 == 0 and img.ctypes.data % 16 == 0
    img[:] = rr.SENTINEL
    for r in range(rows):
        src[in_lead + r * in_stride: in_lead + r * in_stride + T] = x[r].view(np.uint32)
    assert S.resample_sim_run(orig, new, W, rolloff, src.ctypes.data + 4 * in_lead, in_stride, rows, T, img.ctypes.data + 4 * out_lead,
                              out_stride, 0) == 0
    return img.copy()


def device_image(torch, rs, orig, new, x, in_off, out_off):
    rows, T = x.shape
    frames = rr.out_frames(orig, new, T)
    in_stride, in_lead, in_elems, out_stride, out_lead, out_elems = rr.layout(rows, T, frames, in_off, out_off)
    dev = torch.device("cuda:0")
    host = np.full(in_elems, np.nan, np.float32)  # NaN between the rows: a read outside a row's [0, T) shows
    for r in range(rows):
        host[in_lead + r * in_stride: in_lead + r * in_stride + T] = x[r]
    src = torch.from_numpy(host).to(dev)
    buf = torch.full((out_elems,), rr.SENTINEL - (1 << 32), dtype=torch.int32, device=dev)
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    rs.resample_device(src.data_ptr() + 4 * in_lead, in_stride, rows, T, buf.data_ptr() + 4 * out_lead, out_stride, sync=True)
    return buf.cpu().numpy().view(np.uint32), out_lead, out_stride, frames


@pytest.mark.parametrize("orig,new", [(2, 3), (7, 5), (44100, 16000), (48000, 44100), (192000, 8000)])
def test_device_equals_the_host_build_bit_for_bit(torch, pkg, sim, orig, new):
    rng = np.random.default_rng(orig + 3 * new)
    with pkg.NewResampler(orig, new) as rs:
        plan = rs.plan()
        info, h32, first = rr.sim_plan(sim, orig, new)
        assert {k: plan[k] for k in info} == info
        assert np.array_equal(plan["h"].view(np.uint32), h32.view(np.uint32)) and np.array_equal(plan["first"], first)
        with pytest.raises(ValueError):
            rs.last_ms()  # no pass yet on this handle
        Ts = [T for T in rr.boundary_frames(info, orig, new) if T > info["width"]]  # the two at a tile boundary, and 3 001
        assert len(Ts) == 3
        for rows in (1, 5):
            for T in Ts:
                assert rs.out_frames(T) == rr.out_frames(orig, new, T)
                x = rr.signal(rng, rows, T)
                ref = rr.resample64(x, orig, new, h=plan["h"], first=plan["first"])
                lim = rr.bound(plan["h"], plan["first"], x, orig, new)
                run = rr.running_bound(plan["h"], plan["first"], x, orig, new)
                for in_off in range(4):
                    for out_off in range(4):
                        img, lead, stride, frames = device_image(torch, rs, orig, new, x, in_off, out_off)
                        want = host_image(sim, orig, new, x, in_off, out_off)
                        if not np.array_equal(img, want):
                            bad = np.nonzero(img != want)[0]
                            raise AssertionError("rows %d T %d offsets %d/%d: element %d of the buffer (rows start at %d, stride "
                                                 "%d): got %#x, the host build %#x (%d differ)"
                                                 % (rows, T, in_off, out_off, bad[0], lead, stride, img[bad[0]], want[bad[0]], len(bad)))
                        got = np.stack([img[lead + r * stride: lead + r * stride + frames] for r in range(rows)]).view(np.float32)
                        assert (np.abs(got.astype(np.float64) - ref) <= lim).all()
                        assert (np.abs(got.astype(np.float64) - ref) <= run).all(), "above the running bound"
        assert rs.last_ms() > 0


def assert_same_image(img, want, what, lead, stride):
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError("%s: element %d of the buffer (rows start at %d, stride %d): got %#x, want %#x (%d differ)"
                             % (what, bad[0], lead, stride, img[bad[0]], want[bad[0]], len(bad)))


@pytest.mark.parametrize("orig,new,W,rolloff", rr.CASES)
def test_device_equals_the_host_build_for_other_parameters(torch, pkg, sim, orig, new, W, rolloff):
    """rr.CASES: upsampling pairs, other lowpass_filter_width and rolloff values, tile_out 1 024, 512, 256, 128 and 64, the
    table of 22 051 phases, 2 to 1 551 taps; lengths above the filter's width, a row of values over nine decades, the four
    offset pairs of rr.OFFSETS. The whole buffer equals the host build's, the rows lie within the running bound."""
    rng = np.random.default_rng(orig + 3 * new + W)
    paths = set()
    with pkg.NewResampler(orig, new, 0, W, rolloff) as rs:
        plan = rs.plan()
        info, h32, first = rr.sim_plan(sim, orig, new, W, rolloff)
        assert {k: plan[k] for k in info} == info and info["tile_out"] == rr.TILE_OUT.get((orig, new, W, rolloff), 1024)
        assert np.array_equal(plan["h"].view(np.uint32), h32.view(np.uint32)) and np.array_equal(plan["first"], first)
        for rows in (1, 5):
            for T in [T for T in rr.sweep_frames(info, orig, new) if T > info["width"]]:
                assert rs.out_frames(T) == rr.out_frames(orig, new, T)
                x = rr.signal(rng, rows, T)
                if rows > 1:
                    x[1] = (rng.standard_normal(T) * np.exp(rng.uniform(-20.0, 0.0, T))).astype(np.float32)
                ref = rr.resample64(x, orig, new, W, rolloff, h=plan["h"], first=plan["first"])
                run = rr.running_bound(plan["h"], plan["first"], x, orig, new, W, rolloff)
                for out_off, in_off in rr.OFFSETS:
                    img, lead, stride, frames = device_image(torch, rs, orig, new, x, in_off, out_off)
                    assert_same_image(img, host_image(sim, orig, new, x, in_off, out_off, W, rolloff),
                                      "rows %d T %d offsets %d/%d" % (rows, T, in_off, out_off), lead, stride)
                    got = np.stack([img[lead + r * stride: lead + r * stride + frames] for r in range(rows)]).view(np.float32)
                    err = np.abs(got.astype(np.float64) - ref)
                    assert (err <= run).all(), "rows %d T %d: error %g above the running bound %g" % (
                        rows, T, err.flat[np.argmax(err - run)], run.flat[np.argmax(err - run)])
                    paths |= rr.chain_paths(info["tile_out"], rows, frames, out_off)
    print("%d -> %d W %d rolloff %g: tile_out %d, chains per work item %s" % (orig, new, W, rolloff, info["tile_out"], sorted(paths)))


@pytest.mark.parametrize("orig,new,W,rolloff", [(44100, 16000, 6, 0.99), (2, 3, 6, 0.99), (192000, 8000, 6, 0.99), (16000, 44100, 6, 0.99),
                                                (44100, 16000, 64, 0.9475), (3, 1, 6, 1.0)])
def test_device_impulses_come_out_as_single_table_entries(torch, pkg, orig, new, W, rolloff):
    """tests/test_resample_host.py's impulse test on the device: 1.0 (and -0.5) every 2 * width + o + 1 frames, +0.0 elsewhere,
    over three tiles; every output is one entry of the handle's table (times -0.5) or +0.0 at the place the definition gives
    it, the whole buffer compared as uint32."""
    with pkg.NewResampler(orig, new, 0, W, rolloff) as rs:
        plan = rs.plan()
        info = {k: plan[k] for k in ("o", "n", "width", "taps", "tile_out")}
        for amp in (1.0, -0.5):
            x, offsets = rr.impulse_rows(info, orig, new, W, rolloff, amp)
            want = rr.impulse_expected(plan["h"], plan["first"], offsets, x.shape[1], orig, new, W, rolloff, amp)
            assert want.shape[1] >= 3 * info["tile_out"] and np.count_nonzero(want) > 0
            for out_off, in_off in ((0, 0), (3, 1)):
                img, lead, stride, frames = device_image(torch, rs, orig, new, x, in_off, out_off)
                assert_same_image(img, rr.expected_image(want, img.size, lead, stride), "amplitude %g offsets %d/%d" % (amp, in_off, out_off),
                                  lead, stride)


def test_other_float_values(torch, pkg, sim):
    """Denormals, values up to FLT_MAX / 4, -0.0, an infinity and a NaN (rr.special_rows), down and up: the device equals the
    host build bit for bit — denormal table-times-input products and sums are kept, not flushed — except that where the host
    build has a NaN the device has one too, whatever its payload."""
    for orig, new in ((44100, 16000), (2, 3)):
        with pkg.NewResampler(orig, new) as rs:
            x = rr.special_rows(np.random.default_rng(orig), 3001)
            for out_off, in_off in ((0, 0), (1, 3)):
                img, lead, stride, frames = device_image(torch, rs, orig, new, x, in_off, out_off)
                want = host_image(sim, orig, new, x, in_off, out_off)
                rows = np.stack([want[lead + r * stride: lead + r * stride + frames] for r in range(len(x))]).view(np.float32)
                sub = np.abs(rows[0][rows[0] != 0]) < np.float32(2.0 ** -126)
                assert sub.sum() > 100, "the denormal row has no denormal outputs on the host"
                assert np.isfinite(rows[:3]).all() and np.abs(rows[1]).max() > 1e37
                nan = np.isnan(want.view(np.float32))
                assert 0 < nan.sum() < 200 and np.isinf(rows[3]).any()
                assert np.isnan(img.view(np.float32)[nan]).all(), "a NaN of the host build is none on the device"
                assert_same_image(np.where(nan, 0, img), np.where(nan, 0, want), "%d -> %d offsets %d/%d" % (orig, new, in_off, out_off),
                                  lead, stride)


def test_cpp_resampler(torch, pkg, sim):
    """host/resampler.hpp (alac::Resampler: OutFrames, Plan, ResampleDevice, LastMs) through the ctypes shim: the bits and the
    plan of the Python handle, and std::invalid_argument for equal rates."""
    from tests import test_container as tc
    L = tc._build_shim(True, pkg)
    L.shim_resample.restype = ctypes.c_long
    vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    L.shim_resample.argtypes = [u32, u32, u32, ctypes.c_double, vp, sz, sz, sz, vp, sz, vp, vp, vp, sz, vp, sz, vp]
    L.shim_last_error.restype = ctypes.c_char_p
    orig, new, W, rolloff, rows, T = 48000, 44100, 8, 0.95, 3, 2500
    x = torch.from_numpy(rr.signal(np.random.default_rng(8), rows, T)).to("cuda:0")
    with pkg.NewResampler(orig, new, 0, W, rolloff) as rs:
        plan = rs.plan()
        want = rs(x)
    frames = want.shape[1]
    out = torch.full((rows, frames + 1), -7.0, dtype=torch.float32, device="cuda:0")
    of, ms = ctypes.c_uint64(0), ctypes.c_float(-1.0)
    info = np.zeros(5, np.uint32)
    h, first = np.zeros_like(plan["h"]), np.zeros_like(plan["first"])
    torch.cuda.synchronize()
    rc = L.shim_resample(orig, new, W, rolloff, x.data_ptr(), T, rows, T, out.data_ptr(), frames + 1, ctypes.byref(of), info.ctypes.data,
                         h.ctypes.data, h.size, first.ctypes.data, first.size, ctypes.byref(ms))
    assert rc == 0, L.shim_last_error()
    assert of.value == frames == rr.out_frames(orig, new, T) and ms.value > 0
    assert [int(v) for v in info] == [plan[k] for k in ("o", "n", "width", "taps", "tile_out")]
    assert np.array_equal(h.view(np.uint32), plan["h"].view(np.uint32)) and np.array_equal(first, plan["first"])
    assert torch.equal(out[:, :frames].view(torch.int32), want.view(torch.int32)) and bool((out[:, frames] == -7.0).all())
    rc = L.shim_resample(orig, orig, W, rolloff, x.data_ptr(), T, rows, T, out.data_ptr(), frames + 1, ctypes.byref(of), info.ctypes.data,
                         h.ctypes.data, h.size, first.ctypes.data, first.size, ctypes.byref(ms))
    assert rc == -6 and b"no resampling plan" in L.shim_last_error()
    assert bool((out[:, frames] == -7.0).all()) and torch.equal(out[:, :frames].view(torch.int32), want.view(torch.int32))


def test_small_inputs_and_no_work(torch, pkg, sim):
    """Rows shorter than the filter is wide, and calls without work, which touch nothing."""
    orig, new = 44100, 16000
    rng = np.random.default_rng(5)
    with pkg.NewResampler(orig, new) as rs:
        for T in (1, 2, 16, 17):
            x = rr.signal(rng, 3, T)
            img, _, _, _ = device_image(torch, rs, orig, new, x, 1, 3)
            assert np.array_equal(img, host_image(sim, orig, new, x, 1, 3))
        buf = torch.full((64,), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        rs.resample_device(buf.data_ptr(), 8, 0, 8, buf.data_ptr(), 8)
        rs.resample_device(buf.data_ptr(), 8, 2, 0, buf.data_ptr(), 8)
        rs.resample_device(None, 0, 0, 0, None, 0)
        rs.synchronize()
        assert bool((buf == 7.0).all().item())
        for bad in [(None, 8, 2, 8, buf.data_ptr(), 8), (buf.data_ptr(), 8, 2, 8, None, 8), (buf.data_ptr() + 2, 8, 2, 8, buf.data_ptr() + 128, 8),
                    (buf.data_ptr(), 7, 2, 8, buf.data_ptr() + 128, 8), (buf.data_ptr(), 8, 2, 8, buf.data_ptr() + 128, 2),
                    (buf.data_ptr(), 1 << 62, 2, 8, buf.data_ptr() + 128, 8)]:
            with pytest.raises(ValueError):
                rs.resample_device(*bad)
        assert bool((buf == 7.0).all().item())


def test_resample_function(torch, pkg):
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.uniform(-1, 1, (3, 2, 1000)).astype(np.float32)).to("cuda:0")
    y = pkg.resample(x, 44100, 16000)
    frames = rr.out_frames(44100, 16000, 1000)
    assert tuple(y.shape) == (3, 2, frames) and y.is_cuda and y.dtype is torch.float32
    for a in range(3):
        for c in range(2):
            assert torch.equal(pkg.resample(x[a, c], 44100, 16000), y[a, c])
    with pkg.NewResampler(44100, 16000) as rs:
        plan = rs.plan()
    rows = x.cpu().numpy().reshape(6, 1000)
    ref = rr.resample64(rows, 44100, 16000, h=plan["h"], first=plan["first"])
    assert (np.abs(y.cpu().numpy().reshape(6, frames) - ref) <= rr.bound(plan["h"], plan["first"], rows, 44100, 16000)).all()
    assert pkg.resample(x, 44100, 44100) is x  # equal rates: the input
    # a non-contiguous input, a CPU tensor and a numpy array
    t = x.transpose(0, 1)
    assert not t.is_contiguous() and torch.equal(pkg.resample(t, 44100, 16000), y.transpose(0, 1))
    half = x[..., ::2]
    assert torch.equal(pkg.resample(half, 48000, 44100), pkg.resample(half.contiguous(), 48000, 44100))
    assert torch.equal(pkg.resample(x.cpu(), 44100, 16000), y) and torch.equal(pkg.resample(x.cpu().numpy(), 44100, 16000), y)
    assert tuple(pkg.resample(x[..., :0], 44100, 16000).shape) == (3, 2, 0)
    for bad in (x.double(), x.to(torch.int32), x.cpu().numpy().astype(np.float64)):
        with pytest.raises(ValueError):
            pkg.resample(bad, 44100, 16000)
    with pytest.raises(ValueError):
        pkg.resample(x, 44100, 0)


# ---- files of different rates -----------------------------------------------------------------------------------------
FL = 256


@pytest.fixture(scope="module")
def files(oracle, synth, tmp_path_factory):
    """Two 16-bit stereo files of 20 full packets of 256 frames and a short one, at 44 100 and at 48 000 Hz, and one with
    another channel count -> {name: path}."""
    d = tmp_path_factory.mktemp("rates")
    made = {}
    for name, rate, ch, seed in (("a44", 44100, 2, 1), ("b48", 48000, 2, 2), ("mono48", 48000, 1, 3)):
        cfg = oracle.make_config(FL, 16, ch, sample_rate=rate)
        path = d / (name + ".m4a")
        path.write_bytes(m4a.write_m4a(cfg, cr.file_packets(oracle, synth, cfg, 20, seed)))
        made[name] = str(path)
    return made


def test_load_clips_over_mixed_rates(torch, pkg, files):
    a, b = files["a44"], files["b48"]
    total = {k: pkg.load(files[k])[0].shape[1] for k in ("a44", "b48")}
    assert total["a44"] == total["b48"] == 20 * FL + FL // 3 + 1
    R, L = 16000, 500
    srcs = [a, b, b, a, b, a]
    offs = [0, 7, 3 * FL + 1, 3000, total["b48"] - 300, total["a44"] + 5]  # the last two: over a file's end, and past it
    clips, lengths, rate = pkg.load_clips(srcs, offs, L, sample_rate=R)
    assert rate == R and tuple(clips.shape) == (6, 2, L) and clips.dtype is torch.float32 and clips.is_cuda
    assert lengths.dtype is torch.int32 and lengths.is_cuda
    for j, (src, off) in enumerate(zip(srcs, offs)):
        r = 44100 if src == a else 48000
        Ls = -(-L * r // R)
        alone, valid, own = pkg.load_clips([src], [off], Ls)
        assert own == r and tuple(alone.shape) == (1, 2, Ls)
        want = pkg.resample(alone, r, R)[:, :, :L]
        assert tuple(want.shape) == (1, 2, L)
        assert torch.equal(clips[j].view(torch.int32), want[0].view(torch.int32)), "clip %d" % j
        v = int(valid[0].item())
        assert int(lengths[j].item()) == min(L, -(-v * R // r)), "clip %d" % j
    assert [int(x) for x in lengths.cpu()[:4]] == [L] * 4 and int(lengths[4].item()) == -(-300 * R // 48000) and int(lengths[5].item()) == 0
    assert not clips[5].any().item()
    # a rate one of the groups already has: that group is gathered, not resampled
    clips48, lengths48, rate = pkg.load_clips([a, b], [10, 10], L, sample_rate=48000)
    assert rate == 48000 and torch.equal(clips48[1], pkg.load_clips([b], [10], L)[0][0]) and int(lengths48[1].item()) == L
    Ls = -(-L * 44100 // 48000)
    assert torch.equal(clips48[0], pkg.resample(pkg.load_clips([a], [10], Ls)[0], 44100, 48000)[0, :, :L])
    # without sample_rate nothing changes: differing rates are a configuration error
    with pytest.raises(pkg.ErrConfig, match="source 1: SampleRate 48000"):
        pkg.load_clips(srcs, offs, L)
    # and with it every other difference still is
    with pytest.raises(pkg.ErrConfig, match="source 2: NumChannels 1"):
        pkg.load_clips([a, b, files["mono48"]], [0, 0, 0], L, sample_rate=R)
    with pytest.raises(ValueError):
        pkg.load_clips([a, b], [0, 0], L, sample_rate=R, dtype=torch.int32)


def test_load_at_another_rate(torch, pkg, files):
    path = files["a44"]
    full, rate = pkg.load(path)
    assert rate == 44100
    got, sr = pkg.load(path, sample_rate=16000)
    assert sr == 16000 and tuple(got.shape) == (2, rr.out_frames(44100, 16000, full.shape[1]))
    assert torch.equal(got, pkg.resample(full, 44100, 16000))
    # frame_offset / num_frames stay in the file's own frames
    got, sr = pkg.load(path, frame_offset=FL + 3, num_frames=1000, sample_rate=16000)
    assert sr == 16000 and torch.equal(got, pkg.resample(full[:, FL + 3:FL + 1003], 44100, 16000))
    same, sr = pkg.load(path, sample_rate=44100)  # the file's own rate: the existing path
    assert sr == 44100 and torch.equal(same, full)
    with pytest.raises(ValueError):
        pkg.load(path, sample_rate=16000, dtype=torch.int32)
