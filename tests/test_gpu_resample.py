"""alacgpu_resample_device on the GPU: bit for bit what the host build of the same header (tests/host_sim/resample_sim.cpp)
writes, over whole sentinel-filled buffers, and within the float32 dot-product bound of the numpy float64 restatement
(tests/resample_ref.py) run on the table the handle reports as its own; and the Python entries over it: resample(),
load(sample_rate=) and load_clips(sample_rate=) on files of different rates.

No test provokes a fault: the arguments the entry refuses are refused on the host, before a launch."""
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


def host_image(S, orig, new, x, in_off, out_off):
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
    assert S.resample_sim_run(orig, new, 6, 0.99, src.ctypes.data + 4 * in_lead, in_stride, rows, T, img.ctypes.data + 4 * out_lead,
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
        assert rs.last_ms() > 0


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
