"""The pack pass, encode_waveform and save() on the GPU: planar float32 / int32 waveforms -> the encoder's PCM -> packets ->
an M4A file, against the numpy restatement of tests/wavepack_ref.py, the encoder's own entry on the restatement's PCM, and
the package's decoders.

Every pass writes into a buffer filled with a sentinel, reads a waveform embedded in a buffer of NaN sentinels with slack in
both strides, and the WHOLE PCM buffer is compared: the bytes, and every byte outside the footprint still the sentinel; an
element read from outside the waveform would show in the clipped count. No test provokes a fault."""
import io

import numpy as np
import pytest

from tests import wave_ref as wr
from tests import wavepack_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


def cfg_of(pkg, fl, depth, ch, rate=44100):
    return pkg.PacketConfig(FrameLength=fl, BitDepth=depth, NumChannels=ch, SampleRate=rate)


def device_pass(torch, enc, fl, depth, ch, x, layout, wtype, wave_mis=0, slack=0, pcm_mis=0, want_clipped=True):
    """x [ch, total] in a sentinel-filled device buffer, the tensor at an address that is wave_mis modulo 16; the pass into a
    sentinel-filled PCM buffer, the stream at an address that is pcm_mis modulo 16 -> (image uint8, base, clipped or None)."""
    dev = torch.device("cuda:0")
    total = x.shape[1]
    lead = 8 + wave_mis // 4
    cs, ps, elems = pr.geometry(layout, fl, ch, total, slack, lead)
    src = pr.lay_out(x, layout, fl, lead, cs, ps, elems)
    d_src = torch.from_numpy(src.view(np.int32)).to(dev)
    base = 16 + pcm_mis
    d_pcm = torch.full((base + total * ch * wr.BPS[depth] + 40,), pr.PCM_SENTINEL, dtype=torch.uint8, device=dev)
    assert d_src.data_ptr() % 16 == 0 and d_pcm.data_ptr() % 16 == 0
    d_clip = torch.full((1,), 0xDEAD, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    enc.pcm_from_waveform_device(d_src.data_ptr() + 4 * lead, layout, wtype, cs, ps, total, d_pcm.data_ptr() + base,
                                 d_clip.data_ptr() if want_clipped else None, sync=True)
    assert np.array_equal(d_src.cpu().numpy().view(np.uint32), src), "the pass wrote to its input"
    return d_pcm.cpu().numpy(), base, int(d_clip.item()) if want_clipped else None


def check(torch, enc, fl, depth, ch, x, layout, wtype, **kw):
    img, base, clipped = device_pass(torch, enc, fl, depth, ch, x, layout, wtype, **kw)
    ref, ref_clipped = pr.pack_ref(x, depth, wtype)
    want = pr.expected_image(ref, img.size, base)
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError("byte %d of the buffer (stream byte %d): got %#x, want %#x (%d differ)" %
                             (bad[0], bad[0] - base, img[bad[0]], want[bad[0]], len(bad)))
    if clipped is not None:
        assert clipped == ref_clipped


@pytest.mark.parametrize("fl", [4096, 4095, 1])
@pytest.mark.parametrize("ch", [1, 2, 3, 6, 8])
@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_pass_equals_numpy_over_the_matrix(torch, pkg, depth, ch, fl):
    rng = np.random.default_rng(depth * 1000 + ch * 10 + fl)
    total = 3 * fl + 1237 % fl if fl > 1 else 301
    with pkg.NewPacketEncoder(cfg_of(pkg, fl, depth, ch)) as enc:
        for wtype in (pr.FLOAT, pr.INT):
            x = pr.random_wave(rng, ch, total, depth, wtype)
            for layout in (pr.STREAM, pr.PACKETS):
                check(torch, enc, fl, depth, ch, x, layout, wtype, want_clipped=(layout == pr.STREAM) == (wtype == pr.FLOAT))
                check(torch, enc, fl, depth, ch, x, layout, wtype, wave_mis=4, slack=1, pcm_mis=1,
                      want_clipped=(layout == pr.STREAM) != (wtype == pr.FLOAT))


@pytest.mark.parametrize("depth,ch", [(16, 2), (24, 2), (20, 3), (32, 8), (16, 1), (24, 7)])
def test_total_frames_around_the_tile_size(torch, pkg, depth, ch):
    rng = np.random.default_rng(depth + ch)
    tile = (8192 // (ch * wr.BPS[depth])) & ~63  # 8 KB worth of frames, a multiple of 64
    for total in (tile - 1, tile, tile + 1, 2 * tile - 1):
        x = pr.random_wave(rng, ch, total, depth, pr.FLOAT)
        with pkg.NewPacketEncoder(cfg_of(pkg, 4096, depth, ch)) as enc:
            check(torch, enc, 4096, depth, ch, x, pr.STREAM, pr.FLOAT, wave_mis=4, slack=1, pcm_mis=3)
        y = pr.random_wave(rng, ch, 2 * total + 5, depth, pr.INT)
        with pkg.NewPacketEncoder(cfg_of(pkg, total, depth, ch)) as enc:
            check(torch, enc, total, depth, ch, y, pr.PACKETS, pr.INT, wave_mis=8, slack=3, pcm_mis=9)


@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 333), (24, 2, 4096), (20, 3, 70), (32, 8, 300), (16, 1, 4095), (24, 6, 513)])
def test_every_alignment_gives_the_same_bytes(torch, pkg, depth, ch, fl):
    rng = np.random.default_rng(depth + ch + fl)
    total = 2 * fl + fl // 3 + 1
    xs = {t: pr.random_wave(rng, ch, total, depth, t) for t in (pr.FLOAT, pr.INT)}
    with pkg.NewPacketEncoder(cfg_of(pkg, fl, depth, ch)) as enc:
        for wave_mis, slack in ((0, 0), (4, 1), (8, 2), (12, 3), (0, 3), (12, 0)):
            for pcm_mis in (0, 1, 2, 4, 7, 8, 13, 15):
                for layout in (pr.STREAM, pr.PACKETS):
                    wtype = pr.FLOAT if (layout == pr.STREAM) == (pcm_mis % 2 == 0) else pr.INT
                    check(torch, enc, fl, depth, ch, xs[wtype], layout, wtype, wave_mis=wave_mis, slack=slack, pcm_mis=pcm_mis)


def test_argument_errors_and_no_frames(torch, pkg):
    dev = torch.device("cuda:0")
    w = torch.zeros(4096, dtype=torch.float32, device=dev)
    o = torch.full((64,), pr.PCM_SENTINEL, dtype=torch.uint8, device=dev)
    off = torch.full((4,), -1, dtype=torch.int64, device=dev)
    clip = torch.full((1,), 7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pkg.NewPacketEncoder(cfg_of(pkg, 100, 16, 2)) as enc:
        p, q = w.data_ptr(), o.data_ptr()
        for args in ((None, 0, 0, 1000, 0, 10, q), (p, 0, 0, 1000, 0, 10, None), (p, 2, 0, 1000, 0, 10, q), (p, 0, 2, 1000, 0, 10, q),
                     (p + 2, 0, 0, 1000, 0, 10, q), (p, 0, 0, 9, 0, 10, q), (p, 1, 0, 99, 200, 10, q), (p, 1, 0, 100, 199, 10, q)):
            with pytest.raises(ValueError):
                enc.pcm_from_waveform_device(*args)
        with pytest.raises(ValueError):  # blob_cap below max_bytes
            enc.encode_waveform_device(p, 0, 0, 1000, 0, 10, q, enc.max_bytes(10) - 1, off.data_ptr())
        with pytest.raises(ValueError):
            enc.encode_waveform_device(p, 0, 0, 1000, 0, 10, q, 64, None)
        with pytest.raises(ValueError):
            enc.waveform_last_ms()  # no pass yet
        enc.pcm_from_waveform_device(p, 0, 0, 0, 0, 0, q, clip.data_ptr())
        assert int(clip.item()) == 0
        clip.fill_(7)
        torch.cuda.synchronize()
        enc.encode_waveform_device(p, 1, 0, 100, 200, 0, q, 64, off.data_ptr(), clip.data_ptr())
        assert int(clip.item()) == 0 and int(off[0].item()) == 0
        assert bytes(o.cpu().numpy()) == bytes([pr.PCM_SENTINEL]) * 64


# ---- encode_waveform_device ---------------------------------------------------------------------------------------------
def music(rng, ch, total, depth):
    """In-range samples that compress: slow sines plus a little noise, as integers of the depth -> int64 [ch, total]"""
    top = 1 << (depth - 1)
    t = np.arange(total)[None, :]
    v = (0.4 * top * np.sin(t / 23.0 + np.arange(ch)[:, None])).astype(np.int64) + rng.integers(-40, 41, (ch, total))
    v[:, :4] = [[-top, top - 1, 0, -1]]
    return np.clip(v, -top, top - 1)


def wave_of(v, depth, wtype):
    """The waveform that the decoder makes of the samples v (integers of the depth): what round-trips bit for bit."""
    if wtype == pr.INT:
        return (v << 4 if depth == 20 else v).astype(np.int32)
    return v.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -(depth - 1))


def encode_ready_pcm(torch, enc, pcm, total):
    dev = torch.device("cuda:0")
    d_pcm = torch.from_numpy(pcm).to(dev)
    cap = enc.max_bytes(total)
    n = -(-total // enc.config.FrameLength)
    d_blob = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    enc.encode_device(d_pcm.data_ptr(), total, d_blob.data_ptr(), cap, d_off.data_ptr(), sync=True)
    off = d_off.cpu().numpy()
    return d_blob[:int(off[-1])].cpu().numpy(), off


@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 4096), (24, 2, 1000), (20, 6, 512), (32, 1, 4096), (32, 8, 300), (24, 3, 4095)])
def test_encode_waveform_is_the_encode_of_the_restatements_pcm(torch, pkg, depth, ch, fl):
    """Blob and offsets byte for byte those of encode_device on the restatement's PCM, for both layouts and types, in-range and
    clipping input; the in-range ones come back through decode_waveform bit for bit."""
    rng = np.random.default_rng(depth + ch + fl)
    total = 5 * fl + fl // 2 + 1
    n = 6
    cfg = cfg_of(pkg, fl, depth, ch)
    with pkg.NewPacketEncoder(cfg) as enc, pkg.NewPacketEncoder(cfg) as plain, pkg.NewPacketDecoder(cfg) as dec:
        for wtype, tdt in ((pr.FLOAT, torch.float32), (pr.INT, torch.int32)):
            v = music(rng, ch, total, depth if depth < 32 or wtype == pr.INT else 31)
            for x, exact in ((wave_of(v, depth, wtype), True), (pr.random_wave(rng, ch, total, depth, wtype, loud=0.05), False)):
                pcm, ref_clipped = pr.pack_ref(x, depth, wtype)
                assert (ref_clipped == 0) == (exact or (wtype == pr.INT and depth == 32))
                ref_blob, ref_off = encode_ready_pcm(torch, plain, pcm, total)
                padded = np.zeros((ch, n * fl), x.dtype)
                padded[:, :total] = x
                clips = np.ascontiguousarray(padded.reshape(ch, n, fl).transpose(1, 0, 2))
                for layout, arg in (("stream", x), ("packets", clips)):
                    blob, off, clipped = enc.encode_waveform(arg, layout, frames=total)
                    assert np.array_equal(off.cpu().numpy(), ref_off) and np.array_equal(blob.cpu().numpy(), ref_blob)
                    assert clipped == ref_clipped
                    if exact:
                        wave, frames, status = dec.decode_waveform(blob, off, None, layout, tdt)
                        assert not status.any().item()
                        got = wave.cpu().numpy()
                        if layout == "packets":
                            got = got.transpose(1, 0, 2).reshape(ch, n * fl)[:, :total]
                        assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


def test_pass_and_encode_behind_an_unsynchronized_encode(torch, pkg):
    """encode_device with sync = 0, then encode_waveform_device with sync = 0 on the same handle: stream order alone."""
    rng = np.random.default_rng(8)
    depth, ch, fl = 24, 2, 2048
    total = 40 * fl + 9
    cfg = cfg_of(pkg, fl, depth, ch)
    dev = torch.device("cuda:0")
    x = wave_of(music(rng, ch, total, depth), depth, pr.FLOAT)
    pcm, _ = pr.pack_ref(x, depth, pr.FLOAT)
    other, _ = pr.pack_ref(wave_of(music(rng, ch, total, depth), depth, pr.FLOAT), depth, pr.FLOAT)
    with pkg.NewPacketEncoder(cfg) as plain:
        ref_blob, ref_off = encode_ready_pcm(torch, plain, pcm, total)
        ref_blob0, ref_off0 = encode_ready_pcm(torch, plain, other, total)
    with pkg.NewPacketEncoder(cfg) as enc:
        cap = enc.max_bytes(total)
        d_other, d_x = torch.from_numpy(other).to(dev), torch.from_numpy(x).to(dev)
        blob0, blob1 = (torch.zeros(cap, dtype=torch.uint8, device=dev) for _ in range(2))
        off0, off1 = (torch.zeros(42, dtype=torch.int64, device=dev) for _ in range(2))
        clip = torch.full((1,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        enc.encode_device(d_other.data_ptr(), total, blob0.data_ptr(), cap, off0.data_ptr(), sync=False)
        enc.encode_waveform_device(d_x.data_ptr(), pr.STREAM, pr.FLOAT, total, 0, total, blob1.data_ptr(), cap, off1.data_ptr(),
                                   clip.data_ptr(), sync=False)
        enc.synchronize()
        assert np.array_equal(off0.cpu().numpy(), ref_off0) and np.array_equal(blob0[:int(ref_off0[-1])].cpu().numpy(), ref_blob0)
        assert np.array_equal(off1.cpu().numpy(), ref_off) and np.array_equal(blob1[:int(ref_off[-1])].cpu().numpy(), ref_blob)
        assert int(clip.item()) == 0


def test_python_entry_takes_numpy_cpu_and_cuda_tensors(torch, pkg):
    rng = np.random.default_rng(4)
    depth, ch, fl = 16, 2, 256
    n, frames = 5, 4 * 256 + 100  # shorter than the tensor
    cfg = cfg_of(pkg, fl, depth, ch)
    with pkg.NewPacketEncoder(cfg) as enc, pkg.NewPacketEncoder(cfg) as plain:
        for wtype in (pr.FLOAT, pr.INT):
            x = pr.random_wave(rng, ch, n * fl, depth, wtype, loud=0.01)
            pcm, ref_clipped = pr.pack_ref(x[:, :frames], depth, wtype)
            ref_blob, ref_off = encode_ready_pcm(torch, plain, pcm, frames)
            clips = np.ascontiguousarray(x.reshape(ch, n, fl).transpose(1, 0, 2))
            wide = np.zeros((ch, n * fl + 7), x.dtype)
            wide[:, 3:3 + n * fl] = x
            for layout, a in (("stream", x), ("packets", clips), ("stream", wide[:, 3:3 + n * fl])):  # the last: rows with a stride
                for arg in (a, torch.from_numpy(a.copy()), torch.from_numpy(a.copy()).cuda(), torch.from_numpy(wide).cuda()[:, 3:3 + n * fl]
                            if layout == "stream" else torch.from_numpy(a.copy()).cuda()):
                    blob, off, clipped = enc.encode_waveform(arg, layout, frames=frames)
                    assert blob.is_cuda and blob.dtype is torch.uint8 and off.is_cuda and off.dtype is torch.int64 and off.numel() == n + 1
                    assert isinstance(clipped, int) and clipped == ref_clipped
                    assert np.array_equal(off.cpu().numpy(), ref_off) and np.array_equal(blob.cpu().numpy(), ref_blob)
            blob, off, _ = enc.encode_waveform(x)  # frames defaults to T
            assert off.numel() == n + 1 and int(off[-1].item()) == blob.numel()
        x = np.zeros((ch, n * fl), np.float32)
        for bad, kw in ((x.astype(np.float64), {}), (x.astype(np.int16), {}), (x[0], {}), (np.zeros((3, 100), np.float32), {}),
                        (x[:, ::2], {}), (torch.from_numpy(x)[:, ::2], {}), (x, {"frames": n * fl + 1}), (x, {"frames": -1}),
                        (x, {"layout": "rows"}), (x, {"layout": "packets"}), (np.zeros((2, ch, fl + 1), np.float32), {"layout": "packets"}),
                        (np.zeros((2, ch + 1, fl), np.float32), {"layout": "packets"}), ([[0.0] * 8] * ch, {})):
            with pytest.raises(ValueError):
                enc.encode_waveform(bad, **kw)


# ---- save ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,ch", [(16, 2), (24, 2), (20, 6), (32, 1)])
def test_save_then_load_is_bit_equal(torch, pkg, tmp_path, depth, ch):
    rng = np.random.default_rng(depth + ch)
    fl = 4096
    total = 6 * fl + 1001  # a short last packet
    for wtype, tdt in ((pr.FLOAT, torch.float32), (pr.INT, torch.int32)):
        x = wave_of(music(rng, ch, total, depth if depth < 32 or wtype == pr.INT else 31), depth, wtype)
        path = str(tmp_path / ("w%d.m4a" % wtype))
        mem = io.BytesIO()
        assert pkg.save(path, torch.from_numpy(x), 48000, bits_per_sample=depth) == 0
        assert pkg.save(mem, torch.from_numpy(x).cuda(), 48000, bits_per_sample=depth) == 0
        assert open(path, "rb").read() == mem.getvalue()
        for source in (path, mem.getvalue()):
            wave, rate = pkg.load(source, dtype=tdt)
            assert rate == 48000 and tuple(wave.shape) == (ch, total)
            assert np.array_equal(wave.cpu().numpy().view(np.uint32), x.view(np.uint32))
        if wtype == pr.FLOAT:  # the streaming decoder reads the restatement's PCM out of the file
            with pkg.NewDecoder(path) as d:
                assert bytes(d.ReadAll()) == pr.pack_ref(x, depth, wtype)[0].tobytes()
            cfg = pkg.ParseMagicCookie(pkg.FindALACTrack(mem.getvalue()).cookie)
            assert (cfg.FrameLength, cfg.BitDepth, cfg.NumChannels, cfg.SampleRate) == (fl, depth, ch, 48000)
            assert cfg.MaxFrameBytes > 0 and cfg.AvgBitRate > 0


def test_several_windows_write_the_file_of_one(torch, pkg):
    """More packets than one 48 MB window holds (8-channel 32-bit frames of 4096: 384 packets a window), against the same
    waveform saved in one window: the same bytes, cookie included."""
    ch, fl = 8, 4096
    total = 429 * fl + 100
    g = torch.Generator(device="cuda").manual_seed(3)
    wave = torch.randint(-30000, 30000, (ch, total), dtype=torch.int32, device="cuda", generator=g) * 4097
    several, one = io.BytesIO(), io.BytesIO()
    assert pkg.save(several, wave, 96000, bits_per_sample=32) == 0
    assert pkg.save(one, wave, 96000, bits_per_sample=32, _window=1 << 20) == 0
    assert several.getvalue() == one.getvalue()
    got, rate = pkg.load(several.getvalue(), dtype=torch.int32)
    assert rate == 96000 and torch.equal(got, wave)


def test_save_counts_and_saturates_what_is_out_of_range(torch, pkg):
    rng = np.random.default_rng(12)
    depth, ch, fl, total = 24, 2, 1024, 5000
    x = pr.random_wave(rng, ch, total, depth, pr.FLOAT, loud=0.05)
    v, ref_clipped = pr.quantize(x, depth, pr.FLOAT)
    assert ref_clipped > 50
    mem = io.BytesIO()
    assert pkg.save(mem, x, 44100, bits_per_sample=depth, frame_length=fl) == ref_clipped
    wave, _ = pkg.load(mem.getvalue(), dtype=torch.int32)
    assert np.array_equal(wave.cpu().numpy(), v.astype(np.int32))
    top = 1 << (depth - 1)
    assert (v == top - 1).sum() > 10 and (v == -top).sum() > 10


def test_mid_size_batch_against_the_torch_composition(torch, pkg):
    """4 096 packets of 16-bit stereo, checked on the device against what a caller writes in torch ops today; the pass is timed
    by its own event pair and leaves the encode's alone."""
    ch, fl, n = 2, 4096, 4096
    total = n * fl
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cuda").manual_seed(5)
    x = (torch.rand((ch, total), dtype=torch.float32, device=dev, generator=g) - 0.5) * 2.02
    x[1, 12345] = float("nan")
    x[0, 999] = float("inf")
    r = torch.round(x * 32768.0)  # half to even, in float32
    want_clipped = int((torch.isnan(r) | (r > 32767) | (r < -32768)).sum().item())
    want = torch.nan_to_num(r, nan=0.0).clamp(-32768, 32767).to(torch.int16).t().contiguous().view(torch.uint8).reshape(-1)
    assert want_clipped > 1000
    with pkg.NewPacketEncoder(cfg_of(pkg, fl, 16, ch)) as enc:
        pcm = torch.full((total * 4 + 32,), pr.PCM_SENTINEL, dtype=torch.uint8, device=dev)
        clip = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        enc.pcm_from_waveform_device(x.data_ptr(), pr.STREAM, pr.FLOAT, total, 0, total, pcm.data_ptr() + 16, clip.data_ptr())
        assert torch.equal(pcm[16:16 + total * 4], want) and int(clip.item()) == want_clipped
        assert bool((pcm[:16] == pr.PCM_SENTINEL).all()) and bool((pcm[16 + total * 4:] == pr.PCM_SENTINEL).all())
        blob, off, clipped = enc.encode_waveform(x)
        assert clipped == want_clipped
        pass_ms, enc_ms = enc.waveform_last_ms(), enc.last_kernel_ms()
        assert pass_ms > 0 and enc_ms > pass_ms  # two serial chains of 4 096 samples a packet against one pass over memory
        enc.pcm_from_waveform_device(x.data_ptr(), pr.STREAM, pr.FLOAT, total, 0, total, pcm.data_ptr() + 16, None)
        assert enc.last_kernel_ms() == enc_ms  # a pass alone does not touch the encode's events
        cap = enc.max_bytes(total)
        blob2 = torch.zeros(cap, dtype=torch.uint8, device=dev)
        off2 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        enc.encode_device(want.data_ptr(), total, blob2.data_ptr(), cap, off2.data_ptr())
        assert torch.equal(off, off2) and torch.equal(blob, blob2[:blob.numel()])
