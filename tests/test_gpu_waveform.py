"""alacgpu_waveform_device on the GPU: planar float32 / int32 waveforms behind an unsynchronized device decode, bit for bit
what the numpy restatement of tests/wave_ref.py makes of the ORACLE's decode of the same packets.

Every pass writes into a buffer filled with a sentinel, with slack in channel_stride / packet_stride and elements in front
of and behind the tensor, and the WHOLE buffer is compared: the values, and every element outside the documented
footprint still the sentinel. No test provokes a fault: damaged packets are data errors the decoder reports as status."""
import importlib

import numpy as np
import pytest

from tests import m4a
from tests import wave_ref as wr

pytestmark = pytest.mark.gpu
SHIFT = {16: 0, 20: 0, 24: 1, 32: 2}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


def to_pkg_cfg(pkg, ocfg):
    return pkg.PacketConfig(FrameLength=ocfg.frame_length, BitDepth=ocfg.bit_depth, NumChannels=ocfg.num_channels,
                            PB=ocfg.pb, MB=ocfg.mb, KB=ocfg.kb, MaxRun=ocfg.max_run, SampleRate=ocfg.sample_rate)


def pcm_extremes(depth):
    """The extremes in the PCM domain of the depth (a 20-bit sample comes out left-aligned in its three bytes)."""
    if depth == 20:
        return np.array([-(1 << 19), (1 << 19) - 1, -1, 0, 1], np.int64)
    return wr.extremes(depth)


def short_packet(synth, cfg, frames, seed, escape):
    ne = synth.num_elements(cfg.num_channels)
    kw = dict(force_escape=1) if escape else dict(never_escape=1, bytes_shifted=SHIFT[cfg.bit_depth])
    pcm = synth.signal(cfg, synth.PROFILE_MUSIC, seed, frames)
    return synth.encode_packet(cfg, [synth.default_elem(**kw) for _ in range(ne)], pcm)


def extreme_packet(synth, cfg):
    """One escaped packet whose samples are the depth's extremes, every channel starting at another one."""
    ex = pcm_extremes(cfg.bit_depth)
    fl, ch = cfg.frame_length, cfg.num_channels
    pcm = np.stack([np.resize(np.roll(ex, c), fl) for c in range(ch)], axis=1).astype(np.int32)
    ne = synth.num_elements(ch)
    return synth.encode_packet(cfg, [synth.default_elem(force_escape=1) for _ in range(ne)], pcm)


def packet_list(synth, helpers, cfg, n, seed, damaged=0):
    """A synth batch with the extremes packet, short packets at the start, in the middle and at the end (odd lengths, so
    that the following start[i] are odd and unaligned), and `damaged` mutated packets mixed in."""
    fl = cfg.frame_length
    b = synth.gen_batch(cfg, n, base_seed=seed, threads=8)
    rng = np.random.default_rng(seed)
    packets = [b.packet(i) for i in range(b.n)] + helpers.mutate_packets(b, rng, damaged)
    rng.shuffle(packets)
    packets.insert(len(packets) // 3, extreme_packet(synth, cfg))
    if fl > 1:
        for at, k, esc in ((0, 1, True), (len(packets) // 2, fl // 2 + 1, False), (len(packets) // 2, 3, True),
                           (len(packets), fl - 1, False), (len(packets), max(fl - 3, 1), True)):
            if 1 <= k < fl:
                packets.insert(at, short_packet(synth, cfg, k, seed + k, esc or fl < 16))
    return packets


class Batch:
    """Packets on the device and the oracle's decode of them."""

    def __init__(self, torch, oracle, helpers, cfg, packets):
        self.cfg, self.n = cfg, len(packets)
        blob, offs, sizes = helpers.pack_packets(packets)
        self.ref = oracle.decode_batch(cfg, blob, offs, sizes, threads=8)
        dev = torch.device("cuda:0")
        self.d_blob = torch.from_numpy(blob).to(dev)
        self.d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
        self.d_sz = torch.from_numpy(sizes.astype(np.int32)).to(dev)


def device_pass(torch, dec, b, layout, wtype, pcm_mis=0, stride=None, wave_mis=0, slack=0, use_status=True, want_starts=True):
    """Decode (sync = 0) and convert (sync = 1) on the handle's stream; the slots at an address that is pcm_mis modulo 16, the
    wave tensor at one that is wave_mis modulo 16 inside a sentinel-filled buffer -> (image uint32, base, cs, ps, starts,
    frames, status)."""
    cfg, n = b.cfg, b.n
    fl, ch = cfg.frame_length, cfg.num_channels
    fb = fl * ch * wr.BPS[cfg.bit_depth]
    stride = stride or (fb + 15) // 16 * 16
    dev = b.d_blob.device
    raw = torch.full((n * stride + 64,), 0x5A, dtype=torch.uint8, device=dev)
    assert raw.data_ptr() % 16 == 0
    d_out = raw[pcm_mis:pcm_mis + n * stride]
    d_fr = torch.full((n,), 12345, dtype=torch.int32, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    lead = 8 + wave_mis // 4
    if layout == wr.STREAM:
        cs, ps = n * fl + slack, 0
        elems = lead + ch * cs + 8
    else:
        cs = fl + slack
        ps = ch * cs + (slack and slack + 1)
        elems = lead + n * ps + 8
    buf = torch.full((elems,), wr.SENTINEL - (1 << 32), dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0
    d_starts = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    dec.decode_batch_device(b.d_blob.data_ptr(), b.d_blob.numel(), b.d_off.data_ptr(), b.d_sz.data_ptr(), n, d_out.data_ptr(), stride,
                            d_fr.data_ptr(), d_st.data_ptr(), sync=False)
    dec.waveform_device(d_out.data_ptr(), stride, d_fr.data_ptr(), d_st.data_ptr() if use_status else None, n, layout, wtype,
                        buf.data_ptr() + 4 * lead, cs, ps, d_starts.data_ptr() if want_starts else None, sync=True)
    return (buf.cpu().numpy().view(np.uint32), lead, cs, ps, d_starts.cpu().numpy().view(np.uint64),
            d_fr.cpu().numpy().view(np.uint32), d_st.cpu().numpy())


def check_pass(torch, dec, b, layout, wtype, **kw):
    img, base, cs, ps, starts, frames, status = device_pass(torch, dec, b, layout, wtype, **kw)
    out, r_frames, r_status = b.ref
    fl, depth, ch = b.cfg.frame_length, b.cfg.bit_depth, b.cfg.num_channels
    assert np.array_equal(status, r_status) and np.array_equal(frames, r_frames)
    use_status = kw.get("use_status", True)
    s_ref, ref_starts = wr.ref_stream(out, r_frames, r_status, fl, depth, ch, wtype, use_status)
    ref = s_ref if layout == wr.STREAM else wr.ref_packets(out, r_frames, r_status, fl, depth, ch, wtype, use_status)
    if kw.get("want_starts", True):
        assert np.array_equal(starts, ref_starts), "d_starts is not the cumsum"
    else:
        assert np.all(starts == np.uint64(0xFFFFFFFFFFFFFFFF))
    want = wr.expected_image(ref, layout, img.size, base, cs, ps)
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError("element %d of the buffer (tensor starts at %d): got %#x, want %#x (%d differ)"
                             % (bad[0], base, img[bad[0]], want[bad[0]], len(bad)))


@pytest.mark.parametrize("fl", [4096, 4095, 1])
@pytest.mark.parametrize("ch", [1, 2, 3, 6, 8])
@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_matrix_behind_an_unsynchronized_decode(torch, pkg, oracle, synth, helpers, depth, ch, fl):
    cfg = oracle.make_config(fl, depth, ch)
    packets = packet_list(synth, helpers, cfg, 12 if fl > 1 else 600, depth * 100 + ch * 10 + fl % 7, damaged=3)
    b = Batch(torch, oracle, helpers, cfg, packets)
    with pkg.NewPacketDecoder(to_pkg_cfg(pkg, cfg), 0) as dec:
        for layout in (wr.STREAM, wr.PACKETS):
            for wtype in (wr.FLOAT, wr.INT):
                check_pass(torch, dec, b, layout, wtype, slack=0 if wtype == wr.FLOAT else 5)
        ms = dec.waveform_last_ms()
        assert ms > 0
        assert dec.last_kernel_ms() > 0  # the decode's own timing is still there


@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 4096), (24, 2, 4096), (16, 2, 333), (20, 6, 70), (32, 1, 1000)])
def test_short_packets_anywhere(torch, pkg, oracle, synth, helpers, depth, ch, fl):
    """Packets of every length from PCM shorter than frame_length, at random places: start[i] odd and unaligned all along."""
    cfg = oracle.make_config(fl, depth, ch)
    rng = np.random.default_rng(fl + depth)
    b0 = synth.gen_batch(cfg, 24, base_seed=fl, threads=8)
    packets = [b0.packet(i) for i in range(b0.n)]
    for j in range(40):
        k = int(rng.integers(1, fl))
        packets.insert(int(rng.integers(0, len(packets) + 1)), short_packet(synth, cfg, k, j, escape=bool(j % 2) or k < 16))
    b = Batch(torch, oracle, helpers, cfg, packets)
    assert (b.ref[1] < fl).sum() >= 40 and not b.ref[2].any()
    with pkg.NewPacketDecoder(to_pkg_cfg(pkg, cfg), 0) as dec:
        for layout in (wr.STREAM, wr.PACKETS):
            check_pass(torch, dec, b, layout, wr.FLOAT, slack=3)
            check_pass(torch, dec, b, layout, wr.INT, wave_mis=8)


@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 4096), (24, 2, 512), (20, 3, 100), (32, 8, 64)])
def test_damaged_packets_are_skipped_or_silent(torch, pkg, oracle, synth, helpers, depth, ch, fl):
    """helpers.mutate_packets mixed in, d_status given once and NULL once: STREAM leaves the failed packets out, PACKETS
    writes them as zeros, d_starts is the cumsum."""
    cfg = oracle.make_config(fl, depth, ch)
    b = Batch(torch, oracle, helpers, cfg, packet_list(synth, helpers, cfg, 40, depth + fl, damaged=40))
    assert (b.ref[2] != 0).sum() >= 10 and (b.ref[2] == 0).sum() >= 10
    with pkg.NewPacketDecoder(to_pkg_cfg(pkg, cfg), 0) as dec:
        for use_status in (True, False):
            for layout in (wr.STREAM, wr.PACKETS):
                check_pass(torch, dec, b, layout, wr.FLOAT, use_status=use_status, slack=1)
        check_pass(torch, dec, b, wr.PACKETS, wr.INT, want_starts=False)


@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 4096), (24, 2, 4095), (20, 5, 333), (32, 8, 257), (16, 1, 4096)])
def test_footprint_at_irregular_layouts(torch, pkg, oracle, synth, helpers, depth, ch, fl):
    """A misaligned d_pcm with an odd pcm_stride (the decode's irregular route), and d_wave bases that are not 16-byte
    aligned with slack in both strides: the same values, and nothing outside the footprint."""
    cfg = oracle.make_config(fl, depth, ch)
    fb = fl * ch * wr.BPS[depth]
    b = Batch(torch, oracle, helpers, cfg, packet_list(synth, helpers, cfg, 16, depth + ch, damaged=4))
    with pkg.NewPacketDecoder(to_pkg_cfg(pkg, cfg), 0) as dec:
        for layout in (wr.STREAM, wr.PACKETS):
            check_pass(torch, dec, b, layout, wr.FLOAT, pcm_mis=3, stride=fb + 1 - fb % 2, slack=2)
            assert dec.last_dispatch()["narrow_slots"] == 0 and dec.last_dispatch()["wide_slots"] == 0
            check_pass(torch, dec, b, layout, wr.INT, pcm_mis=8, stride=(fb + 15) // 16 * 16 + 16, wave_mis=4, slack=1)
            check_pass(torch, dec, b, layout, wr.FLOAT, wave_mis=12, slack=3)


def test_argument_checks(torch, pkg, oracle):
    cfg = pkg.PacketConfig(FrameLength=64, BitDepth=16, NumChannels=2)
    dev = torch.device("cuda:0")
    n, fb = 4, 64 * 4
    pcm = torch.zeros(n * fb, dtype=torch.uint8, device=dev)
    fr = torch.zeros(n, dtype=torch.int32, device=dev)
    wave = torch.zeros(2 * n * 64 + 4, dtype=torch.float32, device=dev)
    starts = torch.full((1,), 9, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pkg.NewPacketDecoder(cfg, 0) as dec:
        P, F, W = pcm.data_ptr(), fr.data_ptr(), wave.data_ptr()
        bad = [
            (None, fb, F, None, n, 0, 0, W, n * 64, 0),      # NULL buffers
            (P, fb, None, None, n, 0, 0, W, n * 64, 0),
            (P, fb, F, None, n, 0, 0, None, n * 64, 0),
            (P, fb, F, None, n, 2, 0, W, n * 64, 0),         # unknown layout / type
            (P, fb, F, None, n, 0, 2, W, n * 64, 0),
            (P, fb - 1, F, None, n, 0, 0, W, n * 64, 0),     # pcm_stride below the frame bytes
            (P, fb, F, None, n, 0, 0, W, n * 64 - 1, 0),     # STREAM: channel_stride < n * frame_length
            (P, fb, F, None, n, 1, 0, W, 63, 2 * 63),        # PACKETS: channel_stride < frame_length
            (P, fb, F, None, n, 1, 0, W, 64, 2 * 64 - 1),    # PACKETS: packet_stride < channels * channel_stride
            (P, fb, F, None, n, 0, 0, W + 2, n * 64, 0),     # d_wave not on an element boundary
        ]
        for a in bad:
            with pytest.raises(ValueError):
                dec.waveform_device(*a, None, True)
        with pytest.raises(ValueError):
            dec.waveform_last_ms()  # no pass yet on this configuration
        dec.waveform_device(None, 0, None, None, 0, 0, 0, None, 0, 0, starts.data_ptr(), True)  # an empty batch
        assert int(starts.cpu()[0]) == 0
    assert not wave.cpu().numpy().any()


# ---- the Python entries --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 4096), (24, 6, 512)])
def test_decode_waveform_numpy_and_cuda_inputs(torch, pkg, oracle, synth, helpers, depth, ch, fl):
    cfg = oracle.make_config(fl, depth, ch)
    packets = packet_list(synth, helpers, cfg, 20, fl, damaged=5)
    blob, offs, sizes = helpers.pack_dense(packets)
    ref_triple = oracle.decode_batch(cfg, np.concatenate([blob, np.zeros(64, np.uint8)]), offs, sizes, threads=8)
    out, r_frames, r_status = ref_triple
    offs1 = np.concatenate([offs, [offs[-1] + sizes[-1]]]).astype(np.uint64)
    dev = torch.device("cuda:0")
    with pkg.NewPacketDecoder(to_pkg_cfg(pkg, cfg), 0) as dec:
        inputs = [
            (blob, offs, sizes), (blob.tobytes(), offs1, None),
            (torch.from_numpy(blob).to(dev), torch.from_numpy(offs.astype(np.int64)).to(dev), torch.from_numpy(sizes.astype(np.int32)).to(dev)),
            (torch.from_numpy(blob).to(dev), torch.from_numpy(offs1.astype(np.int64)).to(dev), None),
        ]
        for bl, of, sz in inputs:
            for dtype, wtype in ((torch.float32, wr.FLOAT), (torch.int32, wr.INT)):
                wave, frames, status = dec.decode_waveform(bl, of, sz, layout="stream", dtype=dtype)
                assert wave.is_cuda and wave.dtype is dtype and frames.is_cuda and status.is_cuda
                assert np.array_equal(status.cpu().numpy(), r_status) and np.array_equal(frames.cpu().numpy().view(np.uint32), r_frames)
                ref = wr.ref_stream(out, r_frames, r_status, fl, depth, ch, wtype)[0]
                assert tuple(wave.shape) == ref.shape
                assert np.array_equal(wave.contiguous().view(torch.int32).cpu().numpy().view(np.uint32), ref)
            wave, _, _ = dec.decode_waveform(bl, of, sz, layout="packets")
            ref = wr.ref_packets(out, r_frames, r_status, fl, depth, ch, wr.FLOAT)
            assert tuple(wave.shape) == (len(packets), ch, fl) and wave.dtype is torch.float32
            assert np.array_equal(wave.view(torch.int32).cpu().numpy().view(np.uint32), ref)


def stream_packets(synth, cfg, n, seed):
    b = synth.gen_batch(cfg, n, base_seed=seed, threads=8)
    packets = [b.packet(i) for i in range(b.n)]
    packets.append(short_packet(synth, cfg, cfg.frame_length // 3 + 1, seed, escape=False))  # a file's short last packet
    return packets


@pytest.mark.parametrize("depth,ch", [(16, 2), (24, 2), (16, 6), (24, 6)])
def test_load_equals_the_stream_decoder(torch, pkg, oracle, synth, helpers, tmp_path, depth, ch):
    """load() on a container written by tests/m4a.py = NewDecoder(src).ReadAll() through the numpy restatement; from
    bytes and from a path, float32 and int32."""
    fl = 4096
    cfg = oracle.make_config(fl, depth, ch)
    packets = stream_packets(synth, cfg, 37, depth + ch)
    data = m4a.write_m4a(cfg, packets, per_chunk=[5, 3], gap=7)
    with pkg.NewDecoder(data) as d:
        pcm = np.frombuffer(d.ReadAll(), np.uint8)
        rate = d.Format().SampleRate
    total = pcm.size // (ch * wr.BPS[depth])
    blob, offs, sizes = helpers.pack_packets(packets)
    assert total == int(oracle.decode_batch(cfg, blob, offs, sizes, threads=8)[1].sum()) and total % fl  # the rows close up
    v = wr.unpack(pcm, total, depth, ch)
    path = tmp_path / "a.m4a"
    path.write_bytes(data)
    for src in (data, str(path)):
        wave, sr = pkg.load(src)
        assert sr == rate and wave.dtype is torch.float32 and wave.is_cuda and tuple(wave.shape) == (ch, total)
        assert np.array_equal(wave.contiguous().view(torch.int32).cpu().numpy().view(np.uint32), wr.elements(v, depth, wr.FLOAT).T)
    wave, _ = pkg.load(data, dtype=torch.int32)
    assert np.array_equal(wave.contiguous().cpu().numpy().view(np.uint32), wr.elements(v, depth, wr.INT).T)


def test_load_in_several_windows(torch, pkg, oracle, synth):
    """More packets than one 48 MB window holds (8-channel 32-bit frames of 4096: 384 packets a window)."""
    cfg = oracle.make_config(4096, 32, 8)
    one = stream_packets(synth, cfg, 50, 1)
    packets = (one[:-1] * 9)[:430] + one[-1:]
    data = m4a.write_m4a(cfg, packets)
    with pkg.NewDecoder(data) as d:
        pcm = np.frombuffer(d.ReadAll(), np.uint8)
    total = pcm.size // 32
    wave, _ = pkg.load(data, dtype=torch.int32)
    assert tuple(wave.shape) == (8, total)
    assert np.array_equal(wave.contiguous().cpu().numpy().view(np.uint32), wr.elements(wr.unpack(pcm, total, 32, 8), 32, wr.INT).T)


def test_load_raises_what_read_raises(torch, pkg, oracle, synth):
    cfg = oracle.make_config(4096, 16, 2)
    packets = stream_packets(synth, cfg, 12, 3)
    k = 7
    packets[k] = packets[k][:len(packets[k]) // 2]  # truncated: a bitstream overrun
    data = m4a.write_m4a(cfg, packets)
    stream = importlib.import_module("saprobe-alac_amd.stream")
    with pkg.NewDecoder(data) as d:
        d.Read(k * 4096 * 4)
        with pytest.raises(pkg.ErrDecode) as read_err:
            d.Read(1)
    with pytest.raises(pkg.ErrDecode) as load_err:
        pkg.load(data)
    assert str(load_err.value) == str(read_err.value) and "decoding packet %d" % k in str(load_err.value)
    assert load_err.value.status == read_err.value.status and load_err.value.sentinel == read_err.value.sentinel
    with pytest.raises(stream.ErrNoTrack):
        pkg.load(m4a.box(b"ftyp", b"M4A ") + bytes(64))


# ---- the benchmark batch ---------------------------------------------------------------------------------------------------
def test_large_batch_against_the_torch_composition(torch, pkg, oracle, synth):
    """65 536 x 4096-frame 16-bit stereo packets in STREAM / FLOAT (4 096 distinct packets, each named sixteen times by the
    offsets; a few short ones, so that the rows close up), compared on the device with the composition of torch ops a caller
    would write: nothing of the 2-GiB result is pulled to the host."""
    fl, n = 4096, 65536
    cfg = oracle.make_config(fl, 16, 2)
    b = synth.gen_batch(cfg, 4096, threads=16)
    packets = [b.packet(i) for i in range(b.n)]
    for j, k in ((5, 1), (1000, 2047), (4095, 4093)):
        packets[j] = short_packet(synth, cfg, k, j, escape=k < 16)
    sizes = np.array([len(p) for p in packets], np.uint32)
    offs = np.zeros(len(packets), np.uint64)
    offs[1:] = np.cumsum(sizes[:-1])
    blob = np.frombuffer(b"".join(packets), np.uint8)
    dev = torch.device("cuda:0")
    pick = torch.arange(n, device=dev) % 4096
    d_blob = torch.from_numpy(blob.copy()).to(dev)
    d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)[pick].contiguous()
    d_sz = torch.from_numpy(sizes.astype(np.int32)).to(dev)[pick].contiguous()
    stride = fl * 4
    pcm = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    fr = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    wave = torch.full((2, n * fl), float("nan"), dtype=torch.float32, device=dev)
    starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with pkg.NewPacketDecoder(to_pkg_cfg(pkg, cfg), 0) as dec:
        dec.reserve(n)
        dec.decode_batch_device(d_blob.data_ptr(), d_blob.numel(), d_off.data_ptr(), d_sz.data_ptr(), n, pcm.data_ptr(), stride,
                                fr.data_ptr(), st.data_ptr(), sync=False)
        dec.waveform_device(pcm.data_ptr(), stride, fr.data_ptr(), st.data_ptr(), n, wr.STREAM, wr.FLOAT, wave.data_ptr(), n * fl, 0,
                            starts.data_ptr(), sync=True)
    assert not st.any().item()
    total = int(fr.sum().item())
    ref_frames = oracle.decode_batch(cfg, np.concatenate([blob, np.zeros(64, np.uint8)]), offs, sizes, threads=16, want_output=False)[1]
    assert total == 16 * int(ref_frames.sum()) <= n * fl - 16 * (4095 + 2049 + 3)  # (synth's stream has short packets of its own)
    assert torch.equal(starts[1:], torch.cumsum(fr.to(torch.int64), 0)) and int(starts[0].item()) == 0
    keep = torch.arange(fl, device=dev)[None, :] < fr[:, None]
    comp = (pcm.view(torch.int16).view(n, fl, 2)[keep].to(torch.float32) * (2.0 ** -15)).t().contiguous()
    assert tuple(comp.shape) == (2, total)
    assert torch.equal(wave[:, :total].view(torch.int32), comp.view(torch.int32))
    assert torch.isnan(wave[:, total:]).all().item()


def test_decode_waveform_rejects_what_it_cannot_count(torch, pkg):
    """offsets without sizes has n + 1 entries: none at all is an error, one is an empty batch."""
    cfg = pkg.PacketConfig(FrameLength=64, BitDepth=16, NumChannels=2)
    with pkg.NewPacketDecoder(cfg, 0) as dec:
        with pytest.raises(ValueError):
            dec.decode_waveform(b"", np.zeros(0, np.uint64))
        with pytest.raises(ValueError):
            dec.decode_waveform(b"\0" * 8, np.zeros(2, np.uint64), np.zeros(3, np.uint32))
        wave, frames, status = dec.decode_waveform(b"", np.zeros(1, np.uint64))
        assert tuple(wave.shape) == (2, 0) and frames.numel() == 0 and status.numel() == 0
        clips, _, _ = dec.decode_waveform(b"", np.zeros(0, np.uint64), np.zeros(0, np.uint32), layout="packets")
        assert tuple(clips.shape) == (0, 2, 64)
        buf = torch.empty((2, 100), dtype=torch.float32, device="cuda:0")
        with pytest.raises(ValueError):  # the private window path raises, it does not assert
            dec._decode_waveform(b"\0" * 8, np.zeros(2, np.uint64), np.full(2, 4, np.uint32), "stream", torch.float32, into=(buf, 0))
