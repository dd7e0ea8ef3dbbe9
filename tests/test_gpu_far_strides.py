"""Small data, far strides: every device-resident entry with buffers in which a packet, a slot, a row, a clip, a channel or a bin
lies 2^32 bytes and more behind the pointer the entry is given, because the caller's strides (or offsets[]) put it there. A
32-bit product in an address (pkt * out_stride, row * in_stride, c * channel_stride, an offsets[i] narrowed on the way) passes
the rest of the suite, whose largest buffer is 2 GiB, and breaks here.

Offsets are counted from the pointer handed to the entry; each run has footprints on both sides of byte 2^32 and, where the
geometry allows, one that straddles it. Every buffer is one sentinel-filled allocation from that pointer to its last element,
byte buffers with 2 GiB in front of it (tests/far_buffers.py), so a truncated or sign-extended offset lands in the test's own
memory: no test provokes a fault. Comparisons run on the device (far_buffers.check_footprints: every footprint against the
uploaded expectation, all that differ named, then every other byte must still be the sentinel, in chunks of 256 MiB); the
expectations are those the suite already trusts, computed on compact copies of the small data: the oracle, the numpy
restatements wave_ref / clip_ref / wavepack_ref, and the host builds of the resampler, mel, melfft and fbank headers, bit for
bit (the Kaldi features' logging pass by test_gpu_fbank.py's own bound behind host-build bits). No tolerance is new.

tests/test_far_buffers.py shows without a GPU that these comparisons name a slot, row or channel placed at a truncated offset."""
import numpy as np
import pytest

from tests import clip_ref as cr
from tests import far_buffers as fb
from tests import kaldi_ref as kr
from tests import mel_ref as mr
from tests import melfft_ref as fr
from tests import resample_ref as rr
from tests import wave_ref as wr
from tests import wavepack_ref as pr

pytestmark = pytest.mark.gpu

LINE = fb.LINE
E4 = LINE // 4  # the line in 4-byte elements
SHIFT = {16: 0, 20: 0, 24: 1, 32: 2}
F32_FILL = wr.SENTINEL - (1 << 32)  # the float / int32 buffers' sentinel as an int32


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture()
def meter(torch, request):
    m = fb.Meter(torch, request.node.name)
    yield m
    m.report()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def as_i32(torch, a):
    """a float32 / uint32 / int32 numpy array -> an int32 tensor of its bits on the device"""
    return to_dev(torch, np.ascontiguousarray(a).view(np.int32))


# ---- the decoder ---------------------------------------------------------------------------------------------------------------
N_PACKETS = 192
STRIDE = fb.slot_stride()  # 2^25 - 16: slot 128 begins 2 048 bytes below the line
# name, depth, channels, frame length, PB, profile of the full packets, what last_dispatch() must show at the aligned stride
FAMILIES = [
    ("quad16", 16, 2, 1024, 40, 0, dict(narrow="alac_decode_16q")),
    ("w24", 24, 2, 1024, 40, 5, dict(wide="alac_decode_w24")),            # PROFILE_MUSIC_NOSHIFT among the packets
    ("pairs32", 32, 2, 1024, 40, 0, dict(narrow="alac_decode_32q")),
    ("mono16", 16, 1, 2048, 40, 0, dict(narrow="alac_decode_16q")),       # 2 048 frames: a slot of 4 096 bytes straddles too
    ("interleave4", 24, 8, 1024, 40, 0, dict(irregular="alac_interleave4")),
    ("interleave", 16, 3, 1024, 40, 0, dict(irregular="alac_interleave (")),
    ("scan_pb74", 16, 2, 1024, 74, 0, dict(irregular="whole-packet")),
]


def family_packets(synth, helpers, cfg, profile, seed):
    """192 packets of 64 .. frame_length frames: full ones of `profile` and of PROFILE_STRESS, partial ones (MUSIC and STRESS
    signals, compressed and escaped), 8 mutated ones; slot 128, which straddles the line, holds a full packet."""
    fl, depth, ch = cfg.frame_length, cfg.bit_depth, cfg.num_channels
    rng = np.random.default_rng(seed)
    full = synth.gen_batch(cfg, 60, profile=profile, base_seed=seed, threads=8)
    stress = synth.gen_batch(cfg, 36, profile=synth.PROFILE_STRESS, base_seed=seed + 1, threads=8)
    packets = [full.packet(i) for i in range(1, full.n)] + [stress.packet(i) for i in range(stress.n)]
    ne = synth.num_elements(ch)
    for j in range(88):
        k = 64 + (j * 131) % (fl - 64)
        pcm = synth.signal(cfg, synth.PROFILE_STRESS if j % 2 else synth.PROFILE_MUSIC, seed + j, k)
        kw = dict(force_escape=1) if j % 4 == 3 else dict(never_escape=1, bytes_shifted=SHIFT[depth])
        packets.append(synth.encode_packet(cfg, [synth.default_elem(**kw) for _ in range(ne)], pcm))
    packets += helpers.mutate_packets(full, rng, 8)
    packets = [packets[i] for i in rng.permutation(len(packets))]
    packets.insert(128, full.packet(0))
    assert len(packets) == N_PACKETS
    return packets


class FarBlob:
    """The packets in a 0xFF-filled buffer of 2 GiB + 2^32 + 4 MiB bytes: a third of them dense from byte 3 on, one across byte
    2^32, the rest above it, each at an odd offset."""

    def __init__(self, torch, packets):
        n = len(packets)
        third = next(j for j in range(n // 3, n) if len(packets[j]) >= 64)
        low = b"".join(packets[:third])
        across = packets[third]
        assert len(across) >= 2
        at = LINE - len(across) // 2
        up = (LINE + len(across) + 1) | 1
        offs = np.zeros(n, np.uint64)
        sizes = np.array([len(p) for p in packets], np.uint32)
        offs[:third] = 3 + np.concatenate([[0], np.cumsum(sizes[:third - 1])])
        offs[third] = at
        high = bytearray()
        for j in range(third + 1, n):  # every packet above the line at an odd offset: a 0xFF byte in front where it takes one
            if (up + len(high)) % 2 == 0:
                high += b"\xff"
            offs[j] = up + len(high)
            high += packets[j]
        high = bytes(high)
        assert all(int(o) % 2 == 1 for o in offs[third + 1:])
        self.blob_bytes = up + len(high)
        assert self.blob_bytes <= LINE + (4 << 20) and 3 + len(low) < at
        self.far = fb.Far(torch, torch.uint8, LINE + (4 << 20), 0xFF, lead=fb.BYTE_LEAD)
        self.pieces = [(3, to_dev(torch, np.frombuffer(low, np.uint8))), (at, to_dev(torch, np.frombuffer(across, np.uint8))),
                       (up, to_dev(torch, np.frombuffer(high, np.uint8)))]
        for off, t in self.pieces:
            self.far.place(off, t)
        self.offs, self.sizes = offs, sizes
        self.d_off = to_dev(torch, offs.astype(np.int64))
        self.d_sz = to_dev(torch, sizes.astype(np.int32))
        fb.assert_crosses([int(o) for o in offs], [int(s) for s in sizes], 1, LINE, what="blob")

    def assert_unchanged(self, torch):
        rows = [("piece at %d" % off, off, t, t.numel()) for off, t in self.pieces]
        fb.check_footprints(torch, self.far, rows, "the blob after the passes", unit="piece")
        assert torch.equal(self.d_off, to_dev(torch, self.offs.astype(np.int64))) and \
            torch.equal(self.d_sz, to_dev(torch, self.sizes.astype(np.int32)))


def slot_rows(torch, ref, bpf, fbytes, stride):
    """check_footprints' rows for decoded slots: the oracle's frames; a failing packet's slot is unspecified over its frame
    bytes (tests/test_gpu_output_layout.py's table); everything else in and between the slots is the sentinel"""
    out, frames, status = ref
    d_out = to_dev(torch, out)
    rows = []
    for i in range(len(frames)):
        nb = int(frames[i]) * bpf
        ok = status[i] == 0
        rows.append((i, i * stride, d_out[i, :nb] if ok else None, nb if ok else fbytes))
    return rows


@pytest.mark.parametrize("name,depth,ch,fl,pb,profile,expect", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_decode_into_far_slots_from_a_far_blob(torch, pkg, oracle, synth, helpers, meter, name, depth, ch, fl, pb, profile, expect):
    """alacgpu_decode_batch_device, 192 packets whose bytes lie on both sides of blob byte 2^32 (one across it, d_sizes given,
    blob_bytes the true size) into slots 2^25 - 16 bytes apart (aligned16) and 2^25 - 15 (not): slot 128 begins 2 048 bytes
    below output byte 2^32 and holds a full packet of at least 4 096 bytes, 128 slots lie below it and 63 beyond. Frames,
    status words and every slot's bytes are the oracle's; every other byte of the 8 GiB output, its 2 GiB lead included, is
    still the sentinel, and the blob is unchanged.

    Why a wrapped offset shows: a 32-bit pkt * out_stride puts slot 129 at byte 2^25 - 2 064, in front of slot 1, and leaves its
    own place the sentinel: both are named. A blob offset narrowed to 32 bits reads packet k > 64 from the low third, where
    other packets lie (or 0xFF): the status or the PCM differs from the oracle's. Peak device memory 14.3 GiB: 6 GiB blob, 8 GiB
    output."""
    fb._need_gb(torch, 16)
    cfg = oracle.make_config(fl, depth, ch, pb=pb)
    bpf = ch * oracle.bytes_per_sample(depth)
    packets = family_packets(synth, helpers, cfg, profile, depth * 100 + ch * 10 + pb)
    blob, offs, sizes = helpers.pack_packets(packets)
    ref = oracle.decode_batch(cfg, blob, offs, sizes, threads=8)
    assert ref[2][128] == 0 and int(ref[1][128]) * bpf >= 4096 and 4 <= (ref[2] != 0).sum() <= 16
    assert len(set(ref[1].tolist())) > 40 and ref[1].min() < fl // 2  # packets of many lengths
    inp = FarBlob(torch, packets)
    d_fr = torch.full((N_PACKETS,), -1, dtype=torch.int32, device="cuda:0")
    d_st = torch.full((N_PACKETS,), -1, dtype=torch.int32, device="cuda:0")
    want_fr, want_st = to_dev(torch, ref[1].view(np.int32)), to_dev(torch, ref[2])
    out = fb.Far(torch, torch.uint8, N_PACKETS * (STRIDE + 1), 0xA5, lead=fb.BYTE_LEAD)
    meter.mark()
    with pkg.NewPacketDecoder(cr.to_pkg_cfg(pkg, cfg)) as dec:
        for stride in (STRIDE, STRIDE + 1):
            assert out.ptr() % 16 == 0
            below, across, beyond = fb.assert_crosses([i * stride for i in range(N_PACKETS)],
                                                      [int(f) * bpf if s == 0 else 0 for f, s in zip(ref[1], ref[2])], 1, LINE, what=name)
            assert across == 1 and below >= 32 and beyond >= 32
            d_fr.fill_(-1)
            d_st.fill_(-1)
            torch.cuda.synchronize()
            dec.decode_batch_device(inp.far.ptr(), inp.blob_bytes, inp.d_off.data_ptr(), inp.d_sz.data_ptr(), N_PACKETS, out.ptr(),
                                    stride, d_fr.data_ptr(), d_st.data_ptr(), sync=True)
            meter.mark()
            what = "%s stride %d" % (name, stride)
            assert torch.equal(d_st, want_st), "%s: status differs at %s" % (what, torch.nonzero(d_st != want_st).flatten().tolist())
            assert torch.equal(d_fr, want_fr), "%s: frames differ at %s" % (what, torch.nonzero(d_fr != want_fr).flatten().tolist())
            fb.check_footprints(torch, out, slot_rows(torch, ref, bpf, fl * bpf, stride), what)
            d = dec.last_dispatch()
            if stride % 16:
                assert d["narrow_slots"] == 0 and d["wide_slots"] == 0 and d["irregular_slots"] == d["slots"] > 0, d
            elif "narrow" in expect:
                assert d["narrow_kernel"] == expect["narrow"] and d["narrow_slots"] > 0 and not d["gated"], d
            elif "wide" in expect:
                assert d["wide_kernel"] == expect["wide"] and d["wide_slots"] > 0 and d["narrow_slots"] > 0, d
            else:
                assert expect["irregular"] in d["irregular_kernels"] and d["irregular_slots"] > 0, d
                assert d["narrow_slots"] == 0 and d["wide_slots"] == 0, d
    inp.assert_unchanged(torch)


def test_gated_pairs_write_far_slots(torch, pkg, oracle, synth, helpers, meter):
    """The gated twin of the 16-bit wave pairs (alac_decode_16g) runs only between four and five rounds of a device of 256 CUs,
    which 192 packets never are: 70 000 stereo packets of 128 frames at a stride of 2^16 - 16, so that slot 65 552 begins 256
    bytes below output byte 2^32 and straddles it and 4 447 slots lie beyond (4.3 GiB of output behind 2 GiB of lead). The
    slots are the oracle's, gathered with one strided view; everything else is the sentinel.

    A 32-bit pkt * out_stride puts slot 65 553 + j at byte 65 264 + j * 65 520, 256 bytes in front of slot j + 1 and onto its first 256
    bytes, never onto its own place: those slots keep the sentinel, and they and the slots written over are named. Peak device memory 6.7 GiB."""
    fb._need_gb(torch, 8)
    n, fl = 70000, 128
    stride = (1 << 16) - 16
    cfg = oracle.make_config(fl, 16, 2)
    b = synth.gen_batch(cfg, n, base_seed=16, threads=16)
    ref = oracle.decode_batch(cfg, b.blob, b.offsets, b.sizes, threads=16)
    assert not ref[2].any()
    nb = ref[1].astype(np.int64) * 4
    below, across, beyond = fb.assert_crosses([i * stride for i in range(n)], nb.tolist(), 1, LINE)
    assert across == 1 and beyond > 4000 and nb[65552] == fl * 4
    want = np.where(np.arange(fl * 4)[None, :] < nb[:, None], ref[0][:, :fl * 4], np.uint8(0xA5))
    d_blob, d_off, d_sz = to_dev(torch, b.blob), to_dev(torch, b.offsets.astype(np.int64)), to_dev(torch, b.sizes.astype(np.int32))
    out = fb.Far(torch, torch.uint8, n * stride, 0xA5, lead=fb.BYTE_LEAD)
    d_fr = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with pkg.NewPacketDecoder(cr.to_pkg_cfg(pkg, cfg)) as dec:
        dec.decode_batch_device(d_blob.data_ptr(), d_blob.numel(), d_off.data_ptr(), d_sz.data_ptr(), n, out.ptr(), stride,
                                d_fr.data_ptr(), d_st.data_ptr(), sync=True)
        meter.mark()
        d = dec.last_dispatch()
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert d["narrow_kernel"] == "alac_decode_16g" and d["gated"] == 1, d
    assert not bool(d_st.any()) and torch.equal(d_fr, to_dev(torch, ref[1].view(np.int32)))
    fb.check_strided(torch, out, stride, to_dev(torch, want), "gated pairs")
    assert torch.equal(d_blob, to_dev(torch, b.blob))


# ---- waveform and clips behind a decode into far slots ------------------------------------------------------------------------
class FarDecode:
    """192 16-bit stereo packets of up to 1 024 frames decoded with sync=False into slots 2^25 - 16 bytes apart (8 GiB with
    the lead), the oracle's triple next to them."""

    def __init__(self, torch, pkg, oracle, synth, helpers, dec, seed):
        self.cfg = oracle.make_config(1024, 16, 2)
        packets = family_packets(synth, helpers, self.cfg, 0, seed)
        self.b = cr.Batch(torch, oracle, helpers, self.cfg, packets)
        self.ref = self.b.ref
        self.n = self.b.n
        self.out = fb.Far(torch, torch.uint8, self.n * STRIDE, 0xA5, lead=fb.BYTE_LEAD)
        self.d_fr = torch.full((self.n,), -1, dtype=torch.int32, device="cuda:0")
        self.d_st = torch.full((self.n,), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        dec.decode_batch_device(self.b.d_blob.data_ptr(), self.b.d_blob.numel(), self.b.d_off.data_ptr(), self.b.d_sz.data_ptr(), self.n,
                                self.out.ptr(), STRIDE, self.d_fr.data_ptr(), self.d_st.data_ptr(), sync=False)

    def slots(self):
        """the oracle's slots as the restatements take them: [n, frame bytes]"""
        return self.ref[0][:, :1024 * 4], self.ref[1], self.ref[2]

    def assert_slots(self, torch, what):
        fb.check_footprints(torch, self.out, slot_rows(torch, self.ref, 4, 4096, STRIDE), what + ": the slots afterwards")


def wave_rows(torch, ref, layout, cs, ps):
    """check_footprints' rows of a waveform: STREAM [ch, total] -> one per channel; PACKETS [n, ch, fl] -> one per packet and
    channel"""
    d = as_i32(torch, ref)
    if layout == wr.STREAM:
        return [(c, c * cs, d[c], d.shape[1]) for c in range(d.shape[0])]
    return [("%d (channel %d)" % (i, c), i * ps + c * cs, d[i, c], d.shape[2]) for i in range(d.shape[0]) for c in range(d.shape[1])]


def test_waveform_and_clips_with_far_strides_behind_a_far_decode(torch, pkg, oracle, synth, helpers, meter):
    """Behind one decode with sync=False into the far slots of the test above (the passes read slots on both sides of input
    byte 2^32), into one 12 GiB buffer of 4-byte elements:

      waveform_device STREAM, channel_stride 2^30 + 5: channel 1 begins 20 bytes beyond the line; FLOAT and INT
      waveform_device PACKETS, channel_stride 1 027, packet_stride 2^23 - 4: packet 128's row begins 2 048 bytes below the line
                      and straddles it, 63 packets lie beyond; FLOAT and INT; d_starts checked in both layouts
      clips_device    160 clips of 700 frames, clip_stride 2^23 - 4 (clip 128 straddles), begins from clip_ref.spread: inside a
                      slot, across slot boundaries, over short and failed slots and over the grid's end; valid[], clip_status[]
      clips_device    2 clips, channel_stride 2^30 + 5 alone far (clip_stride 2 channel strides): three of the four rows begin
                      beyond the line

    A 32-bit c * channel_stride * 4 puts channel 1 on channel 0's columns 5 .., a 32-bit i * packet_stride * 4 puts packet 129
    in front of packet 1; a 32-bit pkt * pcm_stride reads slot 129 from the gap in front of slot 1, which holds the sentinel
    0xA5, not PCM. Either way the footprint's own place differs and is named. The slots are unchanged afterwards. Peak device
    memory 20.2 GiB: 8 GiB of slots, 12 GiB of waveform."""
    fb._need_gb(torch, 22)
    fl, ch = 1024, 2
    cs_far, ps_far = E4 + 5, (E4 >> 7) - 4
    with pkg.NewPacketDecoder(pkg.PacketConfig(FrameLength=fl, BitDepth=16, NumChannels=ch)) as dec:
        fd = FarDecode(torch, pkg, oracle, synth, helpers, dec, 77)
        n = fd.n
        out, frames, status = fd.slots()
        wave = fb.Far(torch, torch.int32, 3 * cs_far + 4096, F32_FILL, lead=5)
        meter.mark()
        d_starts = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
        for wtype in (wr.FLOAT, wr.INT):
            s_ref, starts = wr.ref_stream(out, frames, status, fl, 16, ch, wtype)
            total = int(starts[-1])
            fb.assert_crosses([0, cs_far], [total] * 2, 4, LINE, straddle=False)
            d_starts.fill_(-1)
            dec.waveform_device(fd.out.ptr(), STRIDE, fd.d_fr.data_ptr(), fd.d_st.data_ptr(), n, wr.STREAM, wtype, wave.ptr(), cs_far, 0,
                                d_starts.data_ptr(), sync=True)
            assert torch.equal(d_starts, to_dev(torch, starts.astype(np.int64)))
            fb.check_footprints(torch, wave, wave_rows(torch, s_ref, wr.STREAM, cs_far, 0), "STREAM type %d" % wtype, unit="channel")
            p_ref = wr.ref_packets(out, frames, status, fl, 16, ch, wtype)
            cs = fl + 3
            assert fb.assert_crosses([i * ps_far for i in range(n)], [fl] * n, 4, LINE) == (128, 1, 63)
            d_starts.fill_(-1)
            dec.waveform_device(fd.out.ptr(), STRIDE, fd.d_fr.data_ptr(), fd.d_st.data_ptr(), n, wr.PACKETS, wtype, wave.ptr(), cs, ps_far,
                                d_starts.data_ptr(), sync=True)
            assert torch.equal(d_starts, to_dev(torch, starts.astype(np.int64)))
            fb.check_footprints(torch, wave, wave_rows(torch, p_ref, wr.PACKETS, cs, ps_far), "PACKETS type %d" % wtype, unit="packet")
        meter.mark()
        # clips: clip_stride far, then channel_stride alone
        rng = np.random.default_rng(12)
        L = 700
        begin16, _ = cr.spread(rng, n, fl, L)
        begin16.append(int(np.nonzero(status)[0][0]) * fl - 10)  # and into the first failed slot
        for what, B, cs, ps, wtype in (("clip_stride far", 160, L + 1, ps_far, wr.FLOAT), ("clip_stride far, INT", 160, L + 1, ps_far, wr.INT),
                                       ("channel_stride far", 2, cs_far, 2 * cs_far + 2, wr.FLOAT)):
            begin = [begin16[(j * 5) % len(begin16)] for j in range(B)] if B > 2 else [n * fl - 300, fl - 1]
            limit = [n] * B
            ref, valid, cstat = cr.ref_clips(out, frames, status, fl, 16, ch, wtype, begin, limit, L)
            assert valid.min() < L and valid.max() > 0 and (B == 2 or (len(set(valid.tolist())) > 3 and cstat.any()))
            offs = [j * ps + c * cs for j in range(B) for c in range(ch)]
            below, across, beyond = fb.assert_crosses(offs, [L] * len(offs), 4, LINE, straddle=B > 2)
            assert beyond >= (60 if B > 2 else 3)
            d_begin = to_dev(torch, np.array(begin, np.int64))
            d_limit = to_dev(torch, np.array(limit, np.int64))
            d_valid = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
            d_cst = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            dec.clips_device(fd.out.ptr(), STRIDE, fd.d_fr.data_ptr(), fd.d_st.data_ptr(), n, d_begin.data_ptr(), d_limit.data_ptr(), B, L,
                             wtype, wave.ptr(), cs, ps, d_valid.data_ptr(), d_cst.data_ptr(), sync=True)
            d_ref = as_i32(torch, ref)
            rows = [("%d (channel %d)" % (j, c), j * ps + c * cs, d_ref[j, c], L) for j in range(B) for c in range(ch)]
            fb.check_footprints(torch, wave, rows, what, unit="clip")
            assert torch.equal(d_valid, as_i32(torch, valid)) and torch.equal(d_cst, to_dev(torch, cstat)), what
            assert torch.equal(d_begin, to_dev(torch, np.array(begin, np.int64)))
        meter.mark()
        assert torch.equal(fd.d_fr, to_dev(torch, fd.ref[1].view(np.int32))) and torch.equal(fd.d_st, to_dev(torch, fd.ref[2]))
        fd.assert_slots(torch, "after the waveform and clip passes")


# ---- the pack pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [16, 24])
@pytest.mark.parametrize("wtype", [pr.FLOAT, pr.INT], ids=["float", "int"])
def test_pack_pass_reads_far_waveforms(torch, pkg, meter, depth, wtype):
    """alacgpu_pcm_from_waveform_device, stereo, FrameLength 1 024, from a NaN-sentinel-filled waveform buffer of 4.5 GiB:
    PACKETS with packet_stride 2^23 - 4 (136 clips and a short last one: clip 128 straddles the line, 8 lie beyond) and STREAM
    with channel_stride 2^30 + 5 (channel 1 begins beyond it); the PCM and the clipped count are wavepack_ref's on the compact
    waveform (loud samples, NaNs and infinities among them), the bytes around the dense PCM the sentinel, the waveform
    unchanged. The output is dense and small here; tests/test_gpu_beyond_4gib.py has the dense 4 GiB one.

    A 32-bit i * packet_stride * 4 reads clip 129 from in front of clip 1 and a 32-bit channel_stride * 4 reads channel 1
    from channel 0's column 5 on; what lies there is other audio or the NaN sentinel, which packs to 0 and counts as clipped, so
    the bytes or the count differ. Peak device memory 4.4 GiB."""
    fb._need_gb(torch, 6)
    fl, ch = 1024, 2
    cs_far, ps_far = E4 + 5, (E4 >> 7) - 4
    rng = np.random.default_rng(depth + wtype)
    total = 136 * fl + 333
    x = pr.random_wave(rng, ch, total, depth, wtype)
    want, clipped = pr.pack_ref(x, depth, wtype)
    assert clipped > 100
    d_x = as_i32(torch, x)
    wave = fb.Far(torch, torch.int32, 137 * ps_far, pr.WAVE_SENTINEL, lead=7)
    meter.mark()
    d_want = to_dev(torch, want)
    with pkg.NewPacketEncoder(pkg.PacketConfig(FrameLength=fl, BitDepth=depth, NumChannels=ch)) as enc:
        for layout in (pr.PACKETS, pr.STREAM):
            if layout == pr.PACKETS:
                cs, ps = fl + 5, ps_far
                rows = [("%d (channel %d)" % (i, c), i * ps + c * cs, d_x[c, i * fl:min((i + 1) * fl, total)], min(fl, total - i * fl))
                        for i in range(137) for c in range(ch)]
                assert fb.assert_crosses([r[1] for r in rows], [r[3] for r in rows], 4, LINE)[2] >= 16
            else:
                cs, ps = cs_far, 0
                rows = [(c, c * cs, d_x[c], total) for c in range(ch)]
                fb.assert_crosses([r[1] for r in rows], [total] * ch, 4, LINE, straddle=False)
            for _, off, t, _ in rows:
                wave.place(off, t)
            pcm = fb.Far(torch, torch.uint8, want.size + 64, pr.PCM_SENTINEL, lead=64)
            d_clip = torch.full((1,), 0xDEAD, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            enc.pcm_from_waveform_device(wave.ptr(), layout, wtype, cs, ps, total, pcm.ptr(), d_clip.data_ptr(), sync=True)
            what = "layout %d depth %d type %d" % (layout, depth, wtype)
            fb.check_footprints(torch, pcm, [("PCM", 0, d_want, want.size)], what, unit="buffer")
            assert int(d_clip.item()) == clipped, (what, int(d_clip.item()), clipped)
            fb.check_footprints(torch, wave, rows, what + ": the waveform afterwards", unit="clip" if layout == pr.PACKETS else "channel")


# ---- the resampler -------------------------------------------------------------------------------------------------------------
FAR_ROW = (E4 >> 1) - 501  # elements: row 2 of three begins 4 008 bytes below the line


@pytest.mark.parametrize("orig,new,T", [(44100, 16000, 3001), (2, 3, 2001)])
def test_resampled_rows_with_far_strides(torch, pkg, meter, orig, new, T):
    """alacgpu_resample_device, three rows: in_row_stride alone far (2^29 - 501 elements: row 2 begins 4 008 bytes below the line
    and straddles it), out_row_stride alone far, and both; the bases 4, 8 and 12 bytes off a 16-byte boundary in turn. The
    rows are the host build's, bit for bit; every other element of the 4 GiB output is the sentinel and the input, rows in a
    NaN-filled buffer, is unchanged.

    A 32-bit row * in_stride * 4 reads row 2 from 4 008 bytes in front of row 0 (the buffer's lead, NaN: the row comes out
    NaN); a 32-bit row * out_stride * 4 writes row 2 there and leaves its place the sentinel. Peak device memory 8 GiB."""
    fb._need_gb(torch, 10)
    sim = rr.build_resample_sim()
    x = rr.signal(np.random.default_rng(T), 3, T)
    frames = rr.out_frames(orig, new, T)
    y = np.zeros((3, frames), np.float32)
    assert sim.resample_sim_run(orig, new, 6, 0.99, x.ctypes.data, T, 3, T, y.ctypes.data, frames, 0) == 0
    d_x, d_y = as_i32(torch, x), as_i32(torch, y)
    nan = 0x7FC00000
    with pkg.NewResampler(orig, new) as rs:
        for k, (in_far, out_far) in enumerate(((True, False), (False, True), (True, True))):
            in_stride = FAR_ROW if in_far else T + 1
            out_stride = FAR_ROW if out_far else frames + 3
            lead = 1024 + 1 + k  # elements: 4, 8, 12 bytes behind a 16-byte boundary
            src = fb.Far(torch, torch.int32, 2 * in_stride + T + 8, nan, lead=lead)
            dst = fb.Far(torch, torch.int32, 2 * out_stride + frames + 8, F32_FILL, lead=lead)
            assert src.ptr() % 16 == dst.ptr() % 16 == 4 * (1 + k)
            meter.mark()
            in_rows = [(r, r * in_stride, d_x[r], T) for r in range(3)]
            out_rows = [(r, r * out_stride, d_y[r], frames) for r in range(3)]
            if in_far:
                assert fb.assert_crosses([r[1] for r in in_rows], [T] * 3, 4, LINE) == (2, 1, 0)
            if out_far:
                assert fb.assert_crosses([r[1] for r in out_rows], [frames] * 3, 4, LINE) == (2, 1, 0)
            for _, off, t, _ in in_rows:
                src.place(off, t)
            torch.cuda.synchronize()
            rs.resample_device(src.ptr(), in_stride, 3, T, dst.ptr(), out_stride, sync=True)
            what = "%d -> %d, in far %s, out far %s" % (orig, new, in_far, out_far)
            fb.check_footprints(torch, dst, out_rows, what, unit="row")
            fb.check_footprints(torch, src, in_rows, what + ": the input afterwards", unit="row")
            del src, dst


def test_one_resampled_row_across_the_line(torch, pkg, meter):
    """One row of T = 2^30 + 12 345 frames, 44 100 -> 16 000 (o = 441, n = 160): the row's own columns cross input byte 2^32, and
    j0 * o of its last tiles passes 2^30. The row is a block of 9 * 441 = 3 969 frames repeated on the device; 3 969 is odd, so
    the frame 2^30 elements lower (2^32 bytes) is another one of the block (2^30 = 1 387 mod 3 969).

    Away from the row's two ends the output then has the period 9 * 160 = 1 440 columns, and one period is the host build's,
    taken from the middle block of a three-block excerpt: EVERY interior column of the 390 million is held to it on the device
    (far_buffers.check_cycled). The first 1 440 columns, which see the zeros in front of the row, the excerpt around input byte
    2^32 and the columns from the last whole period to the row's end are compared with the host build run on excerpts. An
    excerpt starts at a multiple of o, so its column 0 is phase 0 of the row's column (start / o) * n; a column is compared only
    where all its inputs [j * o - width, (j + 1) * o + width) lie inside the excerpt (or beyond the row's own end, where both
    see zeros): the margin is `width` = 17 frames, one block of n columns at each cut end.

    A tile whose 32-bit input offset wrapped would read the frames 2^30 lower, a different place of the block: the period breaks
    from that tile on. Peak device memory 6.4 GiB: 4 GiB in, 1.45 GiB out, 1 GiB while the row is filled."""
    fb._need_gb(torch, 8)
    orig, new = 44100, 16000
    o, n, _, width = rr.geometry(orig, new)
    assert (o, n, width) == (441, 160, 17)
    block, T = 9 * o, (1 << 30) + 12345
    assert block % 2 == 1 and (1 << 30) % block != 0
    sim = rr.build_resample_sim()
    blk = rr.signal(np.random.default_rng(30), 2, block)[0]
    frames = rr.out_frames(orig, new, T)

    def host(a, e):
        """the host build's output of the excerpt [a, e) of the row -> float32 as int32, column 0 = the row's column a / o * n"""
        assert a % o == 0
        xs = np.ascontiguousarray(np.resize(np.roll(blk, -(a % block)), e - a))
        ys = np.zeros(rr.out_frames(orig, new, e - a), np.float32)
        assert sim.resample_sim_run(orig, new, 6, 0.99, xs.ctypes.data, e - a, 1, e - a, ys.ctypes.data, ys.size, 0) == 0
        return ys.view(np.int32)

    src = fb.Far(torch, torch.int32, T + 8, 0x7FC00000, lead=4)
    reps = -(-T // block)
    d_blk = as_i32(torch, blk)
    step = 1 << 16  # blocks per copy: 1 GiB at a time
    for a in range(0, reps, step):
        k = min(step, reps - a)
        m = min(k * block, T - a * block)
        src.at(a * block, m).copy_(d_blk.repeat(k)[:m])
    dst = fb.Far(torch, torch.int32, frames + 8, F32_FILL, lead=4)
    meter.mark()
    torch.cuda.synchronize()
    with pkg.NewResampler(orig, new) as rs:
        tile = rs.plan()["tile_out"]
        assert rs.out_frames(T) == frames and (frames - tile) // n * o > 1 << 30
        rs.resample_device(src.ptr(), T, 1, T, dst.ptr(), frames, sync=True)
    meter.mark()
    P = 9 * n
    period = host(0, 3 * block)[P:2 * P]
    # the first period, with the row's front edge
    assert torch.equal(dst.at(0, P), to_dev(torch, host(0, 3 * block)[:P])), "the first columns differ from the host build"
    # every interior period: the columns [P, last) with last the end of the last period whose inputs end inside the row
    whole = (T - width - o) // block
    body = dst.at(P, (whole - 1) * P).view(whole - 1, P)
    fb.check_cycled(torch, body, to_dev(torch, period)[None, :], "interior periods of 1 440 columns", unit="period")
    # around input byte 2^32: an excerpt of 20 blocks of o frames, its first and last n columns left out
    a = ((1 << 30) - 10 * o) // o * o
    ys = host(a, a + 20 * o)
    m0 = a // o * n
    assert a < 1 << 30 < a + 20 * o
    assert torch.equal(dst.at(m0 + n, 18 * n), to_dev(torch, ys[n:19 * n])), "columns around input byte 2^32 differ"
    # the row's end: from two blocks in front of the last whole period on, the first n columns of the excerpt left out
    a = (whole - 2) * block
    ys = host(a, T)
    m0 = a // o * n
    assert m0 + ys.size == frames
    assert torch.equal(dst.at(m0 + n, ys.size - n), to_dev(torch, ys[n:])), "the last columns differ from the host build"
    fb.assert_fill(torch, dst.t[:dst.lead], F32_FILL, "in front of the row")
    fb.assert_fill(torch, dst.t[dst.lead + frames:], F32_FILL, "behind the row")
    # the input is unchanged: the period, and the NaN around it
    fb.check_cycled(torch, src.at(0, (T // block) * block).view(T // block, block), d_blk[None, :], "the input afterwards", unit="block")
    assert torch.equal(src.at((T // block) * block, T % block), d_blk[:T % block])
    fb.assert_fill(torch, src.t[:src.lead], 0x7FC00000, "in front of the input")
    fb.assert_fill(torch, src.t[src.lead + T:], 0x7FC00000, "behind the input")


# ---- spectrograms --------------------------------------------------------------------------------------------------------------
def row_pass_rows(d_y, row_stride, inner_stride):
    """check_footprints' rows of a [rows, lines, length] output: one per (row, line)"""
    R, B, F = d_y.shape
    return [("%d (line %d)" % (r, b), r * row_stride + b * inner_stride, d_y[r, b], F) for r in range(R) for b in range(B)]


def far_row_pass(torch, meter, call, d_x, d_y, far, what):
    """One pass with one stride far: `far` is "in" (in_row_stride 2^29 - 101: row 2 straddles), "row" (out_row_stride 2^29 - 31:
    row 2 straddles) or "inner" (the bin / line stride (2^30 - length / 2) / (lines - 1): the last line of row 0 straddles, row 1
    lies beyond). d_x [rows, T] and d_y [rows, lines, length] int32 on the device -> the output buffer, checked."""
    R, T = d_x.shape
    _, B, F = d_y.shape
    in_stride = (E4 >> 1) - 101 if far == "in" else T + 1
    inner = (E4 - F // 2) // (B - 1) if far == "inner" else F + 1
    row_stride = (E4 >> 1) - 31 if far == "row" else (B - 1) * inner + F + 2
    src = fb.Far(torch, torch.int32, (R - 1) * in_stride + T + 8, 0x7FC00000, lead=5)
    dst = fb.Far(torch, torch.int32, (R - 1) * row_stride + (B - 1) * inner + F + 8, F32_FILL, lead=6)
    meter.mark()
    in_rows = [(r, r * in_stride, d_x[r], T) for r in range(R)]
    out_rows = row_pass_rows(d_y, row_stride, inner)
    rows = in_rows if far == "in" else out_rows
    fb.assert_crosses([r[1] for r in rows], [r[3] for r in rows], 4, LINE, what=what)
    for _, off, t, _ in in_rows:
        src.place(off, t)
    torch.cuda.synchronize()
    call(src.ptr(), in_stride, R, T, dst.ptr(), row_stride, inner)
    return src, in_rows, dst, out_rows


@pytest.mark.parametrize("far", ["in", "row", "inner"])
@pytest.mark.parametrize("transform", ["direct", "fft"])
def test_mel_rows_with_far_strides(torch, pkg, meter, transform, far):
    """alacgpu_mel_device, the case tiny / n16 (n_fft 16, hop 4, window 12, 5 mel bins), log off, direct and transform="fft":
    in_row_stride, out_row_stride and out_bin_stride far, each on its own (three rows; two where the bin stride is far, 2^28 - 10
    elements: bin 4 of row 0 straddles the line and row 1 lies beyond it). [rows][bins][F] is the host build's bit for bit,
    every other element the sentinel, the input unchanged.

    A 32-bit row * stride * 4 (or b * out_bin_stride * 4) reads row 2 from the NaN in front of row 0, or writes a row or a bin
    in front of row 0 and leaves its place the sentinel. Peak device memory 8 GiB (bin stride far), else 4 GiB."""
    fb._need_gb(torch, 11)
    cfg = mr.CASES["tiny"]
    assert cfg.log is None and (cfg.n_fft, cfg.bins) == (16, 5)
    R, T = (2 if far == "inner" else 3), 301
    x = mr.signal(np.random.default_rng(16), R, T)
    F = mr.out_frames(cfg, T)
    if transform == "fft":
        img, lay = fr.sim_image(fr.build_melfft_sim(), cfg, x)
    else:
        img, lay = mr.sim_image(mr.build_mel_sim(), cfg, x)
    y = mr.rows_of(img, R, cfg.bins, F, lay[5], lay[3], lay[4])
    kw = dict(transform="fft") if transform == "fft" else {}
    with pkg.NewMelSpectrogram(**kw, **cfg.kwargs()) as ms:
        assert ms.out_frames(T) == F > 64
        what = "mel %s, %s far" % (transform, far)
        src, in_rows, dst, out_rows = far_row_pass(torch, meter, lambda *a: ms.mel_device(*a, sync=True), as_i32(torch, x),
                                                   as_i32(torch, y), far, what)
    fb.check_footprints(torch, dst, out_rows, what, unit="row")
    fb.check_footprints(torch, src, in_rows, what + ": the input afterwards", unit="row")


# ---- Kaldi features ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("far", ["in", "row", "inner"])
@pytest.mark.parametrize("name", ["w10", "mfcc13"])
def test_kaldi_features_with_far_strides(torch, pkg, meter, name, far):
    """alacgpu_fbank_device, an fbank and an MFCC case of kaldi_ref.CASES, held as
    test_gpu_fbank.py::test_device_equals_the_host_build_and_logs_within_bounds holds them: the pass with nothing logged is the
    host build's bit for bit, and the case's own pass (log fbank; log, DCT and lifter) lies within kr.check_logged's derived
    bound of the float64 of those values. Both passes run with in_row_stride, out_row_stride (layout frames, three rows) and
    out_inner_stride (layout bins, where it is the bin stride and the large one; two rows) far, each on its own; the logged
    pass's values come to the host (a few hundred KB), everything around them is checked on the device.

    A 32-bit row or line offset reads NaN from in front of row 0 or writes there and leaves the line's own place the
    sentinel. Peak device memory 8 GiB (inner stride far: 23 or 13 lines up to the line, and a second row), else 4 GiB."""
    fb._need_gb(torch, 10)
    sim = kr.build_fbank_sim()
    cfg, _ = kr.CASES[name]
    layout = "bins" if far == "inner" else "frames"
    cfg = cfg.with_(layout=layout)
    pre = cfg.prelog()
    R = 2 if far == "inner" else 3
    T = kr.length_for(cfg, 200)
    F = kr.out_frames(cfg, T)
    assert F == 200
    x = kr.signal(np.random.default_rng(len(name)), R, T, 0.3)
    y = kr.host_values(sim, pre.with_(layout="frames"), x)  # [R, F, cols of the unlogged pass]
    for c, values in ((pre, y), (cfg, None)):
        lines, length = kr.out_shape(c, F)
        with pkg.NewKaldiFeatures(**c.kwargs()) as kf:
            assert kf.out_frames(T) == F
            what = "%s %s, %s far" % (name, "unlogged" if values is not None else "logged", far)
            if values is not None:
                d_y = as_i32(torch, values if layout == "frames" else values.transpose(0, 2, 1))
            else:
                d_y = torch.zeros((R, lines, length), dtype=torch.int32, device="cuda:0")  # the places; the values are read back
            src, in_rows, dst, out_rows = far_row_pass(torch, meter, lambda *a: kf.features_device(*a, sync=True), as_i32(torch, x),
                                                       d_y, far, what)
        if values is None:
            got = torch.stack([dst.at(off, n) for _, off, _, n in out_rows]).view(R, lines, length).cpu().numpy().view(np.float32)
            got = got if layout == "frames" else np.ascontiguousarray(got.transpose(0, 2, 1))
            kr.check_logged(cfg, got, y, what)
            out_rows = [(nm, off, None, n) for nm, off, _, n in out_rows]
        fb.check_footprints(torch, dst, out_rows, what, unit="row")
        fb.check_footprints(torch, src, in_rows, what + ": the input afterwards", unit="row")
        del src, dst
