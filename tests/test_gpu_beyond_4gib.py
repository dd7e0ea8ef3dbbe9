"""Real batches whose own size carries the output, the decode's scratch, the split pipeline's rows, the encoder's input and blob
and the pack pass's two sides over byte 2^32: what anyone decoding or encoding a corpus in one call does, and exactly what a
32-bit product in an address (pkt * out_stride, wave * u_tile_cells, pkt * nch * row_stride, an offsets[i] narrowed on the way)
breaks without a fault and without another test noticing: the suite's other buffers end at 2 GiB.

The batches cycle over an odd number of distinct packets (4 099, 1 031, 7), picked through d_offsets / d_sizes or repeated on
the device, so the expectation is that of one period (the oracle, the encoder's host build, wavepack_ref) and the comparison
runs on the device, chunk by chunk (tests/far_buffers.py: check_cycled). The periods are odd and do not divide floor(2^32 / stride) for any stride
here, so the slot or frame 2^32 bytes lower belongs to another class: a write or a read that wrapped breaks
the cycle at the first slot beyond the line and is named there. PCM outputs have 2 GiB of sentinel in front of them in the same
allocation and a few bytes behind; both must be intact. Every test frees the library's pooled handles when it is done
(alacgpu_trim). No test provokes a fault: every entry gets buffers of the sizes it asks for."""
import numpy as np
import pytest

from tests import clip_ref as cr
from tests import far_buffers as fb
from tests import wave_ref as wr
from tests import wavepack_ref as pr

pytestmark = pytest.mark.gpu

LINE = fb.LINE
PCM_FILL = 0xA5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture()
def meter(torch, pkg, request):
    m = fb.Meter(torch, request.node.name)
    yield m
    m.report()
    torch.cuda.empty_cache()
    pkg.trim()  # pooled handles would keep their gigabytes of scratch for the rest of the suite


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


class CycledDecode:
    """n packets cycling over `period` distinct ones (a synth batch with short and escaped packets among them), decoded into a
    dense sentinel-filled PCM buffer with 2 GiB of lead; the oracle's decode of the period next to it."""

    def __init__(self, torch, pkg, oracle, synth, cfg, n, period, seed):
        self.torch, self.cfg, self.n, self.period = torch, cfg, n, period
        fl = cfg.frame_length
        self.bpf = cfg.num_channels * oracle.bytes_per_sample(cfg.bit_depth)
        self.fbytes = fl * self.bpf
        b = synth.gen_batch(cfg, period, base_seed=seed, threads=16)
        packets = [b.packet(i) for i in range(b.n)]
        for j, k, esc in ((5, 1, True), (period // 3, fl // 2 - 1, False), (period // 2, fl, True), (period - 4, fl - 3, False),
                          (period - 1, 77, True)):
            packets[j] = cr.short_packet(synth, cfg, k, seed + j, escape=esc)
        sizes = np.array([len(p) for p in packets], np.uint32)
        offs = np.zeros(period, np.uint64)
        offs[1:] = np.cumsum(sizes[:-1])
        blob = np.frombuffer(b"".join(packets), np.uint8)
        self.ref = oracle.decode_batch(cfg, np.concatenate([blob, np.zeros(64, np.uint8)]), offs, sizes, threads=16)
        assert not self.ref[2].any() and (self.ref[1] < fl).sum() >= 4 and self.ref[0].shape[1] >= self.fbytes
        dev = torch.device("cuda:0")
        self.pick = torch.arange(n, device=dev) % period
        self.d_blob = to_dev(torch, blob)
        self.d_off = to_dev(torch, offs.astype(np.int64))[self.pick].contiguous()
        self.d_sz = to_dev(torch, sizes.astype(np.int32))[self.pick].contiguous()
        self.keep = (self.d_blob.clone(), self.d_off.clone(), self.d_sz.clone())
        self.pcm = fb.Far(torch, torch.uint8, n * self.fbytes + 64, PCM_FILL, lead=fb.BYTE_LEAD)
        self.d_fr = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
        assert n * self.fbytes > LINE and (LINE // self.fbytes) % period != 0

    def decode(self, dec, sync):
        self.torch.cuda.synchronize()
        dec.decode_batch_device(self.d_blob.data_ptr(), self.d_blob.numel(), self.d_off.data_ptr(), self.d_sz.data_ptr(), self.n,
                                self.pcm.ptr(), self.fbytes, self.d_fr.data_ptr(), self.d_st.data_ptr(), sync=sync)

    def check(self, what):
        torch, n = self.torch, self.n
        out, frames, status = self.ref
        want_fr = to_dev(torch, frames.view(np.int32))[self.pick]
        assert not bool(self.d_st.any()), "%s: packets %s have a status" % (what, torch.nonzero(self.d_st)[:8].flatten().tolist())
        assert torch.equal(self.d_fr, want_fr), "%s: frames differ at %s" % (what, torch.nonzero(self.d_fr != want_fr)[:8].flatten().tolist())
        # a period's slots as the decode must leave them: the oracle's frames, the sentinel behind a short packet's
        exp = np.where(np.arange(self.fbytes)[None, :] < (frames.astype(np.int64) * self.bpf)[:, None], out[:, :self.fbytes], np.uint8(PCM_FILL))
        fb.check_cycled(torch, self.pcm.at(0, n * self.fbytes).view(n, self.fbytes), to_dev(torch, exp), what)
        fb.assert_fill(torch, self.pcm.t[:self.pcm.lead], PCM_FILL, what + ": the 2 GiB in front of the PCM")
        fb.assert_fill(torch, self.pcm.t[self.pcm.lead + n * self.fbytes:], PCM_FILL, what + ": behind the PCM")
        assert torch.equal(self.d_blob, self.keep[0]) and torch.equal(self.d_off, self.keep[1]) and torch.equal(self.d_sz, self.keep[2])


def test_decode_16_bit_stereo_and_its_waveform_beyond_4_gib(torch, pkg, oracle, synth, meter):
    """2^18 + 2^15 + 77 = 294 989 packets of 4 096 frames, 16-bit stereo, cycling over 4 099 (MUSIC, with short and escaped
    packets among them): 4.5 GiB of dense PCM, slot 262 144 begins at byte 2^32. The decode's U scratch has 294 989 / 64 + 332 =
    4 942 one-MiB tiles, so the tiles from 4 096 on lie beyond the line too (4 589 wave slots are in use), and the batch runs in
    more than four rounds of four workgroups per CU on 256 CUs. Then, behind the decode with sync=False, alacgpu_waveform_device in STREAM / FLOAT: channel_stride is the
    least the entry takes, n * 4 096 elements = 4.5 GiB, so channel 1 lies wholly beyond the line and channel 0 crosses it;
    the wave is compared with the composition of torch ops of test_gpu_waveform.py's large batch, 8 192 packets at a time.

    2^32 / 16 384 = 2^18 = 3 887 mod 4 099: a decode whose slot offset wrapped would write slot 2^18 + j over slot j, which is
    packet j of the cycle and not packet j + 3 887, and leave the sentinel beyond the line; a U tile that wrapped would hand
    the predictor another wave's residuals, and the PCM of those packets differs from the oracle's. Peak device memory about
    21.5 GiB: 6.5 GiB PCM with its lead, 4.8 GiB U scratch, 9 GiB wave, 0.8 GiB of comparison."""
    fb._need_gb(torch, 24)
    fl, n = 4096, (1 << 18) + (1 << 15) + 77
    cfg = oracle.make_config(fl, 16, 2)
    cd = CycledDecode(torch, pkg, oracle, synth, cfg, n, 4099, 4)
    cs = n * fl
    wave = fb.Far(torch, torch.int32, 2 * cs + 8, wr.SENTINEL - (1 << 32), lead=4)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    with pkg.NewPacketDecoder(cr.to_pkg_cfg(pkg, cfg), 0) as dec:
        cd.decode(dec, sync=False)
        dec.waveform_device(cd.pcm.ptr(), cd.fbytes, cd.d_fr.data_ptr(), cd.d_st.data_ptr(), n, wr.STREAM, wr.FLOAT, wave.ptr(), cs, 0,
                            d_starts.data_ptr(), sync=True)
        meter.mark()
        d = dec.last_dispatch()
        # wave slots of 64 packets, one U tile each: the tiles from 4 096 on are in use, and more than four rounds of four per CU
        assert d["narrow_slots"] > 4096 and (n_cu > 256 or d["narrow_slots"] > 4 * 4 * n_cu), d
    cd.check("16-bit stereo")
    want_starts = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.cumsum(cd.d_fr.to(torch.int64), 0)])
    assert torch.equal(d_starts, want_starts)
    total = int(d_starts[n].item())
    assert LINE // 4 < total < cs
    step = 8192
    at = d_starts[::step].cpu().tolist() + [total]
    cols = torch.arange(fl, device="cuda:0")[None, :]
    for k, a in enumerate(range(0, n, step)):
        m = min(step, n - a)
        keep = cols < cd.d_fr[a:a + m, None]
        comp = (cd.pcm.at(a * cd.fbytes, m * cd.fbytes).view(torch.int16).view(m, fl, 2)[keep].to(torch.float32) * (2.0 ** -15)).t().contiguous()
        lo, hi = at[k], at[k + 1] if a + m < n else total
        assert comp.shape[1] == hi - lo
        for c in (0, 1):
            assert torch.equal(wave.at(c * cs + lo, hi - lo), comp[c].view(torch.int32)), \
                "channel %d differs from the torch composition among the packets %d .. %d" % (c, a, a + m)
        del keep, comp
    meter.mark()
    for c in (0, 1):
        fb.assert_fill(torch, wave.at(c * cs + total, cs - total), wave.fill, "behind channel %d" % c)
    fb.assert_fill(torch, wave.t[:wave.lead], wave.fill, "in front of the wave")
    fb.assert_fill(torch, wave.t[wave.lead + 2 * cs:], wave.fill, "behind the wave")


def test_decode_24_bit_stereo_beyond_4_gib(torch, pkg, oracle, synth, meter):
    """180 224 + 77 packets of 4 096 frames, 24-bit stereo, cycling over 4 099: 4.13 GiB of PCM through the 3-byte writer; slot
    174 762 straddles byte 2^32 (24 576 does not divide it). floor(2^32 / 24 576) = 174 762 = 2 604 mod 4 099: a slot offset
    that wrapped puts packet 174 763 + j's PCM 8 192 bytes into slot j, and leaves the sentinel beyond the line. Peak device
    memory about 10 GiB: 6.1 GiB PCM with its lead, 3.4 GiB U scratch."""
    fb._need_gb(torch, 12)
    n = 180224 + 77
    cfg = oracle.make_config(4096, 24, 2)
    cd = CycledDecode(torch, pkg, oracle, synth, cfg, n, 4099, 24)
    with pkg.NewPacketDecoder(cr.to_pkg_cfg(pkg, cfg), 0) as dec:
        cd.decode(dec, sync=True)
        meter.mark()
        d = dec.last_dispatch()
        assert d["narrow_kernel"] == "alac_decode_24q" and d["narrow_slots"] > 0, d
    cd.check("24-bit stereo")


def test_decode_24_bit_8_channels_beyond_4_gib(torch, pkg, oracle, synth, meter):
    """45 056 + 77 packets of 4 096 frames, 24-bit, 8 channels, cycling over 1 031: the split pipeline's rows (n * 8 channels *
    4 096 int32 = 5.5 GiB) and the PCM (4.13 GiB) both cross the line, cd / keys2 / perm2 hold n * 8 entries. Rows of packet
    32 768 on lie beyond 2^32 bytes (2^32 / 131 072 = 2^15 = 807 mod 1 031), PCM slots from 43 690 on (43 690 = 388 mod 1 031):
    a row or slot offset that wrapped interleaves another class's samples or writes them into a low slot. Peak device memory
    about 14 GiB: 6.1 GiB PCM with its lead, 5.5 GiB rows, 1.3 GiB U scratch and the descriptors."""
    fb._need_gb(torch, 16)
    n = 45056 + 77
    cfg = oracle.make_config(4096, 24, 8)
    cd = CycledDecode(torch, pkg, oracle, synth, cfg, n, 1031, 8)
    assert n * 8 * 4096 * 4 > LINE
    with pkg.NewPacketDecoder(cr.to_pkg_cfg(pkg, cfg), 0) as dec:
        cd.decode(dec, sync=True)
        meter.mark()
        d = dec.last_dispatch()
        assert "alac_interleave4" in d["irregular_kernels"] and d["narrow_slots"] == 0, d
    cd.check("24-bit 8 channels")


@pytest.fixture(scope="module")
def enc_sim():
    from tests.test_encoder_host import EncSim
    return EncSim()


@pytest.mark.parametrize("profile", ["music", "noise"])
def test_encode_16_bit_stereo_beyond_4_gib(torch, pkg, oracle, synth, enc_sim, meter, profile):
    """2^18 + 4 099 = 266 243 packets of 4 096 frames, 16-bit stereo, through test_gpu_encoder_edges.py's _check_cycled_batch: the
    PCM cycles through 7 packets' worth of synth's MUSIC or NOISE signal, the expectation is the host build's (EncSim) 7
    packets, the offsets are held to their closed form and the blob to its period. 4.06 GiB of PCM go in: packet 2^18 begins at
    input byte 2^32, and 2^18 = 1 mod 7, so an input offset that wrapped encodes class j % 7 where (j + 1) % 7 belongs. NOISE:
    every packet escapes (16 388 bytes), so the blob is 4.06 GiB as well and offsets[] pass 2^32 from packet 262 081 on; a blob
    offset that wrapped leaves the 0xAB sentinel there, and an offsets[i] narrowed to 32 bits breaks the closed form. Peak
    device memory 8.2 GiB: the PCM and the blob's capacity, 4.06 GiB each."""
    from tests.test_gpu_encoder_edges import _check_cycled_batch
    fb._need_gb(torch, 24)
    fl, n = 4096, (1 << 18) + 4099
    assert (1 << 18) % 7 == 1
    ocfg = oracle.make_config(fl, 16, 2)
    prof = synth.PROFILE_MUSIC if profile == "music" else synth.PROFILE_NOISE
    pcm = np.concatenate([synth.signal(ocfg, prof, 100 + k, fl) for k in range(7)])
    pcm[::fl, 0] = [0, 1, -1, 77, -300, 32767, -32768]  # a different first sample: 7 distinct packets whatever the signal
    pcm7 = synth.pack_pcm(ocfg, pcm)
    blob7, off7, _ = enc_sim.encode(ocfg, pcm7, 7 * fl)
    sizes7 = np.diff(off7).astype(np.int64)
    assert len({blob7[int(off7[k]):int(off7[k + 1])].tobytes() for k in range(7)}) == 7
    if profile == "noise":
        assert (sizes7 == sizes7[0]).all() and sizes7[0] > fl * 4 and n * int(sizes7[0]) > LINE, sizes7
    else:
        assert sizes7.max() < fl * 4 * 3 // 4, sizes7
    assert n * fl * 4 > LINE
    _check_cycled_batch(torch, pkg, ocfg, n, pcm7, blob7, sizes7)
    meter.mark()


def test_pack_pass_dense_beyond_4_gib(torch, pkg, meter):
    """alacgpu_pcm_from_waveform_device, depth 32, 8 channels, STREAM / INT, 2^27 + 4 099 frames: 4 GiB of int32 waveform in
    (channel_stride = the frames, so the channels 1 .. 7 begin at multiples of 512 MiB + 16 396 bytes and channel 7 ends beyond
    the line) and 4 GiB of dense PCM out, 32 bytes a frame, frame 2^27 at output byte 2^32. Every channel repeats 4 099 random
    integers, so the PCM cycles over 4 099 frames and is wavepack_ref's on one period; clipped is 0, INT at depth 32 clips
    nothing.

    2^27 = 2 635 mod 4 099 and 2^30 = 585 mod 4 099: an output offset that wrapped writes frame 2^27 + j over frame j, whose
    class differs, and leaves the sentinel beyond the line; an input offset that wrapped reads channel c's frame t from 2^30
    elements lower, another channel's frame of another class. Peak device memory about 10.5 GiB: 4 GiB wave, 6 GiB PCM with its
    lead, 0.5 GiB to build the wave."""
    fb._need_gb(torch, 12)
    ch, P = 8, 4099
    total = (1 << 27) + P
    rng = np.random.default_rng(27)
    blk = rng.integers(-(1 << 31), 1 << 31, (ch, P), dtype=np.int64).astype(np.int32)
    want, clipped = pr.pack_ref(blk, 32, pr.INT)
    assert clipped == 0 and want.size == P * 32 and (1 << 27) % P != 0 and (1 << 30) % P != 0
    d_blk = to_dev(torch, blk)
    wave = fb.Far(torch, torch.int32, ch * total + 8, pr.WAVE_SENTINEL, lead=4)
    reps = -(-total // P)
    for c in range(ch):
        wave.at(c * total, total).copy_(d_blk[c].repeat(reps)[:total])
    pcm = fb.Far(torch, torch.uint8, total * 32 + 64, pr.PCM_SENTINEL, lead=fb.BYTE_LEAD)
    d_clip = torch.full((1,), 0xDEAD, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    with pkg.NewPacketEncoder(pkg.PacketConfig(FrameLength=4096, BitDepth=32, NumChannels=ch)) as enc:
        enc.pcm_from_waveform_device(wave.ptr(), pr.STREAM, pr.INT, total, 0, total, pcm.ptr(), d_clip.data_ptr(), sync=True)
        meter.mark()
    fb.check_cycled(torch, pcm.at(0, total * 32).view(total, 32), to_dev(torch, want).view(P, 32), "dense PCM", unit="frame")
    assert int(d_clip.item()) == 0
    fb.assert_fill(torch, pcm.t[:pcm.lead], pr.PCM_SENTINEL, "the 2 GiB in front of the PCM")
    fb.assert_fill(torch, pcm.t[pcm.lead + total * 32:], pr.PCM_SENTINEL, "behind the PCM")
    for c in range(ch):  # the waveform is unchanged
        fb.check_cycled(torch, wave.at(c * total, (total // P) * P).view(total // P, P), d_blk[c][None, :], "channel %d afterwards" % c,
                        unit="period")
        assert torch.equal(wave.at(c * total + (total // P) * P, total % P), d_blk[c][:total % P])
    fb.assert_fill(torch, wave.t[:wave.lead], pr.WAVE_SENTINEL, "in front of the wave")
    fb.assert_fill(torch, wave.t[wave.lead + ch * total:], pr.WAVE_SENTINEL, "behind the wave")
