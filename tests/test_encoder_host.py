"""The batch encoder's logic on the CPU: csrc/alac_enc.h built with g++ (tests/host_sim/enc_sim.cpp), stage for stage what the
gfx950 kernels of k_enc.hip run.

* round trip through the oracle to the identical PCM over bit depths, channel counts, frame lengths, short last packets,
  long zero runs, and MUSIC / NOISE / QUIET signals;
* the bit-exact pin: every packet equals what synth.encode_packet makes from the parameters its own header carries;
* the compression bar: no larger than synth's WARM order 8 / mixRes 2 packets of the same PCM;
* the cookie parses back to the encoder's config."""
import ctypes

import numpy as np
import pytest

from tests import host_build

BPS = {16: 2, 20: 3, 24: 3, 32: 4}
SHIFT = {16: 0, 20: 0, 24: 1, 32: 2}


def build_enc_sim():
    L = host_build.shared("enc_sim.cpp", "libenc_sim.so", host_build.SIM + ["-pthread"])
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.enc_sim_max_bytes.restype = u64
    L.enc_sim_max_bytes.argtypes = [vp, u64]
    L.enc_sim_cookie.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp]
    L.enc_sim_encode.restype = ctypes.c_long
    L.enc_sim_encode.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, ctypes.c_int]
    return L


class EncSim:
    def __init__(self):
        self.L = build_enc_sim()

    def encode(self, cfg, pcm_bytes, total_frames, threads=8, want_starts=False):
        """-> (blob uint8, offsets uint64[n + 1], escaped uint32[n]) [+ element header bit positions uint64[n, 5]]"""
        pcm = np.frombuffer(bytes(pcm_bytes) or b"\0", np.uint8)
        cap = int(self.L.enc_sim_max_bytes(ctypes.byref(cfg), total_frames))
        fl = cfg.frame_length
        n = (total_frames + fl - 1) // fl
        blob = np.zeros(max(cap, 1), np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        esc = np.zeros(max(n, 1), np.uint32)
        starts = np.zeros((max(n, 1), 5), np.uint64)
        got = self.L.enc_sim_encode(ctypes.byref(cfg), pcm.ctypes.data, total_frames, blob.ctypes.data, cap,
                                    offsets.ctypes.data, esc.ctypes.data, starts.ctypes.data, threads)
        assert got == n
        if want_starts:
            return blob[:int(offsets[-1])].copy(), offsets, esc[:n], starts[:n]
        return blob[:int(offsets[-1])].copy(), offsets, esc[:n]

    def cookie(self, cfg, max_frame_bytes, avg_bit_rate):
        out = (ctypes.c_uint8 * 24)()
        self.L.enc_sim_cookie(ctypes.byref(cfg), max_frame_bytes, avg_bit_rate, out)
        return bytes(out)


@pytest.fixture(scope="module")
def enc_sim():
    return EncSim()


def make_pcm(synth, cfg, profile, total_frames, seed=7):
    """Interleaved int32 [frames][channels] in the PCM domain of the depth, made of synth's seeded signal source in pieces
    of frame_length (so the signal changes at packet boundaries like a real stream does not, which costs nothing here)."""
    fl = max(cfg.frame_length, 1)
    parts, done, k = [], 0, 0
    while done < total_frames:
        m = min(4096 if fl > 4096 else fl, total_frames - done)
        parts.append(synth.signal(cfg, profile, seed * 1000003 + k, m))
        done += m
        k += 1
    return np.concatenate(parts) if parts else np.zeros((0, cfg.num_channels), np.int32)


def oracle_round_trip(oracle, cfg, blob, offsets, pcm_bytes, total_frames):
    n = len(offsets) - 1
    sizes = np.diff(offsets).astype(np.uint32)
    buf = np.concatenate([blob, np.zeros(64, np.uint8)])
    out, frames, status = oracle.decode_batch(cfg, buf, offsets[:-1], sizes, threads=8)
    assert not status.any(), "oracle rejects packet %s" % np.nonzero(status)[0][:8]
    fl = cfg.frame_length
    expect = [min(fl, total_frames - i * fl) for i in range(n)]
    assert frames.tolist() == expect
    bpf = cfg.num_channels * BPS[cfg.bit_depth]
    got = b"".join(out[i, :int(frames[i]) * bpf].tobytes() for i in range(n))
    assert got == pcm_bytes


def header_elem(synth, cfg, packet, bitpos):
    """The parameters the element header at bit `bitpos` of a packet carries (decoder.go:210-235, :267-293, :348-376), as a
    synth Elem: COEF_GIVEN with the header's coefficients, the escape flag as force_escape / never_escape."""
    bits = np.unpackbits(np.frombuffer(packet, np.uint8))

    class R:
        pos = bitpos

    def get(n):
        v = 0
        for _ in range(n):
            v = (v << 1) | int(bits[R.pos])
            R.pos += 1
        return v

    tag = get(3)
    get(4)
    assert get(12) == 0
    flags = get(4)
    partial, bs, esc = flags >> 3, (flags >> 1) & 3, flags & 1
    if partial:
        get(32)
    if esc:
        el = synth.default_elem(order=8, mix_res=2, bytes_shifted=SHIFT[cfg.bit_depth], force_escape=1)
    else:
        mix_bits, mix_res = get(8), get(8)
        kw = dict(mix_bits=mix_bits, mix_res=mix_res if mix_res < 128 else mix_res - 256, bytes_shifted=bs,
                  never_escape=1, coef_mode=synth.COEF_GIVEN)
        for name in ("u", "v")[:2 if tag == 1 else 1]:
            mode, den, pbf, order = get(4), get(4), get(3), get(5)
            kw.update({"mode_" + name: mode, "den_shift": den, "pb_factor": pbf, "order_" + name: order})
            kw["coefs_" + name] = [c - 65536 if c >= 32768 else c for c in (get(16) for _ in range(order))]
        el = synth.default_elem(**kw)
    el.partial = partial
    return el


MATRIX = [(d, ch, fl) for d in (16, 20, 24, 32) for ch in (1, 2, 3, 6, 8) for fl in (4096, 4095, 1)]


@pytest.mark.parametrize("depth,ch,fl", MATRIX)
def test_round_trip_through_the_oracle(enc_sim, synth, oracle, depth, ch, fl):
    cfg = oracle.make_config(fl, depth, ch)
    total = {4096: 3 * 4096 + 1000, 4095: 2 * 4095 + 17, 1: 37}[fl]
    pcm = make_pcm(synth, cfg, synth.PROFILE_MUSIC, total, seed=depth * 10 + ch)
    pcm_bytes = synth.pack_pcm(cfg, pcm)
    blob, offsets, _ = enc_sim.encode(cfg, pcm_bytes, total)
    oracle_round_trip(oracle, cfg, blob, offsets, pcm_bytes, total)
    # only the last packet is short, and only it carries the partial flag (flags of the first element header, bits 19..22)
    n = len(offsets) - 1
    assert n == -(-total // fl)
    for i in range(n):
        pkt = blob[int(offsets[i]):int(offsets[i + 1])].tobytes()
        short = i == n - 1 and total % fl != 0
        assert (int.from_bytes(pkt[:3], "big") >> 1) & 8 == (8 if short else 0), "packet %d" % i


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
@pytest.mark.parametrize("profile", ["NOISE", "QUIET"])
def test_noise_escapes_and_quiet_runs(enc_sim, synth, oracle, depth, profile):
    cfg = oracle.make_config(4096, depth, 2)
    total = 4 * 4096 - 5
    pcm = make_pcm(synth, cfg, getattr(synth, "PROFILE_" + profile), total, seed=3)
    pcm_bytes = synth.pack_pcm(cfg, pcm)
    blob, offsets, esc = enc_sim.encode(cfg, pcm_bytes, total)
    oracle_round_trip(oracle, cfg, blob, offsets, pcm_bytes, total)
    raw = total * 2 * BPS[depth]
    if profile == "NOISE":
        assert esc.all(), "full-scale noise must go out raw"
    else:
        # a third of the signal is silent stretches of 97 frames, which go out as zero runs; the rest is a few bits a sample
        # above the shift block
        assert not esc.any() and len(blob) < raw * (8 * SHIFT[depth] + 6) // depth, "quiet signal must compress well"


def test_long_silent_mono_packet_caps_the_zero_run(enc_sim, synth, oracle):
    cfg = oracle.make_config(70000, 16, 1)
    pcm = np.zeros((70000, 1), np.int32)
    pcm[0, 0] = 5
    pcm_bytes = synth.pack_pcm(cfg, pcm)
    blob, offsets, esc = enc_sim.encode(cfg, pcm_bytes, 70000)
    assert not esc.any()
    # 65 535 zeros in one run code, then the rest: a few bytes beyond the header
    assert len(blob) < 80
    oracle_round_trip(oracle, cfg, blob, offsets, pcm_bytes, 70000)
    # the same packet from synth's writer (WARM, order 8, mixRes 2): byte for byte
    el = synth.default_elem(order=8, mix_res=2, never_escape=1)
    assert synth.encode_packet(cfg, [el], pcm) == blob.tobytes()


def test_total_frames_not_a_multiple_of_the_frame_length(enc_sim, synth, oracle):
    cfg = oracle.make_config(1000, 24, 2)
    total = 5 * 1000 + 1
    pcm = make_pcm(synth, cfg, synth.PROFILE_MUSIC, total)
    pcm_bytes = synth.pack_pcm(cfg, pcm)
    blob, offsets, _ = enc_sim.encode(cfg, pcm_bytes, total)
    assert len(offsets) == 7
    oracle_round_trip(oracle, cfg, blob, offsets, pcm_bytes, total)
    # partial flag only on the last packet
    for i in range(6):
        pkt = blob[int(offsets[i]):int(offsets[i + 1])].tobytes()
        assert (int.from_bytes(pkt[:3], "big") >> 1) & 8 == (8 if i == 5 else 0)  # the partial flag of the first element


def test_low_bits_of_20_bit_samples_are_ignored(enc_sim, synth, oracle):
    cfg = oracle.make_config(4096, 20, 2)
    pcm = make_pcm(synth, cfg, synth.PROFILE_MUSIC, 4096)
    pcm_bytes = bytearray(synth.pack_pcm(cfg, pcm))
    clean, off1, _ = enc_sim.encode(cfg, bytes(pcm_bytes), 4096)
    for i in range(0, len(pcm_bytes), 3):
        pcm_bytes[i] |= 0x0B
    dirty, off2, _ = enc_sim.encode(cfg, bytes(pcm_bytes), 4096)
    assert np.array_equal(clean, dirty) and np.array_equal(off1, off2)


@pytest.mark.parametrize("depth,ch,profile", [(16, 2, "MUSIC"), (24, 2, "MUSIC"), (20, 3, "MUSIC"), (32, 6, "MUSIC"),
                                              (16, 8, "QUIET"), (24, 2, "NOISE"), (16, 1, "MUSIC"), (32, 2, "QUIET")])
def test_packets_equal_synth_with_their_header_parameters(enc_sim, synth, oracle, depth, ch, profile):
    """The bit-exact pin: whatever policy chose the parameters, the Golomb writer, the shift block and the header fields are
    synth's (alac_synth_encode_packet with COEF_GIVEN and the header's escape flag)."""
    cfg = oracle.make_config(4096, depth, ch)
    total = 3 * 4096 + 333
    pcm = make_pcm(synth, cfg, getattr(synth, "PROFILE_" + profile), total, seed=11)
    pcm_bytes = synth.pack_pcm(cfg, pcm)
    blob, offsets, esc, starts = enc_sim.encode(cfg, pcm_bytes, total, want_starts=True)
    ne = synth.num_elements(ch)
    for i in range(len(offsets) - 1):
        pkt = blob[int(offsets[i]):int(offsets[i + 1])].tobytes()
        elems = [header_elem(synth, cfg, pkt, int(starts[i, e])) for e in range(ne)]
        assert all(bool(el.force_escape) == bool(esc[i] >> e & 1) for e, el in enumerate(elems))
        ref = synth.encode_packet(cfg, elems, pcm[i * 4096:(i + 1) * 4096])
        assert ref == pkt, "packet %d differs from synth with its header's parameters" % i


def _full_music_packets(synth, cfg, n=1024):
    b = synth.gen_batch(cfg, n, threads=8)
    keep = [i for i in range(n) if int(b.frames[i]) == cfg.frame_length]
    bpf = cfg.num_channels * BPS[cfg.bit_depth]
    rows = b.pcm[keep, :cfg.frame_length * bpf]
    return keep, rows


@pytest.mark.parametrize("depth", [16, 24])
def test_compression_bar_against_synth_warm_order8(enc_sim, synth, oracle, depth):
    """The full-length packets of gen_batch(cfg, 1024) (MUSIC, default seed), concatenated: the encoder's bytes are no more
    than synth's WARM packets with order 8 / mixRes 2 over the same 4096-frame slices."""
    cfg = oracle.make_config(4096, depth, 2)
    keep, rows = _full_music_packets(synth, cfg)
    assert 990 <= len(keep) < 1024
    stream = rows.tobytes()
    total = len(keep) * 4096
    blob, offsets, _ = enc_sim.encode(cfg, stream, total)
    assert len(offsets) - 1 == len(keep)
    ref = 0
    bs = SHIFT[depth]
    for k in range(len(keep)):
        pcm = np.frombuffer(rows[k].tobytes(), np.uint8)
        if depth == 16:
            v = pcm.view("<i2").astype(np.int32)
        else:
            w = pcm.reshape(-1, 3).astype(np.int32)
            v = ((w[:, 0] << 8) | (w[:, 1] << 16) | (w[:, 2] << 24)) >> 8
        el = synth.default_elem(order=8, mix_res=2, bytes_shifted=bs)
        ref += len(synth.encode_packet(cfg, [el], v.reshape(-1, 2)))
    got = int(offsets[-1])
    print("depth %d: encoder %d bytes (%.4f of raw), synth WARM order 8 %d" % (depth, got, got / len(stream), ref))
    assert got <= ref
    oracle_round_trip(oracle, cfg, blob, offsets, stream, total)


def test_cookie_parses_back_to_the_config(enc_sim, pkg, oracle):
    cfg = oracle.make_config(4095, 24, 6, pb=40, mb=10, kb=14, max_run=255, sample_rate=96000)
    c = enc_sim.cookie(cfg, 123456, 987654)
    assert len(c) == 24
    back = pkg.ParseMagicCookie(c)
    assert (back.FrameLength, back.BitDepth, back.NumChannels, back.PB, back.MB, back.KB, back.MaxRun, back.SampleRate) == \
        (4095, 24, 6, 40, 10, 14, 255, 96000)
    assert back.MaxFrameBytes == 123456 and back.AvgBitRate == 987654


def test_encoder_rejects_bad_configs_before_the_gpu(pkg):
    """alacgpu_encoder_create rejects what alacgpu_create rejects, before any HIP call (no GPU needed)."""
    pkg.build()
    for kw in ({"BitDepth": 13}, {"NumChannels": 0}, {"NumChannels": 9}, {"FrameLength": 0}, {"FrameLength": (1 << 24) + 1}):
        with pytest.raises(pkg.ErrConfig):
            pkg.NewPacketEncoder(pkg.PacketConfig(**kw))


# PB / MB / KB at the ends of their bytes: KB 0 leaves only escaped elements (alac_enc.h: encode_chain), PB > 127 makes some
# zero runs unencodable (escaped too); everything else is the regular path with extreme Golomb parameters
COOKIE_PARAMS = [(0, 10, 14), (255, 10, 14), (40, 0, 14), (40, 255, 14), (40, 10, 0), (40, 10, 1), (40, 10, 31),
                 (40, 10, 32), (40, 10, 255), (4, 10, 0), (255, 255, 255), (0, 0, 0), (128, 0, 1)]


@pytest.mark.parametrize("pb,mb,kb", COOKIE_PARAMS)
@pytest.mark.parametrize("depth,ch,profile", [(16, 1, "QUIET"), (24, 2, "MUSIC"), (32, 1, "MUSIC"), (20, 3, "QUIET")])
def test_round_trip_over_cookie_parameter_extremes(enc_sim, synth, oracle, pb, mb, kb, depth, ch, profile):
    cfg = oracle.make_config(4096, depth, ch, pb=pb, mb=mb, kb=kb)
    total = 2 * 4096 + 17
    pcm = make_pcm(synth, cfg, getattr(synth, "PROFILE_" + profile), total, seed=pb + mb + kb)
    pcm_bytes = synth.pack_pcm(cfg, pcm)
    blob, offsets, esc, starts = enc_sim.encode(cfg, pcm_bytes, total, want_starts=True)
    oracle_round_trip(oracle, cfg, blob, offsets, pcm_bytes, total)
    ne = synth.num_elements(ch)
    if kb == 0:
        assert all(int(e) == (1 << ne) - 1 for e in esc), "KB 0: every element must go out raw"
    elif pb <= 127 and depth == 16 and profile == "QUIET":  # residuals of +-3: compressed whatever the Golomb parameters
        assert not any(esc), "the regular path must be exercised"
    for i in range(len(offsets) - 1):  # and the pin holds for these parameters as well
        pkt = blob[int(offsets[i]):int(offsets[i + 1])].tobytes()
        elems = [header_elem(synth, cfg, pkt, int(starts[i, e])) for e in range(ne)]
        assert synth.encode_packet(cfg, elems, pcm[i * 4096:(i + 1) * 4096]) == pkt, "packet %d" % i
