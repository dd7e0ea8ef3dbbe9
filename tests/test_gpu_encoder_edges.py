"""Edge-case PCM (tests/edge_pcm.py) through the encoder and decoder kernels on the MI355X, and the device-entry contracts of
alacgpu_encode_device that no other test pins.

(a) Every signal: the GPU's packets equal the host build of the encoder (enc_sim, which test_encoder_edges.py checks against
    the oracle, synth's writer and goref's trace), and the GPU decoder, fed with the encoder's offsets and d_sizes = NULL,
    gives back the source PCM, the frame counts and status 0 — over the decode routes on purpose: the wave pairs of regular
    packets up to 65 536 frames (default, ALACGPU_LANES_MIN=3, ALACGPU_PPW=64), the scan route of longer packets and of more
    than two channels, and the whole-packet walker (PB above 73). Which route ran is asserted from last_dispatch() and from
    lane_sim's classes of the same packets.
(b) Misaligned d_pcm / d_blob with sentinels around the blob, sync = 0 encodes back to back while the scratch regrows, the
    ordering contract with work queued on the handle's stream, the cookie's "so far" counters and a zero-frame encode, and
    batches that need two launches of alac_enc_chains and of alac_enc_pack (k_enc.hip: kChainsPerLaunch, kPacketsPerPack)."""
import importlib

import numpy as np
import pytest

from tests import edge_pcm
from tests.far_buffers import _need_gb
from tests.test_encoder_host import BPS, EncSim, make_pcm, oracle_round_trip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc_sim():
    return EncSim()


@pytest.fixture(scope="module")
def torch(pkg):
    t = importlib.import_module("torch")
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    pkg.build()
    return t


def pkg_cfg(pkg, ocfg):
    return pkg.PacketConfig(FrameLength=ocfg.frame_length, BitDepth=ocfg.bit_depth, NumChannels=ocfg.num_channels,
                            PB=ocfg.pb, MB=ocfg.mb, KB=ocfg.kb, MaxRun=ocfg.max_run, SampleRate=ocfg.sample_rate)


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def gpu_encode(torch, enc, pcm_bytes, frames):
    cap = enc.max_bytes(frames)
    fl = enc.config.FrameLength
    n = (frames + fl - 1) // fl
    d_pcm = to_dev(torch, np.frombuffer(pcm_bytes or b"\0", np.uint8).copy())
    d_blob = torch.zeros(max(cap, 1), dtype=torch.uint8, device="cuda:0")
    d_off = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    enc.encode_device(d_pcm.data_ptr(), frames, d_blob.data_ptr(), cap, d_off.data_ptr(), sync=True)
    return d_blob, d_off


def gpu_decode(torch, pkg, cfg, d_blob, d_off):
    """-> (out [n, stride] on the device, frames, status, last_dispatch())"""
    n = d_off.numel() - 1
    stride = cfg.FrameLength * cfg.NumChannels * BPS[cfg.BitDepth]
    d_out = torch.zeros((n, stride), dtype=torch.uint8, device="cuda:0")
    d_fr = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    blob_bytes = int(d_off[-1].item())
    with pkg.NewPacketDecoder(cfg, 0) as dec:
        dec.decode_batch_device(d_blob.data_ptr(), blob_bytes, d_off.data_ptr(), None, n, d_out.data_ptr(), stride,
                                d_fr.data_ptr(), d_st.data_ptr(), sync=True)
        disp = dec.last_dispatch()
    return d_out, d_fr.cpu().numpy(), d_st.cpu().numpy(), disp


# name, depth, channels, frame length, packets, PB, environment, the route every packet takes
EDGE_CASES = [
    ("silence", 16, 2, 4096, 300, 40, {}, "regular"),
    ("dual_mono", 16, 2, 4096, 300, 40, {}, "regular"),
    ("bursts", 16, 2, 4096, 300, 40, {}, "regular"),
    ("bursts", 16, 1, 4096, 300, 40, {}, "regular"),
    ("dual_mono", 24, 2, 4096, 300, 40, {"ALACGPU_LANES_MIN": "3"}, "regular"),
    ("bursts", 16, 2, 4096, 300, 40, {"ALACGPU_LANES_MIN": "3"}, "regular"),
    ("click_last", 16, 2, 4096, 300, 40, {"ALACGPU_PPW": "64"}, "regular"),
    ("dual_mono", 16, 2, 4096, 300, 40, {"ALACGPU_PPW": "64"}, "regular"),
    ("silence", 16, 2, 65536, 64, 40, {}, "regular"),
    ("silence", 16, 1, 65536, 64, 40, {}, "regular"),
    ("click_first", 16, 2, 65536, 64, 40, {}, "regular"),
    ("dual_mono", 16, 2, 65536, 64, 40, {}, "regular"),
    ("bursts", 16, 2, 65536, 64, 40, {}, "regular"),
    ("silence", 24, 2, 65536, 64, 40, {}, "scan"),  # shift bytes and a few bytes of entropy stream: classify_regular
    ("run_ladder", 16, 1, edge_pcm.LADDER_FL, 14, 40, {}, "scan"),
    ("run_ladder", 16, 2, edge_pcm.LADDER_FL, 14, 40, {}, "scan"),
    ("silence", 16, 2, 65537, 16, 40, {}, "scan"),
    ("bursts", 16, 8, 4096, 200, 40, {}, "scan"),
    ("antiphase_full", 24, 6, 4096, 100, 40, {}, "scan"),
    ("silence", 16, 8, 4096, 100, 40, {}, "scan"),
    ("silence", 16, 2, 4096, 300, 100, {}, "walker"),
    ("bursts", 16, 2, 4096, 300, 100, {}, "walker"),
    ("antiphase_full", 16, 2, 4096, 100, 127, {}, "walker"),
    ("run_ladder", 16, 2, edge_pcm.LADDER_FL, 7, 74, {}, "walker"),
    ("run_ladder", 16, 1, edge_pcm.LADDER_FL, 7, 100, {}, "walker"),
]


@pytest.mark.parametrize("name,depth,ch,fl,n,pb,env,route", EDGE_CASES)
def test_gpu_edge_signals_both_directions(pkg, torch, synth, oracle, lane_sim, enc_sim, monkeypatch, name, depth, ch, fl, n, pb,
                                          env, route):
    for k in ("ALACGPU_LANES_MIN", "ALACGPU_PPW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():  # read when a decoder handle is made
        monkeypatch.setenv(k, v)
    ocfg = oracle.make_config(fl, depth, ch, pb=pb)
    total = n * fl - (3 if n > 1 else 0)  # a short last packet
    pcm_bytes = synth.pack_pcm(ocfg, edge_pcm.make(name, synth, ocfg, total))
    ref_blob, ref_off, _ = enc_sim.encode(ocfg, pcm_bytes, total)
    oracle_round_trip(oracle, ocfg, ref_blob, ref_off, pcm_bytes, total)
    cfg = pkg_cfg(pkg, ocfg)
    with pkg.NewPacketEncoder(cfg) as enc:
        d_blob, d_off = gpu_encode(torch, enc, pcm_bytes, total)
    off = d_off.cpu().numpy().astype(np.uint64)
    assert np.array_equal(off, ref_off)
    assert np.array_equal(d_blob[:int(off[-1])].cpu().numpy(), ref_blob), "GPU encoder differs from the host build"

    d_out, fr, st, disp = gpu_decode(torch, pkg, cfg, d_blob, d_off)
    assert not st.any(), "GPU decoder rejects packets %s" % np.nonzero(st)[0][:8]
    assert fr.tolist() == [min(fl, total - i * fl) for i in range(n)]
    bpf = ch * BPS[depth]
    want = np.frombuffer(pcm_bytes, np.uint8)
    full = total // fl
    w = to_dev(torch, want[:full * fl * bpf].copy()).view(full, fl * bpf)
    assert torch.equal(d_out[:full], w), "PCM differs from the source"
    if n > full:
        assert np.array_equal(d_out[full, :(total - full * fl) * bpf].cpu().numpy(), want[full * fl * bpf:])

    # the route: lane_sim's classes of the same packets, and what the device dispatched
    sizes = np.diff(ref_off).astype(np.uint32)
    classes = lane_sim(ocfg, ref_blob, ref_off[:-1].copy(), sizes, want_classes=True)[3]
    irr = disp["irregular_kernels"]
    if route == "regular":
        assert (classes < 2048).all() and disp["irregular_slots"] == 0 and disp["narrow_kernel"], disp
        if "ALACGPU_PPW" in env:
            assert disp["packets_per_slot"] == int(env["ALACGPU_PPW"]), disp
    elif route == "scan":
        assert (classes >= 2048).all() and disp["irregular_slots"] > 0 and irr.startswith("alac_scan +"), disp
        if ch > 2:
            assert "alac_chan_predict" in irr, disp
    else:  # PB > 73 is not a lean config: classify_regular sends every packet to the whole-packet decoder
        assert disp["irregular_slots"] == disp["slots"] > 0 and irr == "alac_scan (whole-packet decoder)", disp
    print("%s %d-bit %dch fl %d x %d PB %d %s: %s | %s" % (name, depth, ch, fl, n, pb, env, disp["narrow_kernel"], irr))


# ---- device-entry contracts ---------------------------------------------------------------------------------------------
def _music(synth, oracle, fl, depth, ch, total, seed):
    ocfg = oracle.make_config(fl, depth, ch)
    return ocfg, synth.pack_pcm(ocfg, make_pcm(synth, ocfg, synth.PROFILE_MUSIC, total, seed=seed))


@pytest.mark.parametrize("pcm_shift", [0, 1, 2, 3])
def test_gpu_misaligned_pcm_and_blob(pkg, torch, synth, oracle, enc_sim, pcm_shift):
    """d_pcm and d_blob at byte offsets 0..3 inside larger allocations: the bytes are the aligned encode's; the 0xAB bytes in
    front of d_blob and from d_blob + offsets[n] to the end of the allocation stay as they were (alac_enc_pack stores whole
    dwords of the absolute address space and bytes only at a packet's two ends)."""
    ocfg, pcm_bytes = _music(synth, oracle, 1000, 24, 2, 37 * 1000 + 5, seed=pcm_shift + 3)
    ocfg2 = oracle.make_config(1000, 24, 2)
    silent = synth.pack_pcm(ocfg2, edge_pcm.silence(synth, ocfg2, 3 * 1000 + 1))
    pcm_bytes += silent  # tiny packets at the end: both of a packet's ends in one dword
    total = len(pcm_bytes) // 6
    ref_blob, ref_off, _ = enc_sim.encode(ocfg, pcm_bytes, total)
    cfg = pkg_cfg(pkg, ocfg)
    with pkg.NewPacketEncoder(cfg) as enc:
        cap = enc.max_bytes(total)
        src = np.frombuffer(pcm_bytes, np.uint8)
        for blob_shift in (0, 1, 2, 3):
            d_pcm_all = torch.zeros(len(src) + 8, dtype=torch.uint8, device="cuda:0")
            d_pcm_all[pcm_shift:pcm_shift + len(src)] = to_dev(torch, src.copy())
            d_blob_all = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device="cuda:0")
            d_off = torch.zeros(len(ref_off), dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            enc.encode_device(d_pcm_all.data_ptr() + pcm_shift, total, d_blob_all.data_ptr() + blob_shift, cap, d_off.data_ptr(),
                              sync=True)
            off = d_off.cpu().numpy().astype(np.uint64)
            assert np.array_equal(off, ref_off)
            got = d_blob_all.cpu().numpy()
            end = blob_shift + int(off[-1])
            assert np.array_equal(got[blob_shift:end], ref_blob), "pcm +%d blob +%d" % (pcm_shift, blob_shift)
            assert (got[:blob_shift] == 0xAB).all() and (got[end:] == 0xAB).all(), "bytes outside the packets written"


def test_gpu_back_to_back_async_encodes_while_the_scratch_grows(pkg, torch, synth, oracle, enc_sim):
    """three sync = 0 encodes on one handle, each larger than the last (DevMem::ensure frees and reallocates scratch that the
    queued encode before may still use), each to its own outputs, one synchronize() at the end: every result is the host
    build's"""
    fl = 64
    jobs = []
    for k, n in enumerate((100, 5000, 40000)):
        ocfg, pcm_bytes = _music(synth, oracle, fl, 16, 2, n * fl - k, seed=40 + k)
        jobs.append((n * fl - k, pcm_bytes))
    cfg = pkg_cfg(pkg, ocfg)
    outs = []
    with pkg.NewPacketEncoder(cfg) as enc:
        for total, pcm_bytes in jobs:
            d_pcm = to_dev(torch, np.frombuffer(pcm_bytes, np.uint8).copy())
            cap = enc.max_bytes(total)
            d_blob = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
            d_off = torch.zeros(-(-total // fl) + 1, dtype=torch.int64, device="cuda:0")
            outs.append((d_pcm, d_blob, d_off))
        torch.cuda.synchronize()
        for (total, _), (d_pcm, d_blob, d_off) in zip(jobs, outs):
            enc.encode_device(d_pcm.data_ptr(), total, d_blob.data_ptr(), d_blob.numel(), d_off.data_ptr(), sync=False)
        enc.synchronize()
    for (total, pcm_bytes), (_, d_blob, d_off) in zip(jobs, outs):
        ref_blob, ref_off, _ = enc_sim.encode(ocfg, pcm_bytes, total)
        off = d_off.cpu().numpy().astype(np.uint64)
        assert np.array_equal(off, ref_off)
        assert np.array_equal(d_blob[:int(off[-1])].cpu().numpy(), ref_blob)


def test_gpu_encode_orders_after_work_on_the_handles_stream(pkg, torch, synth, oracle, enc_sim):
    """a torch op on the handle's stream fills d_pcm, encode_device(sync = 0) follows with no host sync between them
    (alacgpu.h: inputs ordered on that stream before the call)"""
    ocfg, pcm_bytes = _music(synth, oracle, 4096, 16, 2, 600 * 4096, seed=8)
    total = 600 * 4096
    ref_blob, ref_off, _ = enc_sim.encode(ocfg, pcm_bytes, total)
    cfg = pkg_cfg(pkg, ocfg)
    src = to_dev(torch, np.frombuffer(pcm_bytes, np.uint8).copy())
    d_pcm = torch.zeros_like(src)
    with pkg.NewPacketEncoder(cfg) as enc:
        cap = enc.max_bytes(total)
        d_blob = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
        d_off = torch.zeros(len(ref_off), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        s = torch.cuda.ExternalStream(pkg.lib().alacgpu_encoder_stream(enc._h))
        with torch.cuda.stream(s):
            d_pcm.copy_(src.view(torch.int16).flip(0).flip(0).view(torch.uint8))  # a few kernels of queued work
        enc.encode_device(d_pcm.data_ptr(), total, d_blob.data_ptr(), cap, d_off.data_ptr(), sync=False)
        enc.synchronize()
    off = d_off.cpu().numpy().astype(np.uint64)
    assert np.array_equal(off, ref_off)
    assert np.array_equal(d_blob[:int(off[-1])].cpu().numpy(), ref_blob)


def test_gpu_cookie_counts_everything_so_far_and_a_zero_frame_encode(pkg, torch, synth, oracle, enc_sim):
    ocfg = oracle.make_config(4096, 16, 2, sample_rate=48000)
    ta, tb = 7 * 4096 + 11, 3 * 4096
    a = synth.pack_pcm(ocfg, make_pcm(synth, ocfg, synth.PROFILE_NOISE, ta, seed=1))  # large packets
    b = synth.pack_pcm(ocfg, edge_pcm.bursts(synth, ocfg, tb))
    cfg = pkg_cfg(pkg, ocfg)
    with pkg.NewPacketEncoder(cfg) as enc:
        _, off_a = gpu_encode(torch, enc, a, ta)
        _, off_b = gpu_encode(torch, enc, b, tb)
        c1 = enc.cookie()
        d_pcm = torch.zeros(16, dtype=torch.uint8, device="cuda:0")
        d_blob = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda:0")
        d_off = torch.full((1,), -7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        enc.encode_device(d_pcm.data_ptr(), 0, d_blob.data_ptr(), enc.max_bytes(0), d_off.data_ptr(), sync=True)
        assert d_off.cpu().tolist() == [0] and bool((d_blob == 0xAB).all())
        c2 = enc.cookie()
    assert c1 == c2, "a zero-frame encode changed the cookie"
    sa = np.diff(off_a.cpu().numpy())
    sb = np.diff(off_b.cpu().numpy())
    c = pkg.ParseMagicCookie(c1)
    assert c.MaxFrameBytes == max(int(sa.max()), int(sb.max())) and int(sa.max()) > int(sb.max())
    total_bytes = int(sa.sum()) + int(sb.sum())
    assert abs(c.AvgBitRate - total_bytes * 8 * 48000 / (ta + tb)) <= 1


def _class_blocks(synth, oracle, enc_sim, ocfg, seed):
    """7 distinct packets of frame_length frames -> (pcm bytes of the 7, their packets' bytes, sizes)"""
    fl, ch = ocfg.frame_length, ocfg.num_channels
    rng = np.random.default_rng(seed)
    top = 1 << (ocfg.bit_depth - 1)
    # a different loudness per class (so that packets long enough to compress differ in size), from silence to full scale
    amp = np.repeat([1, 2, 5, 40, 700, 9000, top], fl)[:, None]
    pcm = np.clip(rng.integers(-top, top, size=(7 * fl, ch)) * amp // top, -top, top - 1)
    pcm[::fl, 0] = [0, 1, -1, 77, -300, top - 1, -top]  # and a different first sample: 7 distinct packets
    pcm_bytes = synth.pack_pcm(ocfg, pcm.astype(np.int32))
    blob, off, _ = enc_sim.encode(ocfg, pcm_bytes, 7 * fl)
    assert len({blob[int(off[k]):int(off[k + 1])].tobytes() for k in range(7)}) == 7
    return pcm_bytes, blob, np.diff(off).astype(np.int64)


def _check_cycled_batch(torch, pkg, ocfg, n, pcm7, blob7, sizes7):
    """encode n packets whose PCM cycles through the 7 classes; offsets in closed form; the blob is periodic with period
    sum(sizes7), so viewed as rows of that period every row must be the 7 packets' bytes"""
    dev = torch.device("cuda:0")
    bpp = len(pcm7) // 7
    cycles = -(-n // 7)
    d_pcm = to_dev(torch, np.frombuffer(pcm7, np.uint8).copy()).repeat(cycles)[:n * bpp]
    total = n * ocfg.frame_length
    cfg = pkg_cfg(pkg, ocfg)
    with pkg.NewPacketEncoder(cfg) as enc:
        cap = enc.max_bytes(total)
        d_blob = torch.full((cap,), 0xAB, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        enc.encode_device(d_pcm.data_ptr(), total, d_blob.data_ptr(), cap, d_off.data_ptr(), sync=True)
    del d_pcm
    period = int(sizes7.sum())
    prefix = to_dev(torch, np.concatenate([[0], np.cumsum(sizes7)]).astype(np.int64))
    i = torch.arange(n + 1, dtype=torch.int64, device=dev)
    want_off = (i // 7) * period + prefix[i % 7]
    assert torch.equal(d_off, want_off), "offsets differ from the closed form at %s" % \
        torch.nonzero(d_off != want_off)[:4].flatten().tolist()
    del i, want_off
    full = n // 7
    row = to_dev(torch, blob7.copy())
    rows = d_blob[:full * period].view(full, period)
    bad = torch.nonzero((rows != row).any(dim=1))[:4].flatten().tolist()
    assert not bad, "cycles %s differ (packets %s..)" % (bad, [7 * b for b in bad])
    rest = int(prefix[n % 7].item())
    assert torch.equal(d_blob[full * period:full * period + rest], row[:rest])
    assert bool((d_blob[full * period + rest:] == 0xAB).all())


def test_gpu_two_launches_of_alac_enc_pack(pkg, torch, synth, oracle, enc_sim):
    """2^24 + 4 099 one-frame 16-bit mono packets: more than kPacketsPerPack = 2^24, so alac_enc_pack runs in two launches
    (the second with first_packet = 2^24). Every packet is escaped: 23 + 16 + 3 bits = 6 bytes.

    Why the 7-class cycle catches a lost slice start: packet i holds the PCM of class i % 7. A launch that ignored
    first_packet would write packets 0..4 098 a second time and leave packets 2^24.. unwritten (0xAB sentinels); one that
    took its packet from the slice but its PCM or layout from the batch start would give packet 2^24 + j the bytes of packet
    j, whose class j % 7 differs from (2^24 + j) % 7 because 2^24 = 1 mod 7. Either breaks a row of the periodic blob."""
    _need_gb(torch, 18)
    n = (1 << 24) + 4099
    ocfg = oracle.make_config(1, 16, 1)
    pcm7, blob7, sizes7 = _class_blocks(synth, oracle, enc_sim, ocfg, seed=24)
    assert (sizes7 == 6).all() and n > (1 << 24)
    _check_cycled_batch(torch, pkg, ocfg, n, pcm7, blob7, sizes7)


def test_gpu_two_launches_of_alac_enc_chains(pkg, torch, synth, oracle, enc_sim):
    """2^23 + 65 537 packets of 9 frames, 8 channels: n * 8 > 2^26 = kChainsPerLaunch chains, so alac_enc_chains runs in two
    launches (the second with first_chain = 2^26).

    Why the 7-class cycle catches a lost first_chain: chain t belongs to packet t / 8, class (t / 8) % 7. A second launch that
    started at chain 0 again would leave the chains of packets 2^23.. unencoded; one that wrote its chains to the slice's
    place but encoded them from the batch start would give packet 2^23 + j the chains of packet j, whose class differs
    because 2^23 = 4 mod 7. The sizes of the 7 classes differ, so the offsets' closed form breaks too."""
    _need_gb(torch, 24)
    n = (1 << 23) + 65537
    ocfg = oracle.make_config(9, 16, 8)
    pcm7, blob7, sizes7 = _class_blocks(synth, oracle, enc_sim, ocfg, seed=26)
    assert n * 8 > (1 << 26) and len(set(sizes7.tolist())) > 3
    _check_cycled_batch(torch, pkg, ocfg, n, pcm7, blob7, sizes7)
