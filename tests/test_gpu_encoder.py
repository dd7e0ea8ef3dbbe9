"""The batch encoder on the MI355X (k_enc.hip through the C ABI): its bytes equal the host build of the same logic
(tests/host_sim/enc_sim.cpp, checked against the oracle and the synth writer in test_encoder_host.py), and the GPU
decoder gives back the source PCM from them, fed with the encoder's offsets and d_sizes = NULL."""
import ctypes
import importlib

import numpy as np
import pytest

from tests import m4a
from tests.test_encoder_host import BPS, COOKIE_PARAMS, EncSim, make_pcm

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


def encode_on_device(torch, enc, pcm_bytes, frames):
    """-> (d_blob, d_offsets) torch tensors on cuda:0, through alacgpu_encode_device"""
    dev = torch.device("cuda:0")
    d_pcm = torch.from_numpy(np.frombuffer(pcm_bytes or b"\0", np.uint8).copy()).to(dev)
    cap = enc.max_bytes(frames)
    fl = enc.config.FrameLength
    n = (frames + fl - 1) // fl
    d_blob = torch.zeros(max(cap, 1), dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    enc.encode_device(d_pcm.data_ptr(), frames, d_blob.data_ptr(), cap, d_off.data_ptr(), sync=True)
    return d_blob, d_off


def decode_on_device(torch, pkg, cfg, d_blob, d_off):
    """GPU decode of the encoder's output, d_sizes = NULL -> (pcm bytes of all packets, frames, status)"""
    dev = torch.device("cuda:0")
    n = d_off.numel() - 1
    stride = cfg.FrameLength * cfg.NumChannels * BPS[cfg.BitDepth]
    d_out = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    d_fr = torch.zeros(n, dtype=torch.int32, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    blob_bytes = int(d_off[-1].item())
    with pkg.NewPacketDecoder(cfg, 0) as dec:
        dec.decode_batch_device(d_blob.data_ptr(), blob_bytes, d_off.data_ptr(), None, n, d_out.data_ptr(), stride,
                                d_fr.data_ptr(), d_st.data_ptr(), sync=True)
    return d_out, d_fr, d_st


def check_round_trip(torch, pkg, cfg, d_blob, d_off, pcm_bytes, frames):
    d_out, d_fr, d_st = decode_on_device(torch, pkg, cfg, d_blob, d_off)
    assert not d_st.cpu().numpy().any(), "GPU decoder rejects packets"
    fl, bpf = cfg.FrameLength, cfg.NumChannels * BPS[cfg.BitDepth]
    n = d_off.numel() - 1
    expect = np.array([min(fl, frames - i * fl) for i in range(n)], np.int32)
    assert np.array_equal(d_fr.cpu().numpy(), expect)
    full = frames // fl
    want = np.frombuffer(pcm_bytes, np.uint8)
    if full:  # the full packets: one comparison on the device
        w = torch.from_numpy(want[:full * fl * bpf].copy()).to(d_out.device).view(full, fl * bpf)
        assert torch.equal(d_out[:full], w), "PCM differs"
    if n > full:
        tail = d_out[full, :(frames - full * fl) * bpf].cpu().numpy()
        assert np.array_equal(tail, want[full * fl * bpf:])


MATRIX = [(d, ch, fl) for d in (16, 20, 24, 32) for ch in (1, 2, 3, 6, 8) for fl in (4096, 4095, 1)]


@pytest.mark.parametrize("depth,ch,fl", MATRIX)
def test_gpu_encode_equals_host_build_and_round_trips(pkg, torch, synth, oracle, enc_sim, depth, ch, fl):
    ocfg = oracle.make_config(fl, depth, ch)
    total = {4096: 3 * 4096 + 1000, 4095: 2 * 4095 + 17, 1: 37}[fl]
    pcm_bytes = synth.pack_pcm(ocfg, make_pcm(synth, ocfg, synth.PROFILE_MUSIC, total, seed=depth * 10 + ch))
    ref_blob, ref_off, _ = enc_sim.encode(ocfg, pcm_bytes, total)
    cfg = pkg_cfg(pkg, ocfg)
    with pkg.NewPacketEncoder(cfg) as enc:
        d_blob, d_off = encode_on_device(torch, enc, pcm_bytes, total)
    off = d_off.cpu().numpy().astype(np.uint64)
    assert np.array_equal(off, ref_off)
    assert np.array_equal(d_blob[:int(off[-1])].cpu().numpy(), ref_blob)
    check_round_trip(torch, pkg, cfg, d_blob, d_off, pcm_bytes, total)


@pytest.mark.parametrize("profile,depth,ch,fl,total", [("NOISE", 16, 2, 4096, 4 * 4096 - 5), ("NOISE", 24, 6, 4096, 2 * 4096),
                                                       ("QUIET", 16, 8, 4096, 3 * 4096 + 7), ("QUIET", 32, 2, 4096, 4096),
                                                       ("SILENT", 16, 1, 70000, 70000)])
def test_gpu_escapes_runs_and_long_frames(pkg, torch, synth, oracle, enc_sim, profile, depth, ch, fl, total):
    ocfg = oracle.make_config(fl, depth, ch)
    if profile == "SILENT":
        pcm = np.zeros((total, ch), np.int32)
        pcm[0] = 5
    else:
        pcm = make_pcm(synth, ocfg, getattr(synth, "PROFILE_" + profile), total, seed=5)
    pcm_bytes = synth.pack_pcm(ocfg, pcm)
    ref_blob, ref_off, ref_esc = enc_sim.encode(ocfg, pcm_bytes, total)
    assert (profile == "NOISE") == bool(ref_esc.all())
    cfg = pkg_cfg(pkg, ocfg)
    with pkg.NewPacketEncoder(cfg) as enc:
        d_blob, d_off = encode_on_device(torch, enc, pcm_bytes, total)
    off = d_off.cpu().numpy().astype(np.uint64)
    assert np.array_equal(off, ref_off)
    assert np.array_equal(d_blob[:int(off[-1])].cpu().numpy(), ref_blob)
    check_round_trip(torch, pkg, cfg, d_blob, d_off, pcm_bytes, total)


def test_gpu_batch_of_65536_packets(pkg, torch, synth, oracle, enc_sim):
    """65 536 packets: the size scan runs over 256 workgroups; the batch round-trips in full through the GPU decoder, and a
    seeded sample of 512 packets is byte-identical to the host build (every packet is encoded on its own, so a packet's
    bytes are those of its PCM alone)."""
    ocfg = oracle.make_config(1024, 16, 2)
    n = 65536
    b = synth.gen_batch(ocfg, n, threads=16)
    pcm = b.pcm  # [n, stride]; the 1 % short packets' rows end in zeros, which is just more PCM here
    pcm_bytes = pcm.tobytes()
    frames = n * 1024
    cfg = pkg_cfg(pkg, ocfg)
    with pkg.NewPacketEncoder(cfg) as enc:
        d_blob, d_off = encode_on_device(torch, enc, pcm_bytes, frames)
        ms = enc.last_kernel_ms()
        c = pkg.ParseMagicCookie(enc.cookie())
    off = d_off.cpu().numpy().astype(np.uint64)
    sizes = np.diff(off)
    assert len(off) == n + 1 and sizes.min() > 0
    assert c.MaxFrameBytes == int(sizes.max())
    check_round_trip(torch, pkg, cfg, d_blob, d_off, pcm_bytes, frames)
    rng = np.random.default_rng(1234)
    for i in sorted(rng.choice(n, 512, replace=False).tolist()):
        ref_blob, ref_off, _ = enc_sim.encode(ocfg, pcm[i].tobytes(), 1024, threads=2)
        got = d_blob[int(off[i]):int(off[i + 1])].cpu().numpy()
        assert np.array_equal(got, ref_blob), "packet %d differs from the host build" % i
    print("65 536 x 1024-frame 16-bit stereo packets: %.3f ms, %.4f of raw" % (ms, float(off[-1]) / len(pcm_bytes)))


def test_host_entry_equals_device_entry_pinned_and_pageable(pkg, torch, synth, oracle):
    ocfg = oracle.make_config(4096, 24, 2)
    total = 20 * 4096 + 99
    pcm_bytes = synth.pack_pcm(ocfg, make_pcm(synth, ocfg, synth.PROFILE_MUSIC, total, seed=9))
    cfg = pkg_cfg(pkg, ocfg)
    L = pkg.lib()
    with pkg.NewPacketEncoder(cfg) as enc:
        d_blob, d_off = encode_on_device(torch, enc, pcm_bytes, total)
        dev_off = d_off.cpu().numpy().astype(np.uint64)
        dev_blob = d_blob[:int(dev_off[-1])].cpu().numpy()
        # pageable input (staged)
        blob, offsets = enc.encode(np.frombuffer(pcm_bytes, np.uint8))
        assert np.array_equal(offsets, dev_off) and np.array_equal(blob, dev_blob)
        # pinned input and pinned output (transferred in place)
        p_in = L.alacgpu_host_alloc(len(pcm_bytes))
        cap = enc.max_bytes(total)
        p_out = L.alacgpu_host_alloc(cap)
        assert p_in and p_out
        try:
            ctypes.memmove(p_in, pcm_bytes, len(pcm_bytes))
            pin = np.ctypeslib.as_array((ctypes.c_uint8 * len(pcm_bytes)).from_address(p_in))
            blob2, offsets2 = enc.encode(pin)
            assert np.array_equal(offsets2, dev_off) and np.array_equal(blob2, dev_blob)
            offs3 = np.zeros(len(dev_off), np.uint64)
            got = ctypes.c_uint64()
            rc = L.alacgpu_encode(enc._h, p_in, total, p_out, cap, offs3.ctypes.data, ctypes.byref(got))
            assert rc == 0 and got.value == int(dev_off[-1])
            out = np.ctypeslib.as_array((ctypes.c_uint8 * got.value).from_address(p_out)).copy()
            assert np.array_equal(offs3, dev_off) and np.array_equal(out, dev_blob)
        finally:
            L.alacgpu_host_free(p_in)
            L.alacgpu_host_free(p_out)
        # int32 [frames][channels] input in the PCM domain
        pcm = make_pcm(synth, ocfg, synth.PROFILE_MUSIC, total, seed=9)
        blob4, offsets4 = enc.encode(pcm)
        assert np.array_equal(offsets4, dev_off) and np.array_equal(blob4, dev_blob)


def test_small_blob_cap_is_rejected_and_nothing_is_written(pkg, torch, synth, oracle):
    ocfg = oracle.make_config(4096, 16, 2)
    total = 3 * 4096
    pcm_bytes = synth.pack_pcm(ocfg, make_pcm(synth, ocfg, synth.PROFILE_MUSIC, total))
    cfg = pkg_cfg(pkg, ocfg)
    dev = torch.device("cuda:0")
    with pkg.NewPacketEncoder(cfg) as enc:
        cap = enc.max_bytes(total)
        d_pcm = torch.from_numpy(np.frombuffer(pcm_bytes, np.uint8).copy()).to(dev)
        d_blob = torch.full((cap + 4096,), 0xAB, dtype=torch.uint8, device=dev)
        d_off = torch.full((5,), -7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(ValueError):
            enc.encode_device(d_pcm.data_ptr(), total, d_blob.data_ptr(), cap - 1, d_off.data_ptr(), sync=True)
        torch.cuda.synchronize()
        assert bool((d_blob == 0xAB).all()) and bool((d_off == -7).all())
        with pytest.raises(ValueError):
            enc.encode(np.frombuffer(pcm_bytes, np.uint8)[:-1])  # not a whole number of frames


def test_encoded_file_reads_back_through_the_stream_decoder(pkg, torch, synth, oracle):
    """cookie -> ParseMagicCookie -> config; the packets in an M4A (tests/m4a.py); stream.NewDecoder gives the source PCM."""
    stream = importlib.import_module("saprobe-alac_amd.stream")
    ocfg = oracle.make_config(4096, 16, 2, sample_rate=48000)
    total = 37 * 4096 + 1234
    pcm_bytes = synth.pack_pcm(ocfg, make_pcm(synth, ocfg, synth.PROFILE_MUSIC, total, seed=21))
    with pkg.NewPacketEncoder(pkg_cfg(pkg, ocfg)) as enc:
        blob, offsets = enc.encode(pcm_bytes)
        cookie = enc.cookie()
    cfg = pkg.ParseMagicCookie(cookie)
    sizes = np.diff(offsets)
    assert (cfg.FrameLength, cfg.BitDepth, cfg.NumChannels, cfg.SampleRate) == (4096, 16, 2, 48000)
    assert cfg.MaxFrameBytes == int(sizes.max())
    assert abs(cfg.AvgBitRate - len(blob) * 8 * 48000 / total) <= 1
    packets = [blob[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(len(sizes))]
    data = m4a.write_m4a(cfg, packets, per_chunk=[5])
    with stream.NewDecoder(data, window=16) as d:
        f = d.Format()
        assert (f.SampleRate, f.BitDepth, f.Channels) == (48000, 16, 2)
        assert d.ReadAll() == pcm_bytes


@pytest.mark.parametrize("pb,mb,kb", COOKIE_PARAMS)
def test_gpu_cookie_parameter_extremes(pkg, torch, synth, oracle, enc_sim, pb, mb, kb):
    """PB / MB / KB at the ends of their bytes (KB 0: every element raw): GPU bytes = host build, GPU round trip."""
    ocfg = oracle.make_config(4096, 16, 2, pb=pb, mb=mb, kb=kb)
    total = 3 * 4096 + 17
    pcm_bytes = synth.pack_pcm(ocfg, make_pcm(synth, ocfg, synth.PROFILE_QUIET, total, seed=pb + mb + kb))
    ref_blob, ref_off, ref_esc = enc_sim.encode(ocfg, pcm_bytes, total)
    assert (kb == 0) == bool(ref_esc.all())
    cfg = pkg_cfg(pkg, ocfg)
    with pkg.NewPacketEncoder(cfg) as enc:
        d_blob, d_off = encode_on_device(torch, enc, pcm_bytes, total)
    off = d_off.cpu().numpy().astype(np.uint64)
    assert np.array_equal(off, ref_off)
    assert np.array_equal(d_blob[:int(off[-1])].cpu().numpy(), ref_blob)
    check_round_trip(torch, pkg, cfg, d_blob, d_off, pcm_bytes, total)


def test_gpu_scan_carries_across_chunks(pkg, torch, synth, oracle, enc_sim):
    """70 000 packets = 274 workgroup sums: the single-workgroup scan runs two chunks of 256 and carries between them. The
    whole batch (offsets and bytes) equals the host build and round-trips through the GPU decoder."""
    ocfg = oracle.make_config(16, 16, 2)
    n = 70000
    total = n * 16 - 5
    pcm_bytes = synth.pack_pcm(ocfg, make_pcm(synth, ocfg, synth.PROFILE_MUSIC, total, seed=77))
    ref_blob, ref_off, _ = enc_sim.encode(ocfg, pcm_bytes, total)
    cfg = pkg_cfg(pkg, ocfg)
    with pkg.NewPacketEncoder(cfg) as enc:
        d_blob, d_off = encode_on_device(torch, enc, pcm_bytes, total)
    off = d_off.cpu().numpy().astype(np.uint64)
    assert len(off) == n + 1 and np.array_equal(off, ref_off)
    assert np.array_equal(d_blob[:int(off[-1])].cpu().numpy(), ref_blob)
    check_round_trip(torch, pkg, cfg, d_blob, d_off, pcm_bytes, total)
