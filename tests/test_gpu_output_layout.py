"""Where the decoder writes, not only what: every decode entry runs on a guarded output buffer and every byte of it is
accounted for afterwards.

The buffer is one flat allocation of lead + n * stride + tail bytes filled with a position-dependent pattern
((i * 7 + 3) % 251, so shifted or duplicated writes show too); the entry gets base + lead. After the decode:

  region                                   device entry           host entry, _start / _wait, decode_packet
  [0, frames * bpf) of a slot              the oracle's PCM       the oracle's PCM
  [frames * bpf, fb) of a decoded packet   pattern (untouched)    zero
  [0, fb) of a failing packet              unspecified            zero
  [fb, stride) of every slot, lead, tail   pattern                pattern

Layouts a-f (include/alacgpu.h): stride fb, round16(fb), round16(fb) + 16 at a 16-byte aligned base, and misaligned
bases or strides, which send every packet down the irregular kernels (alac_regular.h: classify_regular). Packets:
a synth batch, partial packets of every residue the stagers care about (4-frame groups of the 3-byte writers, 16-byte
pieces, 32-dword flush chunks), compressed and escaped, mutated and truncated packets. Expected bytes come from the
oracle on the same packets."""
import ctypes
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEAD = 64    # guard bytes in front of slot 0 (a multiple of 16: the layout's offset adds to it)
TAIL = 320   # guard bytes behind the last slot
PARTIAL_K = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
SHIFT = {16: 0, 20: 0, 24: 1, 32: 2}
E_OK, E_ARG, E_DECODE = 0, -2, -4


@pytest.fixture(scope="module")
def torch(pkg):
    import importlib
    t = importlib.import_module("torch")
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


def r16(x):
    return (x + 15) // 16 * 16


def pattern(nbytes):
    return ((np.arange(nbytes, dtype=np.int64) * 7 + 3) % 251).astype(np.uint8)


def layouts(fb):
    """layout -> (offset of slot 0 from a 16-byte boundary, stride)"""
    return {"a": (0, fb), "b": (0, r16(fb)), "c": (0, r16(fb) + 16), "d": (4, r16(fb) + 16), "e": (1, fb + 3),
            "f": (0, fb + 1)}


def aligned(off, stride):
    return off % 16 == 0 and stride % 16 == 0


def pkg_cfg(pkg, ocfg):
    return pkg.PacketConfig(FrameLength=ocfg.frame_length, BitDepth=ocfg.bit_depth, NumChannels=ocfg.num_channels,
                            PB=ocfg.pb, MB=ocfg.mb, KB=ocfg.kb, MaxRun=ocfg.max_run, SampleRate=ocfg.sample_rate)


def partial_packets(synth, cfg, seed):
    """Packets of k < frame_length frames for every k of PARTIAL_K and fl - 1, each compressed (the width's shift bytes)
    and escaped."""
    fl, depth = cfg.frame_length, cfg.bit_depth
    pcm = synth.signal(cfg, synth.PROFILE_MUSIC, seed, fl)
    ne = synth.num_elements(cfg.num_channels)
    out = []
    for k in sorted({k for k in PARTIAL_K + (fl - 1,) if 1 <= k < fl}):
        for kw in (dict(never_escape=1, bytes_shifted=SHIFT[depth]), dict(force_escape=1)):
            out.append(synth.encode_packet(cfg, [synth.default_elem(**kw) for _ in range(ne)], pcm[:k]))
    return out


def packet_set(synth, helpers, cfg, n, profile, seed):
    """A shuffled list of packets: a synth batch, the partial packets, mutated and truncated ones."""
    b = synth.gen_batch(cfg, n, profile=profile, base_seed=seed, threads=8)
    packets = [b.packet(i) for i in range(b.n)] + partial_packets(synth, cfg, seed)
    rng = np.random.default_rng(seed)
    packets += helpers.mutate_packets(b, rng, 48)
    for _ in range(24):
        p = b.packet(int(rng.integers(b.n)))
        packets.append(p[:int(rng.integers(1, len(p)))])
    return [packets[i] for i in rng.permutation(len(packets))]


def oracle_ref(oracle, helpers, cfg, packets):
    blob, offs, sizes = helpers.pack_packets(packets)
    return oracle.decode_batch(cfg, blob, offs, sizes, threads=8)


def host_inputs(helpers, packets):
    blob, offs, _ = helpers.pack_dense(packets)
    return np.ascontiguousarray(blob), np.concatenate([offs, [np.uint64(len(blob))]]).astype(np.uint64)


class DeviceInputs:
    def __init__(self, torch, helpers, packets):
        blob, offs, sizes = helpers.pack_dense(packets)
        dev = torch.device("cuda:0")
        self.n = len(packets)
        self.blob_bytes = len(blob)
        self.blob = torch.from_numpy(np.ascontiguousarray(blob)).to(dev)
        self.off = torch.from_numpy(np.concatenate([offs, [np.uint64(len(blob))]]).astype(np.int64)).to(dev)
        self.sz = torch.from_numpy(sizes.astype(np.int32)).to(dev)


def device_decode(torch, dec, inp, off, stride, use_sizes):
    """alacgpu_decode_batch_device into a guarded buffer -> (lead, pattern, buffer after, frames, status)"""
    lead = LEAD + off
    pat = pattern(lead + inp.n * stride + TAIL)
    d_buf = torch.from_numpy(pat).to(torch.device("cuda:0"))
    assert d_buf.data_ptr() % 16 == 0
    d_fr = torch.full((inp.n,), -1, dtype=torch.int32, device=d_buf.device)
    d_st = torch.full((inp.n,), -1, dtype=torch.int32, device=d_buf.device)
    torch.cuda.synchronize()  # the handle's stream does not order against torch's
    dec.decode_batch_device(inp.blob.data_ptr(), inp.blob_bytes, inp.off.data_ptr(), inp.sz.data_ptr() if use_sizes else None,
                            inp.n, d_buf.data_ptr() + lead, stride, d_fr.data_ptr(), d_st.data_ptr(), sync=True)
    return lead, pat, d_buf.cpu().numpy(), d_fr.cpu().numpy().view(np.uint32), d_st.cpu().numpy()


def check_layout(what, ref, bpf, lead, stride, pat, got, frames, status, device):
    """Status words and frame counts are the oracle's, and every byte of the guarded buffer is what the table in the
    module docstring says. device: the device entry's rules, else the host entries'. -> slots of failing packets that the
    decode wrote to (device entry)."""
    out, rframes, rstatus = ref
    assert np.array_equal(status, rstatus), "%s: status differs at %s" % (what, np.nonzero(status != rstatus)[0][:8])
    assert np.array_equal(frames, rframes), "%s: frame count differs at %s" % (what, np.nonzero(frames != rframes)[0][:8])
    n, fb = out.shape
    exp = pat.copy()
    e = exp[lead:lead + n * stride].reshape(n, stride)
    g = got[lead:lead + n * stride].reshape(n, stride)
    nb = rframes.astype(np.int64) * bpf
    have = np.arange(fb)[None, :] < nb[:, None]
    e[:, :fb] = np.where(have, out, e[:, :fb] if device else np.uint8(0))
    bad = rstatus != 0
    written = 0
    if device:
        written = int((g[bad, :fb] != e[bad, :fb]).any(axis=1).sum())
        e[bad, :fb] = g[bad, :fb]  # a failing packet's slot: unspecified, but nothing outside it may change
    diff = np.nonzero(got != exp)[0]
    if len(diff):
        def where(o):
            if o < lead:
                return "lead byte %d" % o
            if o >= lead + n * stride:
                return "tail byte %d" % (o - lead - n * stride)
            i, c = divmod(int(o) - lead, stride)
            region = "PCM" if c < nb[i] else "behind the frames" if c < fb else "gap"
            return "slot %d byte %d (%s; %d PCM bytes of %d, status %#x): %d, want %d" % (
                i, c, region, nb[i], fb, rstatus[i], got[o], exp[o])
        raise AssertionError("%s: %d bytes differ: %s" % (what, len(diff), "; ".join(where(o) for o in diff[:6])))
    return written


# depth, channels, frame length, profile of the batch
PAIR_CASES = [(16, 1, 333, 0), (16, 2, 700, 0), (16, 2, 4096, 3), (20, 2, 333, 3), (24, 1, 1000, 0), (24, 2, 333, 0),
              (32, 1, 700, 3), (32, 2, 1000, 0)]
# (5: no shift bytes, wide keys; 6: each channel its own predictor order)
WIDE_CASES = [(24, 2, 1000, 5), (32, 2, 700, 6), (24, 2, 333, 6), (32, 2, 4096, 5)]
IRREGULAR_CASES = [(16, 2, 32, 0), (24, 1, 17, 3), (20, 2, 8, 0)]
MULTI_CASES = [(16, 3, 200, 0), (16, 4, 100, 3), (16, 6, 64, 0), (16, 8, 48, 0), (24, 8, 40, 3), (32, 3, 100, 0),
               (32, 7, 64, 0), (20, 5, 70, 0), (16, 7, 90, 3)]


@pytest.mark.parametrize("depth,ch,fl,profile", PAIR_CASES + WIDE_CASES + IRREGULAR_CASES + MULTI_CASES)
def test_device_entry_writes_only_the_frames(torch, pkg, oracle, synth, helpers, depth, ch, fl, profile):
    """alacgpu_decode_batch_device at six layouts, with and without d_sizes: PCM where the oracle has frames, nothing
    behind a partial frame, in a slot's gap, in front of slot 0 or behind the last slot. The aligned layouts take one
    route whatever the gap; the misaligned ones take the irregular kernels only."""
    cfg = oracle.make_config(fl, depth, ch)
    bpf = ch * oracle.bytes_per_sample(depth)
    fb = fl * bpf
    packets = packet_set(synth, helpers, cfg, 160 if fl < 4096 else 96, profile, depth * 131 + ch * 17 + fl)
    ref = oracle_ref(oracle, helpers, cfg, packets)
    assert (ref[2] != 0).sum() >= 8 and (ref[1][ref[2] == 0] < fl).sum() >= 10
    inp = DeviceInputs(torch, helpers, packets)
    disp = {}
    with pkg.NewPacketDecoder(pkg_cfg(pkg, cfg)) as dec:
        for name, (off, stride) in layouts(fb).items():
            for use_sizes in (True, False):
                lead, pat, got, fr, st = device_decode(torch, dec, inp, off, stride, use_sizes)
                what = "layout %s (offset %d, stride %d) sizes %s" % (name, off, stride, use_sizes)
                written = check_layout(what, ref, bpf, lead, stride, pat, got, fr, st, device=True)
                if not (ch <= 2 and fl > 32 and aligned(off, stride)):
                    # no wave pair runs: today the irregular kernels leave a failing packet's slot alone (the wave pairs
                    # may have written its first samples); pinned so that a change to it is deliberate
                    assert written == 0, "%s: %d failing slots written" % (what, written)
                disp[name, use_sizes] = dec.last_dispatch()
    on = [k for k in disp if aligned(*layouts(fb)[k[0]])]
    off16 = [k for k in disp if k not in on]
    assert len(on) >= 4 and len(off16) >= 6
    for k in on:
        assert disp[k] == disp[on[0]], (k, disp[k], disp[on[0]])  # the gap never changes the route
    for k in off16:
        assert disp[k]["narrow_slots"] == 0 and disp[k]["wide_slots"] == 0, (k, disp[k])
        assert disp[k]["irregular_slots"] == disp[k]["slots"] > 0, (k, disp[k])
    d = disp[on[0]]
    if ch <= 2 and fl > 32:
        assert d["narrow_slots"] > 0, d
        if profile == synth.PROFILE_MUSIC_NOSHIFT:  # chanBits above 23: the wide keys' wave pairs
            assert d["wide_slots"] > 0, d
    else:
        assert d["narrow_slots"] == 0 and d["wide_slots"] == 0, d


@pytest.mark.parametrize("depth,fl,fit", [(16, 64, None), (16, 64, "5"), (24, 48, None)])
def test_large_batches_write_only_the_frames(torch, pkg, oracle, synth, helpers, monkeypatch, depth, fl, fit):
    """70 000 stereo packets with partial ones among them, at the aligned gapped layout c and the misaligned layout d:
    the gated twin (16-bit between four and five rounds), five four-wave workgroups per CU (ALACGPU_FIT=5), the 24-bit
    four-wave kernel. The dispatch read back names the narrow kernel; the misaligned layout has none."""
    if fit is None:
        monkeypatch.delenv("ALACGPU_FIT", raising=False)
    else:
        monkeypatch.setenv("ALACGPU_FIT", fit)
    n = 70000
    cfg = oracle.make_config(fl, depth, 2)
    bpf = 2 * oracle.bytes_per_sample(depth)
    fb = fl * bpf
    b = synth.gen_batch(cfg, n, base_seed=depth * 7 + fl, threads=16)
    packets = [b.packet(i) for i in range(n)]
    part = partial_packets(synth, cfg, fl)
    for j in range(0, n, 211):
        packets[j] = part[(j // 211) % len(part)]
    ref = oracle_ref(oracle, helpers, cfg, packets)
    assert (ref[1] < fl).sum() >= 300
    inp = DeviceInputs(torch, helpers, packets)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lay = layouts(fb)
    with pkg.NewPacketDecoder(pkg_cfg(pkg, cfg)) as dec:
        for name in ("c", "d"):
            off, stride = lay[name]
            lead, pat, got, fr, st = device_decode(torch, dec, inp, off, stride, True)
            check_layout("n=%d layout %s fit %s" % (n, name, fit), ref, bpf, lead, stride, pat, got, fr, st, device=True)
            d = dec.last_dispatch()
            if name == "d":
                assert d["narrow_slots"] == 0 and d["wide_slots"] == 0 and d["narrow_kernel"] == "", d
                continue
            q = d["narrow_slots"] / n_cu
            assert d["narrow_slots"] > 0, d
            if fit is not None:
                assert d["narrow_kernel"] == "alac_decode_16q" and d["workgroups_per_cu"] == 5 and not d["gated"], d
            elif depth == 16:
                if q <= 4:
                    assert d["narrow_kernel"] == "alac_decode_16q" and not d["gated"], (q, d)
                elif q <= 5:  # alac_gpu.h: decode_mode, between four and five rounds
                    assert d["narrow_kernel"] == "alac_decode_16g" and d["gated"] == 1, (q, d)
                if n_cu == 256:
                    assert 4 < q <= 5, q
            else:
                want = 4 if q <= 4 else 5 if q <= 5 else 4 if q <= 7.5 else 5
                assert d["narrow_kernel"] == "alac_decode_24q" and d["workgroups_per_cu"] == want and not d["gated"], (q, d)


class Pinned:
    """alacgpu_host_alloc'd bytes as a numpy array."""

    def __init__(self, lib, nbytes):
        self.lib = lib
        self.p = lib.alacgpu_host_alloc(nbytes)
        assert self.p, lib.alacgpu_last_error()
        self.a = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(self.p))

    def free(self):
        self.a = None
        self.lib.alacgpu_host_free(self.p)


def host_buffers(lib, mem, total, n):
    """-> (out bytes, frames, status, the pinned blocks to free); out is filled with the pattern"""
    if mem == "pinned":
        bufs = [Pinned(lib, total), Pinned(lib, 4 * n), Pinned(lib, 4 * n)]
        out, fr, st = bufs[0].a, bufs[1].a.view(np.uint32), bufs[2].a.view(np.int32)
    else:
        bufs = []
        out, fr, st = np.empty(total, np.uint8), np.empty(n, np.uint32), np.empty(n, np.int32)
    out[:] = pattern(total)
    fr[:] = 0xdeadbeef
    st[:] = -1
    return out, fr, st, bufs


@pytest.mark.parametrize("depth,ch,fl,n,chunk_mb", [(16, 2, 333, 200, None), (16, 1, 4095, 60, None), (20, 5, 70, 200, None),
                                                    (24, 2, 4096, 60, None), (16, 2, 333, 2600, "1")])
def test_host_entry_leaves_the_gap_alone(torch, pkg, oracle, synth, helpers, monkeypatch, depth, ch, fl, n, chunk_mb):
    """alacgpu_decode_batch at strides fb, round16(fb), round16(fb) + 16 and fb + 3, from pageable memory (also at an odd
    address) and with out / frames / status all pinned: PCM, zeros behind a partial frame and in a failing packet's slot,
    and the caller's bytes in [fb, stride) and around the slots. ALACGPU_CHUNK_MB=1: chunks of 1 MB, at least three."""
    if chunk_mb is None:
        monkeypatch.delenv("ALACGPU_CHUNK_MB", raising=False)
    else:
        monkeypatch.setenv("ALACGPU_CHUNK_MB", chunk_mb)
    cfg = oracle.make_config(fl, depth, ch)
    bpf = ch * oracle.bytes_per_sample(depth)
    fb = fl * bpf
    packets = packet_set(synth, helpers, cfg, n, 0, fl + ch)
    n = len(packets)
    assert chunk_mb is None or n * fb >= 3 << 20
    ref = oracle_ref(oracle, helpers, cfg, packets)
    blob, offs = host_inputs(helpers, packets)
    with pkg.NewPacketDecoder(pkg_cfg(pkg, cfg)) as dec:
        lib = dec._lib
        for stride in (fb, r16(fb), r16(fb) + 16, fb + 3):
            for mem, lead in (("pageable", LEAD), ("pageable", LEAD + 1), ("pinned", LEAD)):
                total = lead + n * stride + TAIL
                out, fr, st, bufs = host_buffers(lib, mem, total, n)
                try:
                    pat = pattern(total)
                    pkg._check(lib.alacgpu_decode_batch(dec._h, blob.ctypes.data, blob.size, offs.ctypes.data, n,
                                                        out.ctypes.data + lead, stride, fr.ctypes.data, st.ctypes.data))
                    check_layout("%s stride %d lead %d" % (mem, stride, lead), ref, bpf, lead, stride, pat, out, fr, st,
                                 device=False)
                finally:
                    for p in bufs:
                        p.free()


def test_decode_packet_writes_one_frame_buffer(torch, pkg, oracle, synth, helpers):
    """alacgpu_decode_packet with out_cap = fb + 64: [0, out_len) the oracle's PCM, zero up to fb, the rest untouched; a
    failing packet's frame buffer is zero."""
    for depth, ch, fl in ((16, 2, 333), (24, 2, 4096), (20, 5, 70)):
        cfg = oracle.make_config(fl, depth, ch)
        bpf = ch * oracle.bytes_per_sample(depth)
        fb = fl * bpf
        b = synth.gen_batch(cfg, 4, base_seed=fl, threads=4)
        rng = np.random.default_rng(fl)
        packets = [b.packet(0), b.packet(1)] + partial_packets(synth, cfg, fl)[::5] + helpers.mutate_packets(b, rng, 12)
        ref = oracle_ref(oracle, helpers, cfg, packets)
        assert (ref[2] != 0).any()
        with pkg.NewPacketDecoder(pkg_cfg(pkg, cfg)) as dec:
            lib = dec._lib
            for i, p in enumerate(packets):
                total = LEAD + fb + 64
                out = pattern(total)
                pat = out.copy()
                buf = np.frombuffer(p, np.uint8) if p else np.zeros(1, np.uint8)
                n_out = ctypes.c_size_t(12345)
                st = ctypes.c_int32(-1)
                rc = lib.alacgpu_decode_packet(dec._h, buf.ctypes.data, len(p), out.ctypes.data + LEAD, fb + 64,
                                               ctypes.byref(n_out), ctypes.byref(st))
                assert st.value == ref[2][i], (i, st.value, ref[2][i])
                assert rc == (E_OK if ref[2][i] == 0 else E_DECODE), (i, rc)
                assert n_out.value == int(ref[1][i]) * bpf, (i, n_out.value)
                check_layout("packet %d (%d-bit %d-ch %d)" % (i, depth, ch, fl), (ref[0][i:i + 1], ref[1][i:i + 1],
                             ref[2][i:i + 1]), bpf, LEAD, fb + 64, pat, out, ref[1][i:i + 1], np.array([st.value], np.int32),
                             device=False)


def test_async_entry_layout_and_errors(torch, pkg, oracle, synth, helpers):
    """alacgpu_decode_batch_start / _wait on guarded buffers with Python work in between: the host entry's footprint; a
    second _start while one is in flight is ALACGPU_E_ARG, names the decode in flight and touches nothing, and the first
    still completes; _wait with nothing in flight is ALACGPU_E_OK; out_stride < frame bytes is accepted by _start and
    reported by _wait, with its text in the waiting thread's alacgpu_last_error."""
    cfg = oracle.make_config(333, 16, 2)
    bpf, fb = 4, 333 * 4
    packets = packet_set(synth, helpers, cfg, 400, 3, 333)
    n = len(packets)
    blob, offs = host_inputs(helpers, packets)
    with pkg.NewPacketDecoder(pkg_cfg(pkg, cfg)) as dec:
        lib, h = dec._lib, dec._h
        assert lib.alacgpu_decode_batch_wait(h) == E_OK
        for stride in (r16(fb), fb + 3):
            total = LEAD + n * stride + TAIL
            out, fr, st, _ = host_buffers(lib, "pageable", total, n)
            out2, fr2, st2, _ = host_buffers(lib, "pageable", total, n)
            pat = pattern(total)
            assert lib.alacgpu_decode_batch_start(h, blob.ctypes.data, blob.size, offs.ctypes.data, n, out.ctypes.data + LEAD,
                                                  stride, fr.ctypes.data, st.ctypes.data) == E_OK
            rc = lib.alacgpu_decode_batch_start(h, blob.ctypes.data, blob.size, offs.ctypes.data, n, out2.ctypes.data + LEAD,
                                                stride, fr2.ctypes.data, st2.ctypes.data)
            msg = lib.alacgpu_last_error() or b""
            assert rc == E_ARG and b"in flight" in msg, (rc, msg)
            ref = oracle_ref(oracle, helpers, cfg, packets)  # Python work while the decode runs
            assert lib.alacgpu_decode_batch_wait(h) == E_OK, lib.alacgpu_last_error()
            check_layout("start/wait stride %d" % stride, ref, bpf, LEAD, stride, pat, out, fr, st, device=False)
            assert np.array_equal(out2, pat) and (fr2 == 0xdeadbeef).all() and (st2 == -1).all()
            assert lib.alacgpu_decode_batch_wait(h) == E_OK
        total = LEAD + n * fb + TAIL
        out, fr, st, _ = host_buffers(lib, "pageable", total, n)
        assert lib.alacgpu_decode_batch_start(h, blob.ctypes.data, blob.size, offs.ctypes.data, n, out.ctypes.data + LEAD,
                                              fb - 1, fr.ctypes.data, st.ctypes.data) == E_OK
        res = {}

        def waiter():
            res["rc"] = lib.alacgpu_decode_batch_wait(h)
            res["msg"] = lib.alacgpu_last_error() or b""

        t = threading.Thread(target=waiter)
        t.start()
        t.join()
        assert res["rc"] == E_ARG and b"out_stride" in res["msg"], res
        assert np.array_equal(out, pattern(total))
        assert lib.alacgpu_decode_batch_wait(h) == E_OK
        # the handle still decodes
        total = LEAD + n * fb + TAIL
        out, fr, st, _ = host_buffers(lib, "pageable", total, n)
        pkg._check(lib.alacgpu_decode_batch(h, blob.ctypes.data, blob.size, offs.ctypes.data, n, out.ctypes.data + LEAD, fb,
                                            fr.ctypes.data, st.ctypes.data))
        check_layout("after the errors", ref, bpf, LEAD, fb, pattern(total), out, fr, st, device=False)


def test_destroy_waits_for_the_decode_in_flight(torch, pkg, oracle, synth, helpers):
    """alacgpu_destroy with a decode in flight returns once the caller's buffers are complete and correct; the next
    alacgpu_create on the device gets that handle back from the pool, and it decodes correctly."""
    cfg = oracle.make_config(4096, 24, 2)
    bpf, fb = 6, 4096 * 6
    packets = packet_set(synth, helpers, cfg, 300, 3, 4096)
    n = len(packets)
    ref = oracle_ref(oracle, helpers, cfg, packets)
    blob, offs = host_inputs(helpers, packets)
    lib = pkg.lib()
    lib.alacgpu_trim()  # an empty pool: the next create takes back the handle destroyed below
    stride = r16(fb) + 16
    total = LEAD + n * stride + TAIL
    dec = pkg.NewPacketDecoder(pkg_cfg(pkg, cfg))
    first = dec._h.value
    out, fr, st, _ = host_buffers(lib, "pageable", total, n)
    assert lib.alacgpu_decode_batch_start(dec._h, blob.ctypes.data, blob.size, offs.ctypes.data, n, out.ctypes.data + LEAD,
                                          stride, fr.ctypes.data, st.ctypes.data) == E_OK
    dec.close()
    check_layout("destroyed in flight", ref, bpf, LEAD, stride, pattern(total), out, fr, st, device=False)
    with pkg.NewPacketDecoder(pkg_cfg(pkg, cfg)) as dec2:
        assert dec2._h.value == first
        out, fr, st, _ = host_buffers(lib, "pageable", total, n)
        pkg._check(lib.alacgpu_decode_batch(dec2._h, blob.ctypes.data, blob.size, offs.ctypes.data, n, out.ctypes.data + LEAD,
                                            stride, fr.ctypes.data, st.ctypes.data))
        check_layout("pooled handle", ref, bpf, LEAD, stride, pattern(total), out, fr, st, device=False)
