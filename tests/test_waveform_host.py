"""The waveform pass on the CPU: csrc/alac_waveform.h built with g++ (tests/host_sim/wave_sim.cpp), tile for tile and work
item for work item what the gfx950 kernel of k_wave.hip runs, against the numpy restatement of tests/wave_ref.py.

* the matrix: depths 16/20/24/32 x channels 1/2/3/6/8 x frame_length 4096/4095/1 x STREAM/PACKETS x FLOAT/INT, slots
  written by hand with every extreme of the depth, short packets at the start, in the middle and at the end, failed
  packets, and every element of the wave buffer outside the documented footprint still the sentinel;
* every alignment of the slots and of the wave buffer gives the same values;
* the oracle's decode of synth packets, damaged ones among them, with and without the status words;
* the entry's argument checks, which return before any HIP call, and the new names in header and binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import wave_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    return wr.build_wave_sim()


def run_sim(L, fl, depth, ch, out, frames, status, layout, wtype, pcm_mis=0, wave_mis=0, slack=0, lead=8, want_starts=True):
    """The slots out[n, stride] copied to an address that is pcm_mis modulo 16, the pass into a sentinel-filled buffer whose
    tensor starts `lead` elements in, at an address that is wave_mis modulo 16 -> (image uint32, base, cs, ps, starts)."""
    n, stride = out.shape
    pcm = wr.at_alignment(max(out.size, 1), pcm_mis)
    pcm[:out.size] = out.reshape(-1)
    if layout == wr.STREAM:
        cs, ps = n * fl + slack, 0
        elems = lead + ch * cs + 8
    else:
        cs = fl + slack
        ps = ch * cs + (slack and slack + 1)
        elems = lead + n * ps + 8
    buf = wr.at_alignment(4 * elems, (wave_mis - 4 * lead) % 16, fill=wr.SENTINEL)
    wave = buf.view(np.uint32)
    frames = np.ascontiguousarray(frames, np.uint32)
    st = None if status is None else np.ascontiguousarray(status, np.int32)
    starts = np.full(n + 1, 0xDEAD, np.uint64)
    rc = L.wave_sim_run(fl, depth, ch, pcm.ctypes.data, stride, frames.ctypes.data, None if st is None else st.ctypes.data, n, layout,
                        wtype, wave.ctypes.data + 4 * lead, cs, ps, starts.ctypes.data if want_starts else None)
    assert rc == 0
    return wave.copy(), lead, cs, ps, starts


def check(L, fl, depth, ch, out, frames, status, layout, wtype, **kw):
    img, base, cs, ps, starts = run_sim(L, fl, depth, ch, out, frames, status, layout, wtype, **kw)
    if layout == wr.STREAM:
        ref, ref_starts = wr.ref_stream(out, frames, status, fl, depth, ch, wtype)
    else:
        ref = wr.ref_packets(out, frames, status, fl, depth, ch, wtype)
        ref_starts = wr.ref_stream(out, frames, status, fl, depth, ch, wtype)[1]
    assert np.array_equal(starts, ref_starts)
    want = wr.expected_image(ref, layout, img.size, base, cs, ps)
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError("element %d of the buffer: got %#x, want %#x (%d differ)" % (bad[0], img[bad[0]], want[bad[0]], len(bad)))


@pytest.mark.parametrize("fl", [4096, 4095, 1])
@pytest.mark.parametrize("ch", [1, 2, 3, 6, 8])
@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_host_build_equals_numpy_over_the_matrix(sim, depth, ch, fl):
    rng = np.random.default_rng(depth * 1000 + ch * 10 + fl)
    n = 7 if fl > 1 else 300
    bpf = ch * wr.BPS[depth]
    stride = (fl * bpf + 15) // 16 * 16
    frames = wr.frame_counts(rng, n, fl, "short")
    status = np.zeros(n, np.int32)
    status[[2, n - 1]] = (0x1101, 3)  # failed packets, one of them with a frame count left standing
    out = wr.hand_slots(rng, n, fl, depth, ch, stride, frames)
    for layout in (wr.STREAM, wr.PACKETS):
        for wtype in (wr.FLOAT, wr.INT):
            check(sim, fl, depth, ch, out, frames, status, layout, wtype)


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_every_extreme_converts_as_numpy_does(sim, depth):
    """One packet that is nothing but the depth's extremes, and the float of each against first principles: the integer
    rounded once to 24 significant bits, ties to even, times an exact power of two."""
    ex = wr.extremes(depth)
    fl, ch = len(ex), 1
    out = wr.pack_samples(ex.reshape(-1, 1), depth).reshape(1, -1)
    frames, status = np.array([fl], np.uint32), np.zeros(1, np.int32)
    for wtype in (wr.FLOAT, wr.INT):
        check(sim, fl, depth, ch, out, frames, status, wr.STREAM, wtype)
    img, base, cs, ps, _ = run_sim(sim, fl, depth, ch, out, frames, status, wr.STREAM, wr.FLOAT)
    got = img[base:base + fl].view(np.float32).astype(np.float64)
    w = wr.WIDTH[depth]
    # what the bytes hold (a 20-bit extreme with its low four bits set is read as the 24-bit value it is)
    held = wr.unpack(out[0], fl, depth, 1)[:, 0]
    assert np.array_equal(held, ex)
    exact = np.array([float(np.float32(int(v))) for v in held]) / float(1 << (w - 1))
    assert np.array_equal(got, exact)
    if depth != 32:
        assert np.array_equal(got * (1 << (w - 1)), held.astype(np.float64))  # exact up to 24 bits
    else:
        assert got.max() == 1.0 and got.min() == -1.0  # 2^31 - 1 rounds up to 2^31


@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 333), (24, 2, 4096), (20, 3, 70), (32, 8, 300), (16, 1, 4095), (24, 6, 513)])
def test_every_alignment_gives_the_same_values(sim, depth, ch, fl):
    """Slots at every byte alignment with an odd stride, wave tensors at every element alignment with odd strides, odd
    frame counts (so that start[i] is odd): the 16-byte loads and stores of the body, the narrow ones at the ends."""
    rng = np.random.default_rng(depth + ch + fl)
    n = 9
    bpf = ch * wr.BPS[depth]
    frames = wr.frame_counts(rng, n, fl, "odd")
    status = np.zeros(n, np.int32)
    status[4] = 2
    for pcm_mis, extra in ((0, 0), (1, 1), (7, 3), (8, 16), (15, 5), (4, 12)):
        stride = (fl * bpf + 15) // 16 * 16 + extra if extra != 1 else fl * bpf + (1 - (fl * bpf) % 2)
        out = wr.hand_slots(rng, n, fl, depth, ch, stride, frames)
        for wave_mis, slack in ((0, 0), (4, 1), (8, 2), (12, 3)):
            for layout in (wr.STREAM, wr.PACKETS):
                check(sim, fl, depth, ch, out, frames, status, layout, wr.FLOAT if layout == wr.STREAM else wr.INT, pcm_mis=pcm_mis,
                      wave_mis=wave_mis, slack=slack)


def test_hostile_frame_counts_are_clamped(sim):
    """d_frames above frame_length counts as frame_length: with channel_stride >= n * frame_length nothing leaves its row."""
    rng = np.random.default_rng(5)
    fl, depth, ch, n = 100, 16, 2, 12
    frames = wr.frame_counts(rng, n, fl, "hostile")
    out = wr.hand_slots(rng, n, fl, depth, ch, fl * ch * 2, frames)
    for layout in (wr.STREAM, wr.PACKETS):
        check(sim, fl, depth, ch, out, frames, None, layout, wr.FLOAT)


def test_no_status_words_and_no_starts(sim):
    rng = np.random.default_rng(6)
    fl, depth, ch, n = 257, 24, 2, 10
    frames = wr.frame_counts(rng, n, fl, "odd")
    out = wr.hand_slots(rng, n, fl, depth, ch, fl * ch * 3 + 2, frames)
    check(sim, fl, depth, ch, out, frames, None, wr.STREAM, wr.FLOAT)
    img, base, cs, ps, starts = run_sim(sim, fl, depth, ch, out, frames, None, wr.PACKETS, wr.INT, want_starts=False)
    assert np.all(starts == 0xDEAD)
    assert np.array_equal(img, wr.expected_image(wr.ref_packets(out, frames, None, fl, depth, ch, wr.INT), wr.PACKETS, img.size, base, cs, ps))


def test_empty_batch(sim):
    starts = np.full(1, 7, np.uint64)
    assert sim.wave_sim_run(4096, 16, 2, None, 0, None, None, 0, wr.STREAM, wr.FLOAT, None, 0, 0, starts.ctypes.data) == 0
    assert starts[0] == 0


@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 4096), (24, 2, 512), (20, 6, 100), (32, 3, 64), (16, 8, 4095)])
def test_oracle_decodes_through_the_host_build(sim, oracle, synth, helpers, depth, ch, fl):
    """From the oracle's (out, frames, status) of a synth batch with short packets at the start, in the middle and at the
    end and damaged packets mixed in: with the status words, and without (the oracle reports no frames for a failure)."""
    cfg = oracle.make_config(fl, depth, ch)
    b = synth.gen_batch(cfg, 10, base_seed=depth + ch, threads=4)
    rng = np.random.default_rng(fl)
    packets = [b.packet(i) for i in range(b.n)] + helpers.mutate_packets(b, rng, 6)
    rng.shuffle(packets)
    ne = synth.num_elements(ch)
    pcm = synth.signal(cfg, synth.PROFILE_MUSIC, 3, fl)
    for at, k in ((0, 1), (len(packets) // 2, fl // 2 + 1), (len(packets), max(fl - 1, 1))):
        if k < fl:
            packets.insert(at, synth.encode_packet(cfg, [synth.default_elem(force_escape=1) for _ in range(ne)], pcm[:k]))
    blob, offs, sizes = helpers.pack_packets(packets)
    out, frames, status = oracle.decode_batch(cfg, blob, offs, sizes, threads=4)
    assert (status != 0).any() and (status == 0).any() and (frames < fl).any()
    for st in (status, None):
        for layout in (wr.STREAM, wr.PACKETS):
            check(sim, fl, depth, ch, out, frames, st, layout, wr.FLOAT, wave_mis=4, slack=1)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_new_surface(pkg):
    text = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    for name, value in (("ALACGPU_WAVE_STREAM", 0), ("ALACGPU_WAVE_PACKETS", 1), ("ALACGPU_WAVE_FLOAT", 0), ("ALACGPU_WAVE_INT", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), text), name
    for fn in ("alacgpu_waveform_device", "alacgpu_waveform_last_ms"):
        assert re.search(r"\b%s\s*\(" % fn, text) and fn in pkg._EXPORTS
    assert (pkg.WAVE_STREAM, pkg.WAVE_PACKETS, pkg.WAVE_FLOAT, pkg.WAVE_INT) == (0, 1, 0, 1)
    assert hasattr(pkg.PacketDecoder, "waveform_device") and hasattr(pkg.PacketDecoder, "decode_waveform") and callable(pkg.load)
    hpp = open(os.path.join(ROOT, "saprobe-alac_amd", "host", "packet_decoder.hpp")).read()
    assert "alacgpu_waveform_device" in hpp


def test_version_is_0_7_0(pkg):
    pkg.build()
    assert pkg.lib().alacgpu_version() == b"alacgpu 0.7.0 gfx950"


def test_null_handle_is_an_argument_error_before_any_hip_call(pkg):
    pkg.build()
    L = pkg.lib()
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data
    assert L.alacgpu_waveform_device(None, p, 16, p, None, 1, 0, 0, p, 16, 0, None, 0) == -2
    assert L.alacgpu_waveform_device(None, None, 0, None, None, 0, 0, 0, None, 0, 0, None, 0) == -2
    ms = ctypes.c_float()
    assert L.alacgpu_waveform_last_ms(None, ctypes.byref(ms)) == -2
    assert b"null" in L.alacgpu_last_error()


def test_kernel_unit_is_in_the_code_object(pkg):
    pkg.build()
    so = open(pkg.lib_path(), "rb").read()
    assert b"alac_wave_convert" in so and b"alac_wave_offsets" in so
