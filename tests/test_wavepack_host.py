"""The pack pass on the CPU: csrc/alac_wavepack.h built with g++ (tests/host_sim/pack_sim.cpp), slice for slice, tile for
tile and work item for work item what the gfx950 kernel of k_wavepack.hip runs, against the numpy restatement of
tests/wavepack_ref.py.

* the matrix: depths 16/20/24/32 x channels 1/2/3/6/8 x frame_length 4096/4095/1 x STREAM/PACKETS x FLOAT/INT, three
  packets plus an odd remainder, samples beyond the range, NaNs and infinities among them, the clipped count exact, every
  byte of the PCM buffer outside the footprint still the sentinel, and every element behind the last clip's frames
  unread (they are NaNs that would count);
* total_frames around the tile size, a slice size of two workgroups;
* every alignment of the waveform, its strides and the PCM buffer gives the same bytes;
* the extremes against first principles (exact rationals) as well as the restatement;
* the pack of the forward restatement's output gives the source bytes back;
* the entries' argument checks, which return before any HIP call, and the new names in header, binding and .hpp."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import wave_ref as wr
from tests import wavepack_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    return pr.build_pack_sim()


def run_sim(L, fl, depth, ch, x, layout, wtype, wave_mis=0, slack=0, pcm_mis=0, lead=8, per=0, want_clipped=True):
    """x [ch, total] laid out in a sentinel-filled buffer whose tensor starts `lead` elements in, at an address that is wave_mis
    modulo 16; the pass into a sentinel-filled PCM buffer whose stream starts 16 + pcm_mis bytes in, at an address that is pcm_mis
    modulo 16 -> (image uint8, base, clipped, launches)."""
    total = x.shape[1]
    cs, ps, elems = pr.geometry(layout, fl, ch, total, slack, lead)
    src = pr.lay_out(x, layout, fl, lead, cs, ps, elems)
    buf = wr.at_alignment(4 * elems, (wave_mis - 4 * lead) % 16)
    buf.view(np.uint32)[:] = src
    nbytes = total * ch * wr.BPS[depth]
    base = 16 + pcm_mis
    pcm = wr.at_alignment(base + nbytes + 40, 0)
    pcm[:] = pr.PCM_SENTINEL
    clipped = np.full(1, 0xDEAD, np.uint64)
    launches = np.zeros(1, np.uint64)
    rc = L.pack_sim_run(fl, depth, ch, buf.ctypes.data + 4 * lead, layout, wtype, cs, ps, total, pcm.ctypes.data + base,
                        clipped.ctypes.data if want_clipped else None, per, launches.ctypes.data)
    assert rc == 0
    assert np.array_equal(buf.view(np.uint32), src), "the pass wrote to its input"
    return pcm.copy(), base, int(clipped[0]), int(launches[0])


def check(L, fl, depth, ch, x, layout, wtype, **kw):
    img, base, clipped, launches = run_sim(L, fl, depth, ch, x, layout, wtype, **kw)
    ref, ref_clipped = pr.pack_ref(x, depth, wtype)
    want = pr.expected_image(ref, img.size, base)
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError("byte %d of the buffer (stream byte %d): got %#x, want %#x (%d differ)" %
                             (bad[0], bad[0] - base, img[bad[0]], want[bad[0]], len(bad)))
    if kw.get("want_clipped", True):
        assert clipped == ref_clipped
    return launches


@pytest.mark.parametrize("fl", [4096, 4095, 1])
@pytest.mark.parametrize("ch", [1, 2, 3, 6, 8])
@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_host_build_equals_numpy_over_the_matrix(sim, depth, ch, fl):
    rng = np.random.default_rng(depth * 1000 + ch * 10 + fl)
    total = 3 * fl + 1237 % fl if fl > 1 else 301
    for wtype in (pr.FLOAT, pr.INT):
        x = pr.random_wave(rng, ch, total, depth, wtype)
        assert pr.pack_ref(x, depth, wtype)[1] > 0 or (wtype == pr.INT and depth == 32)
        for layout in (pr.STREAM, pr.PACKETS):
            check(sim, fl, depth, ch, x, layout, wtype)


@pytest.mark.parametrize("depth,ch", [(16, 2), (24, 2), (20, 3), (32, 8), (16, 1), (24, 7)])
def test_total_frames_around_the_tile_size(sim, depth, ch):
    """One frame less than a tile, a tile, one more, and two tiles less one: STREAM cuts its one segment into tiles, PACKETS
    gets clips of that length (two and a bit of them)."""
    rng = np.random.default_rng(depth + ch)
    tile = sim.pack_sim_tile_frames(depth, ch)
    assert tile % 64 == 0 and tile * ch * wr.BPS[depth] <= 8192
    for total in (tile - 1, tile, tile + 1, 2 * tile - 1):
        x = pr.random_wave(rng, ch, total, depth, pr.FLOAT)
        check(sim, 4096, depth, ch, x, pr.STREAM, pr.FLOAT, wave_mis=4, slack=1, pcm_mis=3)
        y = pr.random_wave(rng, ch, 2 * total + 5, depth, pr.INT)
        check(sim, total, depth, ch, y, pr.PACKETS, pr.INT, wave_mis=8, slack=3, pcm_mis=9)


@pytest.mark.parametrize("layout", [pr.STREAM, pr.PACKETS])
def test_slices_of_two_workgroups(sim, layout):
    """The launch loop with a slice of two tiles: every tile runs once, in ceil(tiles / 2) launches."""
    rng = np.random.default_rng(11)
    depth, ch, fl = 24, 2, 3000
    tile = sim.pack_sim_tile_frames(depth, ch)
    total = 3 * fl + 77
    x = pr.random_wave(rng, ch, total, depth, pr.FLOAT)
    tiles = -(-total // tile) if layout == pr.STREAM else 4 * -(-fl // tile)
    assert tiles >= 7
    assert check(sim, fl, depth, ch, x, layout, pr.FLOAT, per=2) == -(-tiles // 2)
    assert check(sim, fl, depth, ch, x, layout, pr.FLOAT, per=0) == 1


@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 333), (24, 2, 4096), (20, 3, 70), (32, 8, 300), (16, 1, 4095), (24, 6, 513)])
def test_every_alignment_gives_the_same_bytes(sim, depth, ch, fl):
    """The waveform at 0 / 4 / 8 / 12 modulo 16 with slack in both strides (so that the rows of one tensor differ in their
    alignment), the PCM stream at several offsets modulo 16: the 16-byte loads and stores of the body, the narrow ones at
    the ends."""
    rng = np.random.default_rng(depth + ch + fl)
    total = 2 * fl + fl // 3 + 1
    xs = {t: pr.random_wave(rng, ch, total, depth, t) for t in (pr.FLOAT, pr.INT)}
    for wave_mis, slack in ((0, 0), (4, 1), (8, 2), (12, 3), (0, 3), (12, 0)):
        for pcm_mis in (0, 1, 2, 4, 7, 8, 13, 15):
            for layout in (pr.STREAM, pr.PACKETS):
                wtype = pr.FLOAT if (layout == pr.STREAM) == (pcm_mis % 2 == 0) else pr.INT
                check(sim, fl, depth, ch, xs[wtype], layout, wtype, wave_mis=wave_mis, slack=slack, pcm_mis=pcm_mis)


def test_without_a_counter(sim):
    rng = np.random.default_rng(3)
    x = pr.random_wave(rng, 2, 5000, 16, pr.FLOAT)
    img, base, clipped, _ = run_sim(sim, 4096, 16, 2, x, pr.PACKETS, pr.FLOAT, want_clipped=False)
    assert clipped == 0xDEAD
    assert np.array_equal(img, pr.expected_image(pr.pack_ref(x, 16, pr.FLOAT)[0], img.size, base))


def test_no_frames(sim):
    buf = np.zeros(4, np.uint32)
    pcm = np.full(16, pr.PCM_SENTINEL, np.uint8)
    clipped = np.full(1, 7, np.uint64)
    for layout in (pr.STREAM, pr.PACKETS):
        assert sim.pack_sim_run(4096, 16, 2, buf.ctypes.data, layout, pr.FLOAT, 4096, 8192, 0, pcm.ctypes.data, clipped.ctypes.data, 0, None) == 0
        assert clipped[0] == 0 and np.all(pcm == pr.PCM_SENTINEL)


def _exact(x, depth):
    """First principles: the float's exact rational times 2^(q - 1), rounded half to even, saturated -> (value, clipped)."""
    top = 1 << (depth - 1)
    if np.isnan(x):
        return 0, 1
    if np.isinf(x):
        return (top - 1 if x > 0 else -top), 1
    v = round(Fraction(float(x)) * top)  # Python rounds a Fraction half to even
    c = min(max(v, -top), top - 1)
    return c, int(c != v)


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_float_extremes_against_first_principles(sim, depth):
    top = 1 << (depth - 1)
    f32 = np.float32
    one, inv = f32(1.0), f32(2.0 ** -(depth - 1))
    xs = [one, -one, f32(top - 1) * inv, f32(-top) * inv, f32(-top + 1) * inv]  # +-full scale, +-1.0 (f32(top - 1) rounds up at 32 bits)
    xs += [f32(k + 0.5) * inv for k in (0, 1, 2, 3, 4, -1, -2, -3, -4, -5, 1000, 1001, -1000, -1001)]  # ties, both directions
    if depth <= 24:
        xs += [f32(top - 1 + 0.5) * inv, f32(top - 1 - 0.5) * inv, f32(-top - 0.5) * inv, f32(-top + 0.5) * inv, f32(top - 1 + 0.25) * inv,
               f32(-top - 0.75) * inv]  # ties and near-ties at the two bounds
    xs += [np.nextafter(one, f32(0)), np.nextafter(one, f32(2)), np.nextafter(-one, f32(0)), np.nextafter(-one, f32(-2))]  # just inside / outside
    xs += [f32(np.inf), f32(-np.inf), f32(np.nan), -f32(np.nan), f32(1e-45), f32(-1e-45), f32(1e-39), f32(-0.0), f32(0.0), f32(3e38), f32(-3e38),
           f32(0.5), f32(-0.5), f32(1.5), f32(-1.5)]
    x = np.array(xs, f32).reshape(1, -1)
    want = [_exact(v, depth) for v in x[0]]
    vals = np.array([w[0] for w in want], np.int64) << (4 if depth == 20 else 0)
    n_clipped = sum(w[1] for w in want)
    assert n_clipped >= 8 and (vals == 0).sum() >= 6
    ref, ref_clipped = pr.pack_ref(x, depth, pr.FLOAT)
    assert np.array_equal(ref, wr.pack_samples(vals.reshape(-1, 1), depth)) and ref_clipped == n_clipped  # the restatement itself
    for layout in (pr.STREAM, pr.PACKETS):
        img, base, clipped, _ = run_sim(sim, x.shape[1], depth, 1, x, layout, pr.FLOAT)
        got = wr.unpack(img[base:], x.shape[1], depth, 1)[:, 0]
        assert np.array_equal(got, vals), (got, vals)
        assert clipped == n_clipped
        check(sim, x.shape[1], depth, 1, x, layout, pr.FLOAT)


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_int_extremes_against_first_principles(sim, depth):
    w = wr.WIDTH[depth]
    top = 1 << (w - 1)
    vs = [int(v) for v in wr.extremes(depth)] + [top, top + 1, -top - 1, -top - 2, (1 << 31) - 1, -(1 << 31), 15, -15, 16, -16, 17]
    vs = [v for v in vs if -(1 << 31) <= v < (1 << 31)]
    x = np.array(vs, np.int64).astype(np.int32).reshape(1, -1)
    sat = [min(max(v, -top), top - 1) for v in vs]
    vals = np.array([s & ~15 if depth == 20 else s for s in sat], np.int64)
    n_clipped = sum(int(s != v) for s, v in zip(sat, vs))
    assert (n_clipped == 0) == (depth == 32)
    for layout in (pr.STREAM, pr.PACKETS):
        img, base, clipped, _ = run_sim(sim, 7, depth, 1, x, layout, pr.INT)
        assert np.array_equal(wr.unpack(img[base:], len(vs), depth, 1)[:, 0], vals)
        assert clipped == n_clipped
        check(sim, 7, depth, 1, x, layout, pr.INT)


@pytest.mark.parametrize("depth,ch,fl", [(16, 2, 4096), (20, 3, 500), (24, 2, 1345), (32, 8, 100), (24, 1, 4095)])
def test_pack_inverts_the_forward_pass(sim, depth, ch, fl):
    """Source PCM -> the forward restatement's waveform (tests/wave_ref.py) -> the pack: the source bytes come back, for INT at
    every depth and for FLOAT up to 24 bits, with nothing clipped. A 20-bit source has its low four bits clear, as a 20-bit
    stream has them (the pack clears them: they are not part of the sample). At 32 bits a float32 does not hold the sample, and
    the pack gives the restatement's value."""
    rng = np.random.default_rng(depth * ch)
    n = 3
    total = n * fl
    bps = wr.BPS[depth]
    out = wr.hand_slots(rng, n, fl, depth, ch, fl * ch * bps, np.full(n, fl))
    if depth == 20:
        out.reshape(-1, 3)[:, 0] &= 0xF0
    frames, status = np.full(n, fl, np.uint32), np.zeros(n, np.int32)
    for wtype in (pr.FLOAT, pr.INT):
        dt = np.float32 if wtype == pr.FLOAT else np.int32
        stream = wr.ref_stream(out, frames, status, fl, depth, ch, wtype)[0].view(dt)
        packets = wr.ref_packets(out, frames, status, fl, depth, ch, wtype).view(dt)
        assert np.array_equal(np.concatenate(list(packets), axis=1).view(np.uint32), stream.view(np.uint32))
        for layout in (pr.STREAM, pr.PACKETS):
            img, base, clipped, _ = run_sim(sim, fl, depth, ch, stream, layout, wtype, wave_mis=4, slack=1, pcm_mis=5)
            got = img[base:base + total * ch * bps]
            if depth == 32 and wtype == pr.FLOAT:
                assert np.array_equal(got, pr.pack_ref(stream, depth, wtype)[0])
                assert clipped == pr.pack_ref(stream, depth, wtype)[1] > 0  # 2^31 - 1 became 1.0f
            else:
                assert np.array_equal(got, out.reshape(-1)) and clipped == 0


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------
NEW = ("alacgpu_pcm_from_waveform_device", "alacgpu_encode_waveform_device", "alacgpu_encoder_waveform_last_ms")


def test_header_binding_and_hpp_name_the_new_surface(pkg):
    text = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    for fn in NEW:
        assert re.search(r"\b%s\s*\(" % fn, text) and fn in pkg._EXPORTS
    for name in ("pcm_from_waveform_device", "encode_waveform_device", "encode_waveform", "waveform_last_ms"):
        assert hasattr(pkg.PacketEncoder, name)
    assert callable(pkg.save) and "save" in pkg.__all__
    hpp = open(os.path.join(ROOT, "saprobe-alac_amd", "host", "packet_encoder.hpp")).read()
    for fn, method in zip(NEW, ("PcmFromWaveformDevice", "EncodeWaveformDevice", "WaveformLastMs")):
        assert fn in hpp and method in hpp
    mp4 = __import__("importlib").import_module("saprobe-alac_amd.mp4")
    assert callable(mp4.write_m4a)


def test_null_arguments_are_argument_errors_before_any_hip_call(pkg):
    pkg.build()
    L = pkg.lib()
    buf = np.zeros(64, np.uint32)
    p = buf.ctypes.data
    assert L.alacgpu_pcm_from_waveform_device(None, p, 0, 0, 64, 0, 16, p, None, 0) == -2
    assert b"null" in L.alacgpu_last_error()
    assert L.alacgpu_pcm_from_waveform_device(None, None, 0, 0, 0, 0, 0, None, None, 0) == -2
    assert L.alacgpu_encode_waveform_device(None, p, 0, 0, 64, 0, 16, p, 1 << 20, p, None, 0) == -2
    assert L.alacgpu_encode_waveform_device(None, None, 7, 7, 0, 0, 0, None, 0, None, None, 0) == -2
    ms = ctypes.c_float()
    assert L.alacgpu_encoder_waveform_last_ms(None, ctypes.byref(ms)) == -2
    assert b"null" in L.alacgpu_last_error()


def test_the_sim_rejects_what_the_entry_rejects(sim):
    """pack_sim_run repeats the entry's checks (it has no handle): layout, type, alignment, strides."""
    buf = np.zeros(1 << 14, np.uint32)
    pcm = np.zeros(1 << 16, np.uint8)
    w, o = buf.ctypes.data, pcm.ctypes.data
    run = lambda **k: sim.pack_sim_run(k.get("fl", 100), 16, 2, k.get("w", w), k.get("layout", 0), k.get("type", 0), k.get("cs", 1000),  # noqa: E731
                                       k.get("ps", 2000), k.get("total", 250), k.get("o", o), None, 0, None)
    assert run() == 0 and run(layout=1) == 0
    assert run(layout=2) == -2 and run(type=2) == -2 and run(layout=-1) == -2
    assert run(w=w + 2) == -2 and run(w=None) == -2 and run(o=None) == -2
    assert run(cs=249) == -2 and run(cs=250) == 0
    assert run(layout=1, cs=99) == -2 and run(layout=1, cs=100, ps=199) == -2 and run(layout=1, cs=100, ps=200) == 0
    assert run(fl=1, total=1 << 31, cs=1 << 31) == -2


def test_kernel_unit_is_in_the_code_object(pkg):
    pkg.build()
    so = open(pkg.lib_path(), "rb").read()
    assert b"alac_wave_pack" in so
