"""The clip gather on the CPU: csrc/alac_clips.h built with g++ (tests/host_sim/clip_sim.cpp), tile for tile and work item
for work item what the gfx950 kernel of k_clips.hip runs, against the numpy restatement of tests/clip_ref.py.

Every run writes into a sentinel-filled buffer with slack in both strides and guard elements in front and behind, and the
WHOLE buffer is compared bit for bit: the values, the zeros, and every element outside the [clip][channel] rows still the
sentinel. The slots are written by hand (wave_ref.hand_slots): random bytes behind a slot's frames and in failed slots,
which must not show.

* depths 16/20/24/32 x FLOAT/INT x channels 1/2/6/8; frame lengths 1/7/16/33/4096 x clip lengths 1/3/255/256/257/1000;
* every begin % 4 x every base offset of 0..3 elements, with odd strides;
* short and failed slots inside a clip, limit cutting a clip, begin at / around / past the batch and at 2^64 - 1, limit 0 and
  above n, hostile d_frames, NULL d_status / d_valid / d_clip_status, no clips, no packets;
* the slots ending at an inaccessible page;
* the entry's argument checks, and the new names in the library, the header and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import clip_ref as cr
from tests import wave_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def sim():
    return cr.build_clip_sim()


def slots(rng, n, fl, depth, ch, pattern="short", failed=(), extra=0, exact=False):
    """(out, frames, status): hand-written slots; the stride the decode's fast one plus `extra`, or exactly the frame bytes."""
    fb = fl * ch * wr.BPS[depth]
    stride = fb if exact else (fb + 15) // 16 * 16 + extra
    frames = wr.frame_counts(rng, n, fl, pattern)
    status = np.zeros(n, np.int32)
    for k, i in enumerate(failed):
        status[i] = (0x1101, 3, 0x2202)[k % 3]
    return wr.hand_slots(rng, n, fl, depth, ch, stride, frames), frames, status


def run_sim(S, fl, depth, ch, out, frames, status, begin, limit, L, wtype, base=0, slack=None, pcm_mis=0, want_valid=True,
            want_status=True, guard_bytes=0):
    """The slots copied to an address that is pcm_mis modulo 16, the gather into a sentinel-filled buffer whose tensor starts
    8 + base elements in (base elements behind a 16-byte boundary), rows an odd stride apart -> (image, lead, cs, ps, valid,
    clip_status)."""
    n, stride = out.shape if out is not None else (0, 0)
    pcm = wr.at_alignment(max(n * stride, 16), pcm_mis)
    if n:
        pcm[:out.size] = out.reshape(-1)
    B = len(begin)
    cs = L + (slack if slack is not None else 1 + L % 2)  # odd
    ps = ch * cs + 3
    lead = 8 + base
    elems = lead + B * ps + 8
    buf = wr.at_alignment(4 * elems, 0, fill=wr.SENTINEL)
    img = buf.view(np.uint32)
    fr = np.ascontiguousarray(frames if n else np.zeros(1), np.uint32)
    st = None if status is None else np.ascontiguousarray(status if n else np.zeros(1), np.int32)
    bg = np.array([int(b) for b in begin] or [0], np.uint64)
    lm = np.array([int(x) for x in limit] or [0], np.uint64)
    valid = np.full(max(B, 1), 0xDEAD, np.uint32)
    cstat = np.full(max(B, 1), 0xDEAD, np.int32)
    rc = S.clip_sim_run(fl, depth, ch, pcm.ctypes.data, stride, fr.ctypes.data, None if st is None else st.ctypes.data, n,
                        bg.ctypes.data, lm.ctypes.data, B, L, wtype, img.ctypes.data + 4 * lead, cs, ps,
                        valid.ctypes.data if want_valid else None, cstat.ctypes.data if want_status else None, guard_bytes)
    assert rc == 0
    return img.copy(), lead, cs, ps, valid[:B], cstat[:B]


def check(S, fl, depth, ch, out, frames, status, begin, limit, L, wtype, **kw):
    img, lead, cs, ps, valid, cstat = run_sim(S, fl, depth, ch, out, frames, status, begin, limit, L, wtype, **kw)
    n = 0 if out is None else len(out)
    ref, r_valid, r_cstat = cr.ref_clips(out, frames[:n], None if status is None else status[:n], fl, depth, ch, wtype, begin, limit, L)
    want = cr.expected_image(ref, img.size, lead, cs, ps)
    if not np.array_equal(img, want):
        bad = np.nonzero(img != want)[0]
        raise AssertionError("element %d of the buffer (tensor starts at %d): got %#x, want %#x (%d differ)"
                             % (bad[0], lead, img[bad[0]], want[bad[0]], len(bad)))
    if kw.get("want_valid", True):
        assert np.array_equal(valid, r_valid), (valid, r_valid)
    else:
        assert np.all(valid == 0xDEAD)
    if kw.get("want_status", True):
        assert np.array_equal(cstat, r_cstat), (cstat, r_cstat)
    else:
        assert np.all(cstat == 0xDEAD)
    return ref, r_valid, r_cstat


def spread(rng, n, fl, L):
    """Clip descriptors all over a batch of n slots: in one slot, across slot boundaries, over the short and failed slots in
    the middle, at the batch's end, and a few at random -> (begin, limit)."""
    total = n * fl
    begin = [0, 1, 2, 3, fl - 1, fl, fl + 1, max(total // 2 - L // 2, 0), max(total - L, 0), max(total - L, 0) + 1, total - 1]
    begin += [int(x) for x in rng.integers(0, total, 5)]
    limit = [n] * len(begin)
    return begin, limit


@pytest.mark.parametrize("ch", [1, 2, 6, 8])
@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_host_build_equals_numpy_over_depths_and_channels(sim, depth, ch):
    rng = np.random.default_rng(depth * 10 + ch)
    fl, n, L = 33, 12, 100
    out, frames, status = slots(rng, n, fl, depth, ch, failed=(4,))
    begin, limit = spread(rng, n, fl, L)
    for wtype in (wr.FLOAT, wr.INT):
        check(sim, fl, depth, ch, out, frames, status, begin, limit, L, wtype)


@pytest.mark.parametrize("L", [1, 3, 255, 256, 257, 1000])
@pytest.mark.parametrize("fl", [1, 7, 16, 33, 4096])
def test_frame_lengths_and_clip_lengths(sim, fl, L):
    """Clips inside one slot, over many slots, and longer than a tile (8-channel 32-bit tiles are 256 columns, fewer at the
    smallest frame lengths)."""
    rng = np.random.default_rng(fl * 1000 + L)
    n = max(3, min(1200, (L + 300) // fl + 3))
    for depth, ch, wtype in ((16, 2, wr.FLOAT), (32, 8, wr.INT), (24, 6, wr.FLOAT)):
        out, frames, status = slots(rng, n, fl, depth, ch, failed=(n // 2 + 1,) if n > 4 else ())
        begin, limit = spread(rng, n, fl, L)
        check(sim, fl, depth, ch, out, frames, status, begin, limit, L, wtype)


@pytest.mark.parametrize("depth,ch,fl,L", [(16, 2, 33, 257), (24, 6, 7, 255), (32, 1, 4096, 1000), (20, 8, 16, 256), (16, 1, 1, 300)])
def test_every_alignment_gives_the_same_values(sim, depth, ch, fl, L):
    """Every begin % 4 with every base offset of 0..3 elements, odd channel and clip strides, slots at odd byte alignments."""
    rng = np.random.default_rng(depth + ch + fl)
    n = max(4, (L + 40) // fl + 3)
    for pcm_mis, extra in ((0, 0), (5, 3), (8, 16)):
        out, frames, status = slots(rng, n, fl, depth, ch, pattern="odd", failed=(2,), extra=extra)
        for base in range(4):
            begin = [fl + b for b in range(4)] + [5 * b for b in range(4)]
            for wtype, slack in ((wr.FLOAT, None), (wr.INT, 3 + L % 2)):
                check(sim, fl, depth, ch, out, frames, status, begin, [n] * len(begin), L, wtype, base=base, slack=slack, pcm_mis=pcm_mis)


def test_short_and_failed_slots_leave_a_zero_gap(sim):
    """Worked by hand: slot 1 holds 5 of 16 frames, slot 2 failed with a frame count left standing."""
    rng = np.random.default_rng(1)
    fl, depth, ch, n, L = 16, 16, 2, 4, 48
    frames = np.array([16, 5, 16, 16], np.uint32)
    status = np.array([0, 0, 0x1101, 0], np.int32)
    out = wr.hand_slots(rng, n, fl, depth, ch, fl * ch * 2, frames)
    ref, valid, cstat = check(sim, fl, depth, ch, out, frames, status, [8, 0, 40], [n, n, n], L, wr.FLOAT)
    assert list(valid) == [8 + 5 + 0 + 8, 16 + 5 + 0, 0 + 16] and list(cstat) == [0x1101, 0x1101, 0x1101]
    assert not ref[0, :, 8 + 5:8 + 32].any() and not ref[2, :, :8].any() and not ref[2, :, 24:].any()
    # the samples are the slots' own: clip 0 column 0 is frame 8 of slot 0, column 40 is frame 0 of slot 3
    v0 = wr.elements(wr.unpack(out[0], 16, depth, ch), depth, wr.FLOAT)
    v3 = wr.elements(wr.unpack(out[3], 16, depth, ch), depth, wr.FLOAT)
    assert np.array_equal(ref[0, :, :8], v0[8:].T) and np.array_equal(ref[0, :, 40:], v3[:8].T)
    # without the status words the failed slot's frame count stands, and its bytes show
    _, valid, cstat = check(sim, fl, depth, ch, out, frames, None, [8], [n], L, wr.INT)
    assert list(valid) == [8 + 5 + 16 + 8] and list(cstat) == [0]


def test_limit_cuts_a_clip(sim):
    rng = np.random.default_rng(2)
    fl, depth, ch, n, L = 16, 24, 2, 6, 40
    frames = np.full(n, fl, np.uint32)
    status = np.zeros(n, np.int32)
    status[3] = 7
    out = wr.hand_slots(rng, n, fl, depth, ch, fl * ch * 3, frames)
    begin, limit = [20, 20, 20, 20, 20, 50], [n, 3, 2, 1, 0, 3]
    ref, valid, cstat = check(sim, fl, depth, ch, out, frames, status, begin, limit, L, wr.INT)
    # the failed slot 3 is touched only under the full limit; a limit at or below the clip's first slot leaves nothing
    assert list(valid) == [40 - 12, 28, 12, 0, 0, 0] and list(cstat) == [7, 0, 0, 0, 0, 0]
    assert ref[1, :, :28].any() and not ref[1, :, 28:].any() and not ref[3].any()


@pytest.mark.parametrize("depth,ch,fl,L", [(16, 2, 33, 100), (32, 8, 7, 257), (24, 1, 4096, 5000)])
def test_descriptors_at_and_past_the_batch(sim, depth, ch, fl, L):
    """begin at, just before and past n * frame_length and at the top of 64 bits; limit 0 and above n: zeros where the grid
    has no slot, no read outside the slots."""
    rng = np.random.default_rng(L)
    n = 5
    out, frames, status = slots(rng, n, fl, depth, ch, failed=(1,))
    total = n * fl
    begin = [total - 1, total, total + 1, max(total - L, 0), max(total - L, 0) + 1, total + L, U64, U64 - 1, U64 - L, U64 - L + 1, 1 << 63, (1 << 63) - 1,
             (1 << 32) - 1, 1 << 32, 0, 0, 0, 3, fl]
    limit = [n] * 14 + [0, n + 7, U64, U64, 1 << 32]
    for wtype in (wr.FLOAT, wr.INT):
        ref, valid, _ = check(sim, fl, depth, ch, out, frames, status, begin, limit, L, wtype)
    assert not ref[1].any() and not ref[6].any() and not ref[14].any() and valid[1] == valid[6] == valid[14] == 0
    assert np.array_equal(ref[15], ref[16]) and valid[15] > 0


def test_hostile_frame_counts_are_clamped(sim):
    rng = np.random.default_rng(5)
    fl, depth, ch, n, L = 100, 16, 2, 12, 333
    out, frames, _ = slots(rng, n, fl, depth, ch, pattern="hostile")
    assert frames[n // 3] == fl + 5 and frames[(2 * n) // 3] == 0xFFFFFFFF
    begin, limit = spread(rng, n, fl, L)
    ref, valid, _ = check(sim, fl, depth, ch, out, frames, None, begin, limit, L, wr.FLOAT)
    assert valid.max() <= L


def test_null_status_valid_and_clip_status(sim):
    rng = np.random.default_rng(6)
    fl, depth, ch, n, L = 33, 24, 2, 9, 257
    out, frames, status = slots(rng, n, fl, depth, ch, pattern="odd", failed=(3,))
    begin, limit = spread(rng, n, fl, L)
    check(sim, fl, depth, ch, out, frames, None, begin, limit, L, wr.FLOAT)
    check(sim, fl, depth, ch, out, frames, status, begin, limit, L, wr.INT, want_valid=False)
    check(sim, fl, depth, ch, out, frames, status, begin, limit, L, wr.INT, want_status=False)
    check(sim, fl, depth, ch, out, frames, None, begin, limit, L, wr.FLOAT, want_valid=False, want_status=False)


def test_no_clips_and_no_packets(sim):
    rng = np.random.default_rng(7)
    fl, depth, ch, L = 33, 16, 2, 70
    out, frames, status = slots(rng, 4, fl, depth, ch)
    img, lead, cs, ps, _, _ = run_sim(sim, fl, depth, ch, out, frames, status, [], [], L, wr.FLOAT)
    assert np.all(img == wr.SENTINEL)  # nothing is touched
    assert sim.clip_sim_run(fl, depth, ch, None, 0, None, None, 0, None, None, 0, L, wr.FLOAT, None, 0, 0, None, None, 0) == 0
    # clips over an empty batch are zeros
    ref, valid, cstat = check(sim, fl, depth, ch, None, np.zeros(0, np.uint32), np.zeros(0, np.int32), [0, 5, U64], [0, 9, U64], L, wr.INT)
    assert not ref.any() and not valid.any() and not cstat.any()


@pytest.mark.parametrize("depth,ch,fl,L", [(16, 2, 33, 100), (24, 3, 7, 257), (32, 8, 64, 300), (16, 1, 4096, 1000)])
def test_slots_that_end_at_an_inaccessible_page(sim, depth, ch, fl, L):
    """pcm_stride exactly the frame bytes and a short last slot, whose last frame's last byte is the last accessible one: a read
    behind a slot's frames that leaves the buffer is fatal here."""
    rng = np.random.default_rng(fl)
    n = 6
    out, frames, status = slots(rng, n, fl, depth, ch, failed=(2,), exact=True)
    frames[n - 1] = max(fl - 3, 1)
    bpf = ch * wr.BPS[depth]
    guard = (n - 1) * out.shape[1] + int(frames[n - 1]) * bpf
    total = n * fl
    begin = [max(total - L, 0), max(total - L // 2, 0), total - 1, total - 3, total, 0, (n - 1) * fl, U64]
    for wtype in (wr.FLOAT, wr.INT):
        check(sim, fl, depth, ch, out, frames, status, begin, [n] * len(begin), L, wtype, guard_bytes=guard)
    # hostile: the last slot claims more frames than it has room for; the clamp to frame_length keeps the reads inside
    frames[n - 1] = 0xFFFFFFFF
    check(sim, fl, depth, ch, out, frames, status, begin, [n + 1] * len(begin), L, wr.FLOAT, guard_bytes=n * out.shape[1])


def test_tiles_fit_the_staging_buffer(sim):
    """make_params' tile: a multiple of 32 columns whose segments fit the staging buffer at every frame length."""
    room = sim.clip_sim_stage_bytes()
    for fl in list(range(1, 300)) + [511, 512, 1000, 4095, 4096, 1 << 16, 1 << 24]:
        for depth in (16, 24, 32):
            for ch in (1, 2, 3, 6, 8):
                tc = sim.clip_sim_tile_cols(fl, depth, ch)
                assert tc >= 32 and tc % 32 == 0 and sim.clip_sim_stage_need(fl, depth, ch) <= room, (fl, depth, ch)
    assert sim.clip_sim_tile_cols(4096, 16, 2) == 2048 and sim.clip_sim_tile_cols(4096, 32, 8) == 256


def test_argument_checks(sim):
    fl, depth, ch, n, B, L = 64, 16, 2, 4, 2, 50
    fb = fl * ch * 2
    pcm = np.zeros(n * fb, np.uint8)
    fr = np.zeros(n, np.uint32)
    bg = np.zeros(B, np.uint64)
    lm = np.full(B, n, np.uint64)
    clips = np.zeros(B * ch * L + 4, np.uint32)
    P, F, G, M, C = pcm.ctypes.data, fr.ctypes.data, bg.ctypes.data, lm.ctypes.data, clips.ctypes.data

    def rc(pcm=P, stride=fb, frames=F, n=n, begin=G, limit=M, B=B, L=L, wtype=0, out=C, cs=L, ps=ch * L, depth=depth):
        return sim.clip_sim_run(fl, depth, ch, pcm, stride, frames, None, n, begin, limit, B, L, wtype, out, cs, ps, None, None, 0)

    assert rc() == 0
    for bad in (dict(pcm=None), dict(frames=None), dict(begin=None), dict(limit=None), dict(out=None),  # NULL buffers
                dict(wtype=2), dict(wtype=-1),                                                           # unknown type
                dict(L=0),                                                                               # clip_frames = 0
                dict(out=C + 2), dict(out=C + 1),                                                        # d_clips not on an element boundary
                dict(cs=L - 1), dict(ps=ch * L - 1), dict(cs=L + 1, ps=ch * L + 1),                      # strides too small
                dict(stride=fb - 1),                                                                     # pcm_stride below the frame bytes
                dict(n=1 << 31), dict(B=1 << 31), dict(ps=1 << 62), dict(stride=1 << 62)):               # sizes that overflow
        assert rc(**bad) == -2, bad
    assert not clips.any()
    assert rc(B=0, pcm=None, frames=None, begin=None, limit=None, out=None) == 0  # no clips: nothing is looked at
    assert rc(n=0, stride=0) == 0  # no packets: zeros


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------
def test_library_header_and_binding_name_the_new_surface(pkg):
    pkg.build()
    L = pkg.lib()
    for fn in ("alacgpu_clips_device", "alacgpu_clips_last_ms"):
        assert getattr(ctypes.CDLL(pkg.lib_path()), fn) and fn in pkg._EXPORTS and getattr(L, fn).argtypes
    text = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    for fn in ("alacgpu_clips_device", "alacgpu_clips_last_ms"):
        assert re.search(r"\b%s\s*\(" % fn, text)
    for name in ("clips_device", "clips_last_ms", "decode_clips"):
        assert hasattr(pkg.PacketDecoder, name)
    assert callable(pkg.load_clips) and "load_clips" in pkg.__all__
    hpp = open(os.path.join(ROOT, "saprobe-alac_amd", "host", "packet_decoder.hpp")).read()
    assert "alacgpu_clips_device" in hpp and "ClipsDevice" in hpp
    assert L.alacgpu_version() == b"alacgpu 0.7.0 gfx950"


def test_null_handle_is_an_argument_error_before_any_hip_call(pkg):
    pkg.build()
    L = pkg.lib()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    assert L.alacgpu_clips_device(None, p, 16, p, None, 1, p, p, 1, 4, 0, p, 4, 8, None, None, 0) == -2
    assert L.alacgpu_clips_device(None, None, 0, None, None, 0, None, None, 0, 0, 0, None, 0, 0, None, None, 0) == -2
    ms = ctypes.c_float()
    assert L.alacgpu_clips_last_ms(None, ctypes.byref(ms)) == -2
    assert b"null" in L.alacgpu_last_error()


def test_load_rejects_a_negative_range_before_it_opens_anything(pkg):
    with pytest.raises(ValueError):
        pkg.load(b"", frame_offset=-1)
    with pytest.raises(ValueError):
        pkg.load(b"", num_frames=-2)
    with pytest.raises(ValueError):
        pkg.load_clips([b""], [-1], 10)
    with pytest.raises(ValueError):
        pkg.load_clips([b""], [0], 0)


def test_a_truncated_file_never_reaches_the_decode(pkg, oracle):
    """load_clips on a file whose sample table points past its bytes: the EOF error, with the clip, before anything is
    decoded (so it runs here); and _clip_batch refuses a range that leaves a file rather than let the packet's bytes run
    into the next clip's piece of the blob."""
    from tests import m4a
    cfg = oracle.make_config(4096, 16, 2)
    whole = m4a.write_m4a(cfg, [bytes([k]) * 100 for k in range(1, 4)])
    cut = whole[:len(whole) - 50]  # packet 2 leaves the file
    for srcs, where in (([cut, whole], 0), ([whole, cut], 1)):
        with pytest.raises(pkg.AlacError, match="clip %d: reading sample 2: unexpected EOF" % where):
            pkg.load_clips(srcs, [2 * 4096 + 1 if k == where else 0 for k in range(2)], 100)
    a = (np.arange(150, dtype=np.uint8), np.array([0, 100], np.int64), np.array([100, 100], np.int64), None)
    b = (np.full(300, 7, np.uint8), np.array([0, 100], np.int64), np.array([100, 100], np.int64), None)
    with pytest.raises(pkg.AlacError, match="clip 0"):
        pkg._clip_batch([a, b], [0, 0], [0, 0], [2, 2], 4096)
    blob, offsets, sizes, begin, limit = pkg._clip_batch([a, b], [5, 4096 + 9], [0, 1], [1, 1], 4096)
    assert list(offsets) == [0, 100] and list(sizes) == [100, 100] and blob.size == 200 and list(blob[100:]) == [7] * 100
    assert begin == [5, 4096 + 9] and limit == [1, 2]


def test_kernel_unit_is_in_the_code_object(pkg):
    pkg.build()
    so = open(pkg.lib_path(), "rb").read()
    assert b"alac_clips_gather" in so and b"alac_clips_meta" in so
