"""The clip gather on the CPU: csrc/alac_clips.h built with g++ (tests/host_sim/clip_sim.cpp), tile for tile and work item
for work item what the gfx950 kernel of k_clips.hip runs, against the numpy restatement of tests/clip_ref.py.

Every run writes into a sentinel-filled buffer with slack in both strides and guard elements in front and behind, and the
WHOLE buffer is compared bit for bit: the values, the zeros, and every element outside the [clip][channel] rows still the
sentinel. The slots are written by hand (wave_ref.hand_slots): random bytes behind a slot's frames and in failed slots,
which must not show.

The inputs come from the lists of tests/clip_ref.py, which tests/test_gpu_clip_geometry.py runs on the device.

* depths 16/20/24/32 x FLOAT/INT x channels 1/2/6/8; frame lengths 1/7/16/33/4096 x clip lengths 1/3/255/256/257/1000;
* tiles of 294 and 334 segments (FL 7 and 3), FL 2 with three channels, FL 1 at the smallest pitch (clip_ref.ADDED);
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
U64 = cr.U64


@pytest.fixture(scope="module")
def sim():
    return cr.build_clip_sim()


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


@pytest.mark.parametrize("ch", cr.CHANNELS)
@pytest.mark.parametrize("depth", cr.DEPTHS)
def test_host_build_equals_numpy_over_depths_and_channels(sim, depth, ch):
    for run in cr.depth_channel_runs(depth, ch):
        check(sim, *run.args(), **run.kw)


@pytest.mark.parametrize("L", cr.GRID_L)
@pytest.mark.parametrize("fl", cr.GRID_FL)
def test_frame_lengths_and_clip_lengths(sim, fl, L):
    """Clips inside one slot, over many slots, and longer than a tile (8-channel 32-bit tiles are 256 columns, fewer at the
    smallest frame lengths)."""
    runs = list(cr.grid_runs(fl, L))
    assert [(r.depth, r.ch, r.wtype) for r in runs] == list(cr.GRID_FORMATS)
    for run in runs:
        check(sim, *run.args(), **run.kw)


@pytest.mark.parametrize("depth,ch,fl,L", cr.ADDED)
def test_added_geometries(sim, depth, ch, fl, L):
    """More than 256 segments in one tile (the second turn of the segment-entry loop), FL 2 with three channels, and the
    smallest pitch, three chunks; each case reaches what it is there for."""
    runs = list(cr.added_runs(depth, ch, fl, L))
    geo = runs[0].geometry(sim.clip_sim_tile_cols(fl, depth, ch))
    want = {(32, 1, 7, 2100): dict(tile_cols=2048, tiles_per_clip=2, chunks=4, nseg=294),
            (16, 1, 3, 1000): dict(tile_cols=1024, tiles_per_clip=1, chunks=3, nseg=334),
            (24, 3, 2, 900): dict(tile_cols=448, tiles_per_clip=3, chunks=4, nseg=226),
            (16, 1, 1, 300): dict(tile_cols=256, tiles_per_clip=2, chunks=3, nseg=256)}[(depth, ch, fl, L)]
    assert geo == want, geo
    for run in runs:
        check(sim, *run.args(), **run.kw)


def test_the_shared_lists_reach_the_geometry_they_are_there_for(sim):
    """Across the grid and the added geometries: a tile of more than 256 segments, the 3-chunk pitch, two tiles per clip at 8 x 32
    bits, clips shorter than a quad; and the staging of every one of them fits the segment table."""
    geos = cr.list_geometries(sim.clip_sim_tile_cols)
    assert max(g["nseg"] for g in geos.values()) > 256 and geos[(16, 2, 1, 1000)]["nseg"] == 259
    assert min(g["chunks"] for g in geos.values()) == 3 and geos[(16, 2, 1, 256)]["chunks"] == 3
    assert geos[(32, 8, 4096, 257)]["tile_cols"] == 256 and geos[(32, 8, 4096, 257)]["tiles_per_clip"] == 2
    assert any(k[3] < 4 for k in geos)
    assert all(g["nseg"] * g["chunks"] * 16 <= sim.clip_sim_stage_bytes() for g in geos.values())


@pytest.mark.parametrize("depth,ch,fl,L", cr.ALIGN_CASES)
def test_every_alignment_gives_the_same_values(sim, depth, ch, fl, L):
    """Every begin % 4 with every base offset of 0..3 elements, odd channel and clip strides, slots at odd byte alignments."""
    runs = list(cr.alignment_runs(depth, ch, fl, L))
    assert len(runs) == 24
    for run in runs:
        check(sim, *run.args(), **run.kw)


def test_short_and_failed_slots_leave_a_zero_gap(sim):
    """Worked by hand: slot 1 holds 5 of 16 frames, slot 2 failed with a frame count left standing."""
    fl, depth, ch, n, L, out, frames, status = cr.short_and_failed_case()
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
    fl, depth, ch, n, L, out, frames, status, begin, limit = cr.limit_case()
    ref, valid, cstat = check(sim, fl, depth, ch, out, frames, status, begin, limit, L, wr.INT)
    # the failed slot 3 is touched only under the full limit; a limit at or below the clip's first slot leaves nothing
    assert list(valid) == [40 - 12, 28, 12, 0, 0, 0] and list(cstat) == [7, 0, 0, 0, 0, 0]
    assert ref[1, :, :28].any() and not ref[1, :, 28:].any() and not ref[3].any()


@pytest.mark.parametrize("depth,ch,fl,L", cr.PAST_CASES)
def test_descriptors_at_and_past_the_batch(sim, depth, ch, fl, L):
    """begin at, just before and past n * frame_length and at the top of 64 bits; limit 0 and above n: zeros where the grid
    has no slot, no read outside the slots."""
    rng = np.random.default_rng(L)
    n = 5
    out, frames, status = cr.slots(rng, n, fl, depth, ch, failed=(1,))
    total = n * fl
    begin = [total - 1, total, total + 1, max(total - L, 0), max(total - L, 0) + 1, total + L, U64, U64 - 1, U64 - L, U64 - L + 1, 1 << 63, (1 << 63) - 1,
             (1 << 32) - 1, 1 << 32, 0, 0, 0, 3, fl]
    limit = [n] * 14 + [0, n + 7, U64, U64, 1 << 32]
    for wtype in (wr.FLOAT, wr.INT):
        ref, valid, _ = check(sim, fl, depth, ch, out, frames, status, begin, limit, L, wtype)
    assert not ref[1].any() and not ref[6].any() and not ref[14].any() and valid[1] == valid[6] == valid[14] == 0
    assert np.array_equal(ref[15], ref[16]) and valid[15] > 0


def test_hostile_frame_counts_are_clamped(sim):
    run = cr.hostile_run()
    assert run.frames[len(run.frames) // 3] == run.fl + 5 and run.frames[(2 * len(run.frames)) // 3] == 0xFFFFFFFF and run.status is None
    ref, valid, _ = check(sim, *run.args(), **run.kw)
    assert valid.max() <= run.L


def test_null_status_valid_and_clip_status(sim):
    runs = list(cr.null_runs())
    assert [(r.status is None, r.kw.get("want_valid", True), r.kw.get("want_status", True)) for r in runs] == [
        (True, True, True), (False, False, True), (False, True, False), (True, False, False)]
    for run in runs:
        check(sim, *run.args(), **run.kw)


def test_no_clips_and_no_packets(sim):
    rng = np.random.default_rng(7)
    fl, depth, ch, L = 33, 16, 2, 70
    out, frames, status = cr.slots(rng, 4, fl, depth, ch)
    img, lead, cs, ps, _, _ = run_sim(sim, fl, depth, ch, out, frames, status, [], [], L, wr.FLOAT)
    assert np.all(img == wr.SENTINEL)  # nothing is touched
    assert sim.clip_sim_run(fl, depth, ch, None, 0, None, None, 0, None, None, 0, L, wr.FLOAT, None, 0, 0, None, None, 0) == 0
    # clips over an empty batch are zeros
    ref, valid, cstat = check(sim, fl, depth, ch, None, np.zeros(0, np.uint32), np.zeros(0, np.int32), [0, 5, U64], [0, 9, U64], L, wr.INT)
    assert not ref.any() and not valid.any() and not cstat.any()


@pytest.mark.parametrize("depth,ch,fl,L", cr.EXACT_CASES)
def test_slots_that_end_at_an_inaccessible_page(sim, depth, ch, fl, L):
    """pcm_stride exactly the frame bytes and a short last slot, whose last frame's last byte is the last accessible one: a read
    behind a slot's frames that leaves the buffer is fatal here."""
    n = cr.EXACT_SLOTS
    out, frames, status, begin = cr.exact_stride_case(depth, ch, fl, L)
    bpf = ch * wr.BPS[depth]
    assert out.shape == (n, fl * bpf) and frames[n - 1] == max(fl - 3, 1)
    guard = (n - 1) * out.shape[1] + int(frames[n - 1]) * bpf
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
