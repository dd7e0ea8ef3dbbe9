"""alac_clips_gather and alac_clips_meta on the GPU over the geometry of tests/test_clips_host.py: the same slots, descriptors
and parameters (the shared lists of tests/clip_ref.py, with the same seeds), so that what the host build of csrc/alac_clips.h
runs one work item after the other, the device runs with its barrier, its LDS and its 16-byte accesses at real alignments.

The slots are written by hand and uploaded to a buffer of exactly pcm_mis + n * pcm_stride bytes, the first slot pcm_mis bytes
behind a 16-byte boundary; no decode runs in front (but for the last test). Every gather writes into a sentinel-filled buffer
with the tensor `base` elements behind a 16-byte boundary and odd strides, and the WHOLE buffer is compared bit for bit with
clip_ref.ref_clips / clip_ref.expected_image; valid[] and clip_status[] are prefilled with -1 and an output that was not asked
for must still be all -1. Each test asserts on its own inputs that the geometry it is there for is reached (clip_ref.
tile_geometry: make_params' and make_tile's numbers from the tile_cols the header chose).

No test provokes a fault: the hostile frame counts are values the kernel clamps, which keeps every read inside the slots; the
slots that end at an inaccessible page stay on the CPU."""
import numpy as np
import pytest

from tests import clip_ref as cr
from tests import wave_ref as wr
from tests.test_gpu_clips import assert_image, descriptors, gather, u64_tensor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture(scope="module")
def sim():
    return cr.build_clip_sim()


@pytest.fixture(scope="module")
def decoders(pkg):
    """One handle per (FL, depth, channels), kept for the module"""
    made = {}

    def get(fl, depth, ch):
        if (fl, depth, ch) not in made:
            made[(fl, depth, ch)] = pkg.NewPacketDecoder(pkg.PacketConfig(FrameLength=fl, BitDepth=depth, NumChannels=ch), 0)
        return made[(fl, depth, ch)]

    yield get
    for dec in made.values():
        dec.close()


def raw_gather(torch, dec, fl, depth, ch, out, frames, status, begin, limit, L, wtype, base=0, slack=None, pcm_mis=0, want_valid=True,
               want_status=True):
    """Hand-written slots uploaded pcm_mis bytes behind a 16-byte boundary, into a buffer that ends with the last slot's stride;
    one gather with sync=True into a sentinel-filled buffer whose tensor starts 8 + base elements in, rows an odd stride apart
    -> (image uint32, lead, cs, ps, valid int32, clip_status int32), the last two -1 where they were not passed"""
    dev = torch.device("cuda:0")
    n, stride = out.shape
    d_pcm = torch.empty(pcm_mis + n * stride, dtype=torch.uint8, device=dev)
    assert d_pcm.data_ptr() % 16 == 0
    d_pcm[:pcm_mis] = 0xEE
    d_pcm[pcm_mis:] = torch.from_numpy(np.ascontiguousarray(out).reshape(-1)).to(dev)
    d_fr = torch.from_numpy(np.ascontiguousarray(frames, np.uint32).view(np.int32)).to(dev)
    d_st = None if status is None else torch.from_numpy(np.ascontiguousarray(status, np.int32)).to(dev)
    B = len(begin)
    cs = L + (slack if slack is not None else 1 + L % 2)  # odd
    ps = ch * cs + 3
    lead = 8 + base
    buf = torch.full((lead + B * ps + 8,), wr.SENTINEL - (1 << 32), dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0
    d_begin, d_limit = u64_tensor(torch, begin, dev), u64_tensor(torch, limit, dev)
    d_valid = torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_cst = torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    dec.clips_device(d_pcm.data_ptr() + pcm_mis, stride, d_fr.data_ptr(), None if d_st is None else d_st.data_ptr(), n, d_begin.data_ptr(),
                     d_limit.data_ptr(), B, L, wtype, buf.data_ptr() + 4 * lead, cs, ps, d_valid.data_ptr() if want_valid else None,
                     d_cst.data_ptr() if want_status else None, sync=True)
    return buf.cpu().numpy().view(np.uint32), lead, cs, ps, d_valid.cpu().numpy(), d_cst.cpu().numpy()


def check(torch, decoders, fl, depth, ch, out, frames, status, begin, limit, L, wtype, **kw):
    img, lead, cs, ps, valid, cstat = raw_gather(torch, decoders(fl, depth, ch), fl, depth, ch, out, frames, status, begin, limit, L, wtype, **kw)
    ref, r_valid, r_cstat = cr.ref_clips(out, frames, status, fl, depth, ch, wtype, begin, limit, L)
    assert_image(img, cr.expected_image(ref, img.size, lead, cs, ps), lead)
    if kw.get("want_valid", True):
        assert np.array_equal(valid.view(np.uint32), r_valid), (valid, r_valid)
    else:
        assert np.all(valid == -1)
    if kw.get("want_status", True):
        assert np.array_equal(cstat, r_cstat), (cstat, r_cstat)
    else:
        assert np.all(cstat == -1)
    return ref, r_valid, r_cstat


def test_the_shared_lists_reach_the_geometry_the_device_has_not_run(sim):
    """Across the grid and the added geometries: a tile of more than 256 segments (the second turn of the segment-entry loop), the
    smallest pitch (3 chunks: stage_dq 85, stage_dr 1), two tiles per clip at 8 x 32 bits, clips shorter than a quad."""
    geos = cr.list_geometries(sim.clip_sim_tile_cols)
    assert len(geos) == 3 * len(cr.GRID_FL) * len(cr.GRID_L) + len(cr.ADDED)
    assert max(g["nseg"] for g in geos.values()) == 334 and sum(g["nseg"] > 256 for g in geos.values()) >= 4
    assert min(g["chunks"] for g in geos.values()) == 3 and 256 // 3 == 85 and 256 % 3 == 1
    assert geos[(32, 8, 4096, 257)]["tile_cols"] == 256 and geos[(32, 8, 4096, 257)]["tiles_per_clip"] == 2
    assert {k[3] for k in geos if k[3] < 4} == {1, 3}
    assert {g["chunks"] for k, g in geos.items() if k[2] in (2, 3, 16)} == {3, 4, 6, 20, 34}


@pytest.mark.parametrize("L", cr.GRID_L)
@pytest.mark.parametrize("fl", cr.GRID_FL)
def test_frame_lengths_and_clip_lengths(torch, decoders, sim, fl, L):
    """The host test's full grid for (16, 2, FLOAT), (32, 8, INT) and (24, 6, FLOAT)."""
    runs = list(cr.grid_runs(fl, L))
    assert [(r.depth, r.ch, r.wtype) for r in runs] == list(cr.GRID_FORMATS)
    for run in runs:
        geo = run.geometry(sim.clip_sim_tile_cols(fl, run.depth, run.ch))
        assert len(run.out) <= 1200 and len(run.begin) <= 36 and geo["nseg"] * geo["chunks"] * 16 <= sim.clip_sim_stage_bytes()
        if fl == 1:
            assert geo["chunks"] == (3 if run.ch == 2 else 4) and geo["nseg"] == (geo["tile_cols"] + 3 if L == 1000 else min(L, geo["tile_cols"]))
        if (run.depth, run.ch) == (32, 8):
            assert geo["tile_cols"] == 256 and geo["tiles_per_clip"] == -(-L // 256)
        check(torch, decoders, *run.args(), **run.kw)


ADDED_GEOMETRY = {(32, 1, 7, 2100): dict(tile_cols=2048, tiles_per_clip=2, chunks=4, nseg=294),
                  (16, 1, 3, 1000): dict(tile_cols=1024, tiles_per_clip=1, chunks=3, nseg=334),
                  (24, 3, 2, 900): dict(tile_cols=448, tiles_per_clip=3, chunks=4, nseg=226),
                  (16, 1, 1, 300): dict(tile_cols=256, tiles_per_clip=2, chunks=3, nseg=256)}


@pytest.mark.parametrize("depth,ch,fl,L", cr.ADDED)
def test_added_geometries(torch, decoders, sim, depth, ch, fl, L):
    """294 and 334 segments in one tile, FL 2 with three channels, FL 1 at the smallest pitch; both element types."""
    runs = list(cr.added_runs(depth, ch, fl, L))
    assert runs[0].geometry(sim.clip_sim_tile_cols(fl, depth, ch)) == ADDED_GEOMETRY[(depth, ch, fl, L)]
    assert [r.wtype for r in runs] == [wr.FLOAT, wr.INT] and len(runs[0].out) <= 1200
    for run in runs:
        check(torch, decoders, *run.args(), **run.kw)


@pytest.mark.parametrize("depth,ch,fl,L", cr.ALIGN_CASES)
def test_every_alignment_gives_the_same_values(torch, decoders, depth, ch, fl, L):
    """The host test's five configurations: slots (pcm_mis, extra stride) of (0, 0), (5, 3) and (8, 16), base 0..3, begin of every
    residue mod 4 next to a slot boundary, both element types."""
    runs = list(cr.alignment_runs(depth, ch, fl, L))
    fb = fl * ch * wr.BPS[depth]
    assert sorted({(r.kw["pcm_mis"], r.out.shape[1] - (fb + 15) // 16 * 16) for r in runs}) == sorted(cr.ALIGN_PCM)
    assert {r.kw["base"] for r in runs} == {0, 1, 2, 3} and {r.wtype for r in runs} == {wr.FLOAT, wr.INT}
    assert all({b % 4 for b in r.begin[:4]} == {0, 1, 2, 3} and r.begin[0] == fl for r in runs)
    assert any((r.kw["pcm_mis"] + r.out.shape[1]) % 16 for r in runs), "no slot off a 16-byte boundary"
    for run in runs:
        check(torch, decoders, *run.args(), **run.kw)


@pytest.mark.parametrize("depth,ch,fl,L", cr.EXACT_CASES)
def test_stride_of_exactly_the_frame_bytes_and_a_short_last_slot(torch, decoders, depth, ch, fl, L):
    """The slots of the host's inaccessible-page test, here inside a buffer of exactly pcm_mis + n * pcm_stride bytes: nothing
    between two slots, the last one short, clips at and over the batch's end."""
    n = cr.EXACT_SLOTS
    out, frames, status, begin = cr.exact_stride_case(depth, ch, fl, L)
    assert out.shape == (n, fl * ch * wr.BPS[depth]) and frames[n - 1] == max(fl - 3, 1)
    for k, (wtype, pcm_mis) in enumerate(((wr.FLOAT, 0), (wr.INT, 0), (wr.FLOAT, 7), (wr.INT, 2))):
        check(torch, decoders, fl, depth, ch, out, frames, status, begin, [n] * len(begin), L, wtype, base=k, pcm_mis=pcm_mis)


def test_null_status_valid_and_clip_status(torch, decoders):
    """The host test's four combinations: alac_clips_meta with one null output, and not launched at all."""
    runs = list(cr.null_runs())
    assert [(r.status is None, r.kw.get("want_valid", True), r.kw.get("want_status", True)) for r in runs] == [
        (True, True, True), (False, False, True), (False, True, False), (True, False, False)]
    for run in runs:
        ref, r_valid, r_cstat = check(torch, decoders, *run.args(), **run.kw)
        if run.status is None:  # a failed slot's bytes show, and clip_status is 0
            masked, m_valid, m_cstat = cr.ref_clips(run.out, run.frames, runs[1].status, run.fl, run.depth, run.ch, run.wtype, run.begin, run.limit,
                                                    run.L)
            assert not r_cstat.any() and m_cstat.any() and (r_valid > m_valid).any() and not np.array_equal(ref, masked)


def test_hostile_frame_counts_are_clamped(torch, decoders):
    """d_frames of FL + 5 and 0xFFFFFFFF with no status words, the slots' buffer exactly n * pcm_stride bytes: the clamp to FL
    keeps every read inside it (the entry's contract)."""
    run = cr.hostile_run()
    n = len(run.frames)
    assert run.frames[n // 3] == run.fl + 5 and run.frames[(2 * n) // 3] == 0xFFFFFFFF and run.status is None
    assert run.out.shape[1] == run.fl * run.ch * wr.BPS[run.depth] and not run.kw
    ref, valid, _ = check(torch, decoders, *run.args())
    assert valid.max() <= run.L


def test_short_and_failed_slots_leave_a_zero_gap(torch, decoders):
    """Worked by hand: slot 1 holds 5 of 16 frames, slot 2 failed with a frame count left standing."""
    fl, depth, ch, n, L, out, frames, status = cr.short_and_failed_case()
    ref, valid, cstat = check(torch, decoders, fl, depth, ch, out, frames, status, [8, 0, 40], [n, n, n], L, wr.FLOAT)
    assert list(valid) == [8 + 5 + 0 + 8, 16 + 5 + 0, 0 + 16] and list(cstat) == [0x1101, 0x1101, 0x1101]
    assert not ref[0, :, 8 + 5:8 + 32].any() and not ref[2, :, :8].any() and not ref[2, :, 24:].any()
    _, valid, cstat = check(torch, decoders, fl, depth, ch, out, frames, None, [8], [n], L, wr.INT)
    assert list(valid) == [8 + 5 + 16 + 8] and list(cstat) == [0]


def test_limit_cuts_a_clip(torch, decoders):
    fl, depth, ch, n, L, out, frames, status, begin, limit = cr.limit_case()
    ref, valid, cstat = check(torch, decoders, fl, depth, ch, out, frames, status, begin, limit, L, wr.INT)
    assert list(valid) == [40 - 12, 28, 12, 0, 0, 0] and list(cstat) == [7, 0, 0, 0, 0, 0]
    assert ref[1, :, :28].any() and not ref[1, :, 28:].any() and not ref[3].any()


@pytest.mark.parametrize("depth,ch,fl,n,seed,Ls", [(20, 8, 16, 40, 52, (256, 3)), (16, 1, 1, 400, 17, (300,))])
def test_gather_behind_an_unsynchronized_decode(torch, pkg, oracle, synth, helpers, depth, ch, fl, n, seed, Ls):
    """tests/test_gpu_clips.py's test at FL 16 and FL 1: the slots come from a real decode with sync=False on the same stream. The
    packet list's seed at FL 16 is one that puts a damaged packet under a clip of 3 frames, which the test asserts."""
    cfg = oracle.make_config(fl, depth, ch)
    b = cr.Batch(torch, oracle, helpers, cfg, cr.packet_list(synth, helpers, cfg, n, seed, damaged=3))
    out, r_frames, r_status = b.ref
    assert (r_status != 0).any() and (fl == 1 or (r_frames < fl).any())
    with pkg.NewPacketDecoder(cr.to_pkg_cfg(pkg, cfg), 0) as dec:
        for L in Ls:
            begin, limit = descriptors(b.n, fl, L)
            for wtype in (wr.FLOAT, wr.INT):
                ref, r_valid, r_cst = cr.ref_clips(out, r_frames, r_status, fl, depth, ch, wtype, begin, limit, L)
                assert r_valid.max() > L // 2 and r_valid.min() == 0 and r_cst.any()
                for base in range(4):
                    img, lead, cs, ps, valid, cst, frames, status = gather(torch, dec, b, begin, limit, L, wtype, base,
                                                                           slack=1 + L % 2 if base else 0)
                    assert np.array_equal(status, r_status) and np.array_equal(frames, r_frames)
                    assert_image(img, cr.expected_image(ref, img.size, lead, cs, ps), lead)
                    assert np.array_equal(valid, r_valid) and np.array_equal(cst, r_cst)
        assert dec.clips_last_ms() > 0 and dec.last_kernel_ms() > 0
