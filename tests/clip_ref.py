"""TEST HELPER for the clip gather (alacgpu_clips_device): the numpy restatement every comparison uses, the expected image
of a whole clips buffer, sentinel included, the host build of csrc/alac_clips.h (tests/host_sim/clip_sim.cpp), the case lists
the CPU and the GPU suite share (slots, descriptors and parameters of every gather of raw slots), and the packet lists and
files the GPU tests decode.

The restatement imports nothing of the code under test. It starts from decoded slots (out[n, stride] uint8, frames, status
— the oracle's triple, or slots a test wrote by hand) and follows the definition in include/alacgpu.h with Python integers,
so that no descriptor wraps around: slot i is the frames [i * fl, (i + 1) * fl) of a grid; column t of clip j is grid frame
begin[j] + t, a sample when that does not overflow, its slot lies below min(limit[j], n) and its frame below the slot's f,
zero otherwise. Samples are unpacked and converted by tests/wave_ref.py. All comparisons are bit-exact."""
import ctypes

import numpy as np

from tests import host_build
from tests import wave_ref as wr

SENTINEL = wr.SENTINEL


def ref_clips(out, frames, status, fl, depth, ch, wtype, begin, limit, L):
    """-> (clips uint32 [B, ch, L], valid uint32 [B], clip_status int32 [B])"""
    n = len(frames)
    f = [int(x) for x in wr.frames_used(frames, status, fl)] if n else []
    B = len(begin)
    clips = np.zeros((B, ch, L), np.uint32)
    valid = np.zeros(B, np.uint32)
    cstat = np.zeros(B, np.int32)
    cache = {}
    for j in range(B):
        b, lim = int(begin[j]), min(int(limit[j]), n)
        t = 0
        while t < L:
            g = b + t
            if g >= 1 << 64:
                break  # overflow: this column and all behind it
            i, r = divmod(g, fl)
            if i >= lim:
                break  # slots grow with t: nothing behind this column either
            take = min(fl - r, L - t, (1 << 64) - g)  # columns of this clip in slot i
            if status is not None and cstat[j] == 0 and int(status[i]) != 0:
                cstat[j] = status[i]
            have = max(0, min(f[i], r + take) - r)
            if have:
                if i not in cache:
                    cache[i] = wr.elements(wr.unpack(out[i], f[i], depth, ch), depth, wtype)
                clips[j, :, t:t + have] = cache[i][r:r + have].T
                valid[j] += have
            t += take
    return clips, valid, cstat


def expected_image(ref, elems, base, cs, ps):
    """The whole clips buffer (`elems` uint32 elements, the tensor starting at element `base`, rows cs apart, clips ps apart)
    as the gather must leave it when it was filled with SENTINEL before: the [B][ch] rows at their place, the sentinel
    everywhere else."""
    img = np.full(elems, SENTINEL, np.uint32)
    B, ch, L = ref.shape
    for j in range(B):
        for c in range(ch):
            o = base + j * ps + c * cs
            img[o:o + L] = ref[j, c]
    return img


def build_clip_sim():
    L = host_build.shared("clip_sim.cpp", "libclip_sim.so", host_build.SIM)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.clip_sim_run.argtypes = [u32, u32, u32, vp, u64, vp, vp, u64, vp, vp, u64, u32, ctypes.c_int, vp, u64, u64, vp, vp, u64]
    for fn in (L.clip_sim_tile_cols, L.clip_sim_stage_need):
        fn.restype, fn.argtypes = u32, [u32, u32, u32]
    L.clip_sim_stage_bytes.restype = u32
    return L


# ---- the cases, shared by the CPU and the GPU suite ------------------------------------------------------------------------
# What the host build of alac_clips.h runs (tests/test_clips_host.py), the device runs too (tests/test_gpu_clip_geometry.py): both
# draw their slots, descriptors and parameters from here, with the same seeds.
U64 = (1 << 64) - 1


def slots(rng, n, fl, depth, ch, pattern="short", failed=(), extra=0, exact=False):
    """(out, frames, status): hand-written slots; the stride the decode's fast one plus `extra`, or exactly the frame bytes."""
    fb = fl * ch * wr.BPS[depth]
    stride = fb if exact else (fb + 15) // 16 * 16 + extra
    frames = wr.frame_counts(rng, n, fl, pattern)
    status = np.zeros(n, np.int32)
    for k, i in enumerate(failed):
        status[i] = (0x1101, 3, 0x2202)[k % 3]
    return wr.hand_slots(rng, n, fl, depth, ch, stride, frames), frames, status


def spread(rng, n, fl, L):
    """Clip descriptors all over a batch of n slots: in one slot, across slot boundaries, over the short and failed slots in
    the middle, at the batch's end, and a few at random -> (begin, limit)."""
    total = n * fl
    begin = [0, 1, 2, 3, fl - 1, fl, fl + 1, max(total // 2 - L // 2, 0), max(total - L, 0), max(total - L, 0) + 1, total - 1]
    begin += [int(x) for x in rng.integers(0, total, 5)]
    limit = [n] * len(begin)
    return begin, limit


class Run:
    """One gather: the slots, the descriptors, and how the buffers lie (base, slack, pcm_mis, want_valid, want_status)."""

    def __init__(self, fl, depth, ch, out, frames, status, begin, limit, L, wtype, **kw):
        self.fl, self.depth, self.ch, self.out, self.frames, self.status = fl, depth, ch, out, frames, status
        self.begin, self.limit, self.L, self.wtype, self.kw = begin, limit, L, wtype, kw

    def args(self):
        return (self.fl, self.depth, self.ch, self.out, self.frames, self.status, self.begin, self.limit, self.L, self.wtype)

    def geometry(self, tile_cols):
        return tile_geometry(tile_cols, self.fl, self.depth, self.ch, self.L, self.begin, self.limit, len(self.out))


def tile_geometry(tile_cols, fl, depth, ch, L, begin, limit, n):
    """make_params' and make_tile's numbers for one gather, restated with Python integers from the tile_cols the header chose
    (clip_sim_tile_cols) -> dict(tile_cols, tiles_per_clip, chunks, nseg): chunks = pitch / 16 with pitch = round16(min(FL,
    tile_cols + 3) x bytes per frame) + 32; nseg the most segments any tile of any clip stages."""
    bpf = ch * wr.BPS[depth]
    pitch = (min(fl, tile_cols + 3) * bpf + 15) // 16 * 16 + 32
    tiles = -(-L // tile_cols)
    nseg = 0
    for b, lim in zip(begin, limit):
        end = max(0, min(min(int(lim), n) * fl - int(b), L))
        for tile in range(tiles):
            t0 = tile * tile_cols
            lo, hi = max(t0 - 3, 0), min(t0 + tile_cols, end)
            if hi > lo:
                last = (int(b) + lo) % fl + hi - lo - 1
                nseg = max(nseg, 1 if last < fl else 2 + (last - fl) // fl)
    return dict(tile_cols=tile_cols, tiles_per_clip=tiles, chunks=pitch // 16, nseg=nseg)


DEPTHS, CHANNELS = [16, 20, 24, 32], [1, 2, 6, 8]


def depth_channel_runs(depth, ch):
    rng = np.random.default_rng(depth * 10 + ch)
    fl, n, L = 33, 12, 100
    out, frames, status = slots(rng, n, fl, depth, ch, failed=(4,))
    begin, limit = spread(rng, n, fl, L)
    for wtype in (wr.FLOAT, wr.INT):
        yield Run(fl, depth, ch, out, frames, status, begin, limit, L, wtype)


# frame lengths x clip lengths: clips inside one slot, over many slots, and longer than a tile
GRID_FL, GRID_L = [1, 7, 16, 33, 4096], [1, 3, 255, 256, 257, 1000]
GRID_FORMATS = ((16, 2, wr.FLOAT), (32, 8, wr.INT), (24, 6, wr.FLOAT))
# (depth, channels, FL, L) for what the grid leaves out: more than 256 segments in a tile at FL 7 and FL 3 (294 and 334: the second
# turn of the segment-entry loop), FL 2 with three channels, and the smallest pitch there is (FL 1, 16-bit mono: 3 chunks)
ADDED = [(32, 1, 7, 2100), (16, 1, 3, 1000), (24, 3, 2, 900), (16, 1, 1, 300)]


def grid_slots(fl, L):
    return max(3, min(1200, (L + 300) // fl + 3))


def grid_runs(fl, L):
    rng = np.random.default_rng(fl * 1000 + L)
    n = grid_slots(fl, L)
    for depth, ch, wtype in GRID_FORMATS:
        out, frames, status = slots(rng, n, fl, depth, ch, failed=(n // 2 + 1,) if n > 4 else ())
        begin, limit = spread(rng, n, fl, L)
        yield Run(fl, depth, ch, out, frames, status, begin, limit, L, wtype)


def added_runs(depth, ch, fl, L):
    rng = np.random.default_rng(depth * 100000 + ch * 10000 + fl * 1000 + L)
    n = grid_slots(fl, L)
    out, frames, status = slots(rng, n, fl, depth, ch, failed=(n // 2 + 1,))
    begin, limit = spread(rng, n, fl, L)
    for wtype in (wr.FLOAT, wr.INT):
        yield Run(fl, depth, ch, out, frames, status, begin, limit, L, wtype)


def list_geometries(tile_cols_of):
    """(depth, channels, FL, L) -> tile_geometry of every grid case and every added one, over spread()'s descriptors (the random
    ones among them do not matter: begin 0..3 and FL - 1 are there); tile_cols_of is clip_sim_tile_cols"""
    cases = [(depth, ch, fl, L) for fl in GRID_FL for L in GRID_L for depth, ch, _ in GRID_FORMATS] + ADDED
    geos = {}
    for depth, ch, fl, L in cases:
        n = grid_slots(fl, L)
        begin, limit = spread(np.random.default_rng(0), n, fl, L)
        geos[(depth, ch, fl, L)] = tile_geometry(tile_cols_of(fl, depth, ch), fl, depth, ch, L, begin, limit, n)
    return geos


# every begin % 4 next to a slot boundary x every base offset of 0..3 elements x both types, odd channel and clip strides, the
# slots (pcm_mis, extra stride) off a 16-byte boundary
ALIGN_CASES = [(16, 2, 33, 257), (24, 6, 7, 255), (32, 1, 4096, 1000), (20, 8, 16, 256), (16, 1, 1, 300)]
ALIGN_PCM = ((0, 0), (5, 3), (8, 16))


def align_slots(fl, L):
    return max(4, (L + 40) // fl + 3)


def alignment_runs(depth, ch, fl, L):
    rng = np.random.default_rng(depth + ch + fl)
    n = align_slots(fl, L)
    for pcm_mis, extra in ALIGN_PCM:
        out, frames, status = slots(rng, n, fl, depth, ch, pattern="odd", failed=(2,), extra=extra)
        for base in range(4):
            begin = [fl + b for b in range(4)] + [5 * b for b in range(4)]
            for wtype, slack in ((wr.FLOAT, None), (wr.INT, 3 + L % 2)):
                yield Run(fl, depth, ch, out, frames, status, begin, [n] * len(begin), L, wtype, base=base, slack=slack, pcm_mis=pcm_mis)


# pcm_stride exactly the frame bytes and a short last slot
EXACT_CASES = [(16, 2, 33, 100), (24, 3, 7, 257), (32, 8, 64, 300), (16, 1, 4096, 1000)]
EXACT_SLOTS = 6


def exact_stride_case(depth, ch, fl, L):
    """-> (out, frames, status, begin): the last slot holds max(FL - 3, 1) frames; clips at and over the batch's end"""
    rng = np.random.default_rng(fl)
    n = EXACT_SLOTS
    out, frames, status = slots(rng, n, fl, depth, ch, failed=(2,), exact=True)
    frames[n - 1] = max(fl - 3, 1)
    total = n * fl
    begin = [max(total - L, 0), max(total - L // 2, 0), total - 1, total - 3, total, 0, (n - 1) * fl, U64]
    return out, frames, status, begin


PAST_CASES = [(16, 2, 33, 100), (32, 8, 7, 257), (24, 1, 4096, 5000)]


def hostile_run():
    """d_frames of FL + 5 and 0xFFFFFFFF, no status words"""
    rng = np.random.default_rng(5)
    fl, depth, ch, n, L = 100, 16, 2, 12, 333
    out, frames, _ = slots(rng, n, fl, depth, ch, pattern="hostile")
    assert frames[n // 3] == fl + 5 and frames[(2 * n) // 3] == 0xFFFFFFFF
    begin, limit = spread(rng, n, fl, L)
    return Run(fl, depth, ch, out, frames, None, begin, limit, L, wr.FLOAT)


def null_runs():
    """NULL d_status, d_valid, d_clip_status, and all three"""
    rng = np.random.default_rng(6)
    fl, depth, ch, n, L = 33, 24, 2, 9, 257
    out, frames, status = slots(rng, n, fl, depth, ch, pattern="odd", failed=(3,))
    begin, limit = spread(rng, n, fl, L)
    yield Run(fl, depth, ch, out, frames, None, begin, limit, L, wr.FLOAT)
    yield Run(fl, depth, ch, out, frames, status, begin, limit, L, wr.INT, want_valid=False)
    yield Run(fl, depth, ch, out, frames, status, begin, limit, L, wr.INT, want_status=False)
    yield Run(fl, depth, ch, out, frames, None, begin, limit, L, wr.FLOAT, want_valid=False, want_status=False)


def short_and_failed_case():
    """Worked by hand: slot 1 holds 5 of 16 frames, slot 2 failed with a frame count left standing -> (fl, depth, ch, n, L, out,
    frames, status)"""
    rng = np.random.default_rng(1)
    fl, depth, ch, n, L = 16, 16, 2, 4, 48
    frames = np.array([16, 5, 16, 16], np.uint32)
    status = np.array([0, 0, 0x1101, 0], np.int32)
    return fl, depth, ch, n, L, wr.hand_slots(rng, n, fl, depth, ch, fl * ch * 2, frames), frames, status


def limit_case():
    """Worked by hand: slot 3 failed, limits from n down to 0 -> (fl, depth, ch, n, L, out, frames, status, begin, limit)"""
    rng = np.random.default_rng(2)
    fl, depth, ch, n, L = 16, 24, 2, 6, 40
    frames = np.full(n, fl, np.uint32)
    status = np.zeros(n, np.int32)
    status[3] = 7
    out = wr.hand_slots(rng, n, fl, depth, ch, fl * ch * 3, frames)
    return fl, depth, ch, n, L, out, frames, status, [20, 20, 20, 20, 20, 50], [n, 3, 2, 1, 0, 3]


# ---- packets and files for the GPU tests ---------------------------------------------------------------------------------
SHIFT ={16: 0, 20: 0, 24: 1, 32: 2}


def to_pkg_cfg(pkg, ocfg):
    return pkg.PacketConfig(FrameLength=ocfg.frame_length, BitDepth=ocfg.bit_depth, NumChannels=ocfg.num_channels,
                            PB=ocfg.pb, MB=ocfg.mb, KB=ocfg.kb, MaxRun=ocfg.max_run, SampleRate=ocfg.sample_rate)


def short_packet(synth, cfg, frames, seed, escape):
    ne = synth.num_elements(cfg.num_channels)
    kw = dict(force_escape=1) if escape else dict(never_escape=1, bytes_shifted=SHIFT[cfg.bit_depth])
    pcm = synth.signal(cfg, synth.PROFILE_MUSIC, seed, frames)
    return synth.encode_packet(cfg, [synth.default_elem(**kw) for _ in range(ne)], pcm)


def extreme_packet(synth, cfg):
    """One escaped packet whose samples are the depth's extremes in the PCM domain (a 20-bit sample comes out left-aligned in
    its three bytes), every channel starting at another one."""
    ex = np.array([-(1 << 19), (1 << 19) - 1, -1, 0, 1], np.int64) if cfg.bit_depth == 20 else wr.extremes(cfg.bit_depth)
    fl, ch = cfg.frame_length, cfg.num_channels
    pcm = np.stack([np.resize(np.roll(ex, c), fl) for c in range(ch)], axis=1).astype(np.int32)
    return synth.encode_packet(cfg, [synth.default_elem(force_escape=1) for _ in range(synth.num_elements(ch))], pcm)


def packet_list(synth, helpers, cfg, n, seed, damaged=0):
    """A synth batch with the extremes packet, short packets at the start, in the middle and at the end, and `damaged`
    mutated packets (helpers.mutate_packets: data errors the decoder reports as status) mixed in."""
    fl = cfg.frame_length
    b = synth.gen_batch(cfg, n, base_seed=seed, threads=8)
    rng = np.random.default_rng(seed)
    packets = [b.packet(i) for i in range(b.n)] + helpers.mutate_packets(b, rng, damaged)
    rng.shuffle(packets)
    packets.insert(len(packets) // 3, extreme_packet(synth, cfg))
    if fl > 1:
        for at, k, esc in ((0, 1, True), (len(packets) // 2, fl // 2 + 1, False), (len(packets) // 2, 3, True),
                           (len(packets), fl - 1, False), (len(packets), max(fl - 3, 1), True)):
            if 1 <= k < fl:
                packets.insert(at, short_packet(synth, cfg, k, seed + k, esc or fl < 16))
    return packets


class Batch:
    """Packets on the device and the oracle's decode of them."""

    def __init__(self, torch, oracle, helpers, cfg, packets):
        self.cfg, self.n = cfg, len(packets)
        blob, offs, sizes = helpers.pack_packets(packets)
        self.ref = oracle.decode_batch(cfg, blob, offs, sizes, threads=8)
        dev = torch.device("cuda:0")
        self.d_blob = torch.from_numpy(blob).to(dev)
        self.d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
        self.d_sz = torch.from_numpy(sizes.astype(np.int32)).to(dev)


def file_packets(oracle, synth, cfg, n, seed, last=None):
    """n full packets and a short last one, as an encoder writes a file (synth's batches have short packets of their own
    here and there: those are left out)."""
    b = synth.gen_batch(cfg, n + 8, base_seed=seed, threads=8)
    frames = oracle.decode_batch(cfg, b.blob, b.offsets, b.sizes, threads=8, want_output=False)[1]
    packets = [b.packet(i) for i in range(b.n) if frames[i] == cfg.frame_length][:n]
    assert len(packets) == n
    return packets + [short_packet(synth, cfg, last or cfg.frame_length // 3 + 1, seed, escape=False)]
