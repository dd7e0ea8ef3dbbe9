"""TEST HELPER for the waveform pass (alacgpu_waveform_device): the numpy restatement every comparison uses, the host build
of csrc/alac_waveform.h (tests/host_sim/wave_sim.cpp), and the expected image of a whole wave buffer, sentinel included.

The restatement imports nothing of the code under test. It starts from decoded slots (out[n, stride] uint8, frames, status
— the oracle's triple, or slots a test wrote by hand):
    unpack the bytes to int64 per depth; FLOAT = np.float32(int32) * np.float32(2 ** -(w - 1)), numpy's int32 -> float32
    cast rounding to nearest even; INT = the int32; STREAM placed by np.cumsum, PACKETS zero-padded.
All comparisons are bit-exact: floats are compared as their uint32 views."""
import ctypes

import numpy as np

from tests import host_build

BPS = {16: 2, 20: 3, 24: 3, 32: 4}
WIDTH = {16: 16, 20: 24, 24: 24, 32: 32}
STREAM, PACKETS = 0, 1
FLOAT, INT = 0, 1
SENTINEL = 0xC3C3A5A5  # a float nobody decodes to, an int outside every depth but 32 (and improbable there)


# ---- the numpy restatement -------------------------------------------------------------------------------------------
def unpack(slot, f, depth, ch):
    """The first f frames of a slot -> int64 [f, ch]: little-endian, sign-extended from the bytes' width."""
    bps = BPS[depth]
    b = np.asarray(slot[:f * ch * bps], dtype=np.uint8).reshape(f, ch, bps).astype(np.int64)
    v = np.zeros((f, ch), np.int64)
    for k in range(bps):
        v |= b[:, :, k] << (8 * k)
    top = 1 << (8 * bps - 1)
    return (v ^ top) - top


def elements(v, depth, wtype):
    """int64 samples -> the output elements as uint32 bit patterns."""
    i32 = v.astype(np.int32)
    if wtype == INT:
        return i32.view(np.uint32)
    return (i32.astype(np.float32) * np.float32(2.0 ** -(WIDTH[depth] - 1))).view(np.uint32)


def frames_used(frames, status, fl, use_status=True):
    f = np.minimum(np.asarray(frames, np.int64), fl)
    if use_status and status is not None:
        f = np.where(np.asarray(status) != 0, 0, f)
    return f


def ref_stream(out, frames, status, fl, depth, ch, wtype, use_status=True):
    """-> (wave uint32 [ch, total], starts uint64 [n + 1])"""
    f = frames_used(frames, status, fl, use_status)
    starts = np.zeros(len(f) + 1, np.uint64)
    starts[1:] = np.cumsum(f)
    wave = np.zeros((ch, int(starts[-1])), np.uint32)
    for i in range(len(f)):
        if f[i]:
            wave[:, int(starts[i]):int(starts[i + 1])] = elements(unpack(out[i], int(f[i]), depth, ch), depth, wtype).T
    return wave, starts


def ref_packets(out, frames, status, fl, depth, ch, wtype, use_status=True):
    """-> wave uint32 [n, ch, fl], zero behind a packet's frames"""
    f = frames_used(frames, status, fl, use_status)
    wave = np.zeros((len(f), ch, fl), np.uint32)
    for i in range(len(f)):
        if f[i]:
            wave[i, :, :int(f[i])] = elements(unpack(out[i], int(f[i]), depth, ch), depth, wtype).T
    return wave


def expected_image(ref, layout, elems, base, cs, ps):
    """The whole wave buffer (`elems` uint32 elements, the tensor starting at element `base`) as the pass must leave it
    when it was filled with SENTINEL before: the reference at its place, the sentinel everywhere else."""
    img = np.full(elems, SENTINEL, np.uint32)
    if layout == STREAM:
        ch, total = ref.shape
        for c in range(ch):
            img[base + c * cs:base + c * cs + total] = ref[c]
    else:
        n, ch, fl = ref.shape
        for i in range(n):
            for c in range(ch):
                o = base + i * ps + c * cs
                img[o:o + fl] = ref[i, c]
    return img


def extremes(depth):
    """Every representable extreme of a depth's sample integer (w bits), and for 32 bits the values around 2^24 and
    below 2^31 where the float conversion rounds (ties to even in both directions, and up to 2^31)."""
    w = WIDTH[depth]
    top = 1 << (w - 1)
    v = [-top, top - 1, -1, 0, 1, -top + 1, top - 2]
    if depth == 20:
        v = [x & ~15 for x in v] + v  # left-aligned 20-bit values, and what the bytes could hold anyway
    if depth == 32:
        for k in (24, 25, 30):
            b = 1 << k
            v += [b - 1, b, b + 1, b + 2, b + 3, b + 5, b + 6, b + 7, -b - 1, -b - 3, -b + 1]
        v += [top - 63, top - 64, top - 65, top - 128, top - 129, top - 191, top - 192, top - 193, -top + 63, -top + 64, -top + 65]
    return np.array(v, np.int64)


def pack_samples(v, depth):
    """int64 [..., ch] -> little-endian bytes of the depth's width, flattened"""
    bps = BPS[depth]
    u = np.asarray(v, np.int64) & ((1 << (8 * bps)) - 1)
    b = np.stack([(u >> (8 * k)) & 0xff for k in range(bps)], axis=-1).astype(np.uint8)
    return b.reshape(-1)


def hand_slots(rng, n, fl, depth, ch, stride, frames):
    """Slots written by hand: random bytes everywhere (so the bytes behind a packet's frames and in failed slots are
    garbage that must not show), the depth's extremes sprinkled over every packet's frames."""
    out = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    ex = extremes(depth)
    bps = BPS[depth]
    for i in range(n):
        f = int(min(frames[i], fl))
        if not f:
            continue
        k = min(len(ex) * 2, f * ch)
        where = rng.choice(f * ch, size=k, replace=False)
        vals = ex[rng.integers(0, len(ex), k)]
        vals[:min(k, len(ex))] = ex[:min(k, len(ex))]
        for pos, v in zip(where, vals):
            out[i, pos * bps:(pos + 1) * bps] = pack_samples(np.array([v]), depth)
    return out


def frame_counts(rng, n, fl, pattern):
    """Frame counts for a batch: short packets at the start, in the middle and at the end; values above frame_length
    (a hostile d_frames) in the 'hostile' pattern."""
    f = np.full(n, fl, np.uint32)
    short = sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n)))
    for j, i in enumerate(short):
        f[i] = (1, fl - 1, max(fl // 2 - 1, 0), 0, max(fl - 3, 0))[j % 5] if fl > 1 else j % 2
    if pattern == "odd":
        f[rng.integers(0, n, max(1, n // 3))] = rng.integers(0, fl + 1, max(1, n // 3))
    if pattern == "hostile":
        f[n // 3] = fl + 5
        f[(2 * n) // 3] = 0xFFFFFFFF
    return f


# ---- the host build --------------------------------------------------------------------------------------------------
def build_wave_sim():
    L = host_build.shared("wave_sim.cpp", "libwave_sim.so", host_build.SIM)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.wave_sim_run.argtypes = [u32, u32, u32, vp, u64, vp, vp, u64, ctypes.c_int, ctypes.c_int, vp, u64, u64, vp]
    L.wave_sim_tile_frames.restype = u32
    L.wave_sim_tile_frames.argtypes = [u32, u32]
    return L


def at_alignment(nbytes, misalign, fill=None):
    """A uint8 array of nbytes whose address is `misalign` modulo 16 (and the array that owns the memory)."""
    own = np.zeros(nbytes + 32, np.uint8)
    off = (misalign - own.ctypes.data) % 16
    a = own[off:off + nbytes]
    assert a.ctypes.data % 16 == misalign % 16
    if fill is not None:
        a.view(np.uint32)[:] = fill
    return a
