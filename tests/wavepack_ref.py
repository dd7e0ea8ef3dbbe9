"""TEST HELPER for the pack pass (alacgpu_pcm_from_waveform_device): the numpy restatement every comparison uses, the host
build of csrc/alac_wavepack.h (tests/host_sim/pack_sim.cpp), and the expected image of a whole PCM buffer, sentinel included.

The restatement imports nothing of the code under test. With q = the depth:
    FLOAT  np.rint(x.astype(float32) * float32(2 ** (q - 1))) — numpy multiplies in float32 and rounds to nearest even —
           NaN -> 0, then clipped in int64 to [-2^(q - 1), 2^(q - 1) - 1]; depth 20: << 4
    INT    the int32 clipped in int64 to the container's width 16 / 24 / 24 / 32; depth 20: & ~15
    clipped = the NaNs plus the samples the clip changed
    bytes   wave_ref.pack_samples of the [frames, channels] integers
All comparisons are on bytes."""
import ctypes

import numpy as np

from tests import host_build
from tests import wave_ref as wr

STREAM, PACKETS, FLOAT, INT = wr.STREAM, wr.PACKETS, wr.FLOAT, wr.INT
PCM_SENTINEL = 0x5A
WAVE_SENTINEL = 0x7FC00BAD  # a NaN as float32, beyond every container but the 32-bit one as int32: read by mistake, it counts


def quantize(x, depth, wtype):
    """elements (float32 or int32 array, any shape) -> (int64 values as the sample's bytes hold them, clipped count)"""
    if wtype == FLOAT:
        with np.errstate(over="ignore", invalid="ignore"):
            r = np.rint(np.asarray(x, np.float32) * np.float32(2.0 ** (depth - 1)))
        nan = np.isnan(r)
        r = np.where(nan, np.float32(0), r)
        v = np.clip(r.astype(np.float64), -2.0 ** 40, 2.0 ** 40).astype(np.int64)  # +-inf made finite, still far outside
        top = 1 << (depth - 1)
        c = np.clip(v, -top, top - 1)
        clipped = int(nan.sum()) + int((c != v).sum())
        if depth == 20:
            c = c << 4
        return c, clipped
    v = np.asarray(x, np.int32).astype(np.int64)
    top = 1 << (wr.WIDTH[depth] - 1)
    c = np.clip(v, -top, top - 1)
    clipped = int((c != v).sum())
    if depth == 20:
        c = c & ~15
    return c, clipped


def pack_ref(x, depth, wtype):
    """x [channels, frames] -> (interleaved PCM bytes uint8, clipped)"""
    c, clipped = quantize(x, depth, wtype)
    return wr.pack_samples(c.T, depth), clipped


def expected_image(pcm, nbytes, base):
    """The whole PCM buffer of nbytes as the pass must leave it when it was filled with PCM_SENTINEL before."""
    img = np.full(nbytes, PCM_SENTINEL, np.uint8)
    img[base:base + pcm.size] = pcm
    return img


def lay_out(x, layout, fl, lead, cs, ps, elems):
    """x [channels, frames] (float32 or int32) placed in a WAVE_SENTINEL-filled buffer of `elems` uint32 elements, the tensor
    starting at element `lead`: STREAM rows of stride cs, PACKETS clips of stride ps with rows of stride cs. -> uint32 array"""
    buf = np.full(elems, WAVE_SENTINEL, np.uint32)
    u = np.ascontiguousarray(x).view(np.uint32)
    ch, total = u.shape
    if layout == STREAM:
        for c in range(ch):
            buf[lead + c * cs:lead + c * cs + total] = u[c]
    else:
        for i in range((total + fl - 1) // fl):
            k = min(fl, total - i * fl)
            for c in range(ch):
                o = lead + i * ps + c * cs
                buf[o:o + k] = u[c, i * fl:i * fl + k]
    return buf


def geometry(layout, fl, ch, total, slack, lead=8):
    """-> (cs, ps, elems) of a buffer with `slack` spare elements in both strides and 8 behind the tensor"""
    n = (total + fl - 1) // fl
    if layout == STREAM:
        cs, ps = total + slack, 0
        return cs, ps, lead + ch * cs + 8
    cs = fl + slack
    ps = ch * cs + (slack and slack + 1)
    return cs, ps, lead + max(n, 1) * ps + 8


def random_wave(rng, ch, total, depth, wtype, loud=0.02):
    """A waveform mostly inside the range, a fraction `loud` of it beyond; FLOAT also gets NaNs, infinities and denormals."""
    if wtype == FLOAT:
        x = rng.uniform(-1.0, 1.0, (ch, total)).astype(np.float32)
        k = rng.random((ch, total))
        x = np.where(k < loud, x * np.float32(3), x)
        x = np.where(k > 1 - loud / 4, np.float32(np.nan), x)
        x = np.where((k > 0.5) & (k < 0.5 + loud / 4), np.float32(np.inf) * np.sign(x), x).astype(np.float32)
        x = np.where((k > 0.6) & (k < 0.6 + loud / 4), x * np.float32(1e-40), x).astype(np.float32)
        return x
    top = 1 << (wr.WIDTH[depth] - 1)
    x = rng.integers(-top, top, (ch, total), dtype=np.int64)
    k = rng.random((ch, total))
    x = np.where(k < loud, x * 3, x)
    return np.clip(x, -(1 << 31), (1 << 31) - 1).astype(np.int32)


# ---- the host build --------------------------------------------------------------------------------------------------
def build_pack_sim():
    L = host_build.shared("pack_sim.cpp", "libpack_sim.so", host_build.SIM)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.pack_sim_run.argtypes = [u32, u32, u32, vp, ctypes.c_int, ctypes.c_int, u64, u64, u64, vp, vp, u64, vp]
    L.pack_sim_tile_frames.restype = u32
    L.pack_sim_tile_frames.argtypes = [u32, u32]
    return L
