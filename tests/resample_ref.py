"""The resampler restated in numpy float64, independently of csrc/alac_resample.h, and the host build of
that header for the tests.

    g = gcd(orig, new); o = orig / g; n = new / g; base = min(o, n) * rolloff; width = ceil(W * o / base)
    t = clamp(((k - width) / o - i / n) * base, -W, W);  H[i][k] = 0 where |t| == W, else sinc(pi t) cos(pi t / 2W)^2 base / o
    out_frames(T) = ceil(new * T / orig);  y[j * n + i] = sum_k H[i][k] x[j * o + k - width], x zero outside [0, T)"""
import ctypes
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM_DIR = os.path.join(ROOT, "tests", "host_sim")

# every pair the plan must accept
PAIRS = [(44100, 16000), (16000, 44100), (44100, 48000), (48000, 44100), (48000, 16000), (8000, 48000), (96000, 44100),
         (192000, 8000), (44100, 22051), (3, 2), (2, 3), (7, 5)]


def geometry(orig, new, W=6, rolloff=0.99):
    """-> (o, n, base, width)"""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    return o, n, base, int(math.ceil(W * o / base))


def taps_at(orig, new, i, k, W=6, rolloff=0.99):
    """H[i][k] for integer arrays i, k that broadcast, float64."""
    o, n, base, width = geometry(orig, new, W, rolloff)
    i = np.asarray(i, np.int64)
    k = np.asarray(k, np.int64)
    t = ((k - width).astype(np.float64) / o - i.astype(np.float64) / n) * base
    t = np.clip(t, -float(W), float(W))
    v = np.sinc(t) * np.cos(np.pi * t / (2.0 * W)) ** 2 * base / o  # np.sinc(t) = sin(pi t) / (pi t), 1 at 0
    v = np.where(np.abs(t) == W, 0.0, v)
    return np.where((k >= 0) & (k < 2 * width + o), v, 0.0)


def table(orig, new, W=6, rolloff=0.99, phases=None):
    """The full H: [n][2 * width + o] float64 (phases: those rows only, where n rows would be too many)."""
    o, n, _, width = geometry(orig, new, W, rolloff)
    i = np.arange(n) if phases is None else np.asarray(phases)
    return taps_at(orig, new, i[:, None], np.arange(2 * width + o)[None, :], W, rolloff)


def out_frames(orig, new, T):
    return -((-new * T) // orig)


def _apply(x, o, n, width, h, first, frames):
    """y[r, j * n + i] = sum_q h[i][q] x[r, j * o + first[i] + q - width] in float64, for m < frames."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    R, T = x.shape
    taps = h.shape[1]
    J = -(-frames // n)
    pad_hi = max(0, (J - 1) * o + int(np.max(first)) + taps - width - T) + 1
    xp = np.concatenate([np.zeros((R, width)), x, np.zeros((R, pad_hi))], axis=1)
    y = np.zeros((R, J * n))
    q = np.arange(taps)
    for i in range(n):
        idx = np.arange(J)[:, None] * o + int(first[i]) + q[None, :]  # + width of the padding - width of the definition
        y[:, i::n] = np.einsum("rjq,q->rj", xp[:, idx], h[i])
    return y[:, :frames]


def resample64(x, orig, new, W=6, rolloff=0.99, h=None, first=None):
    """The definition in float64 over rows x [R, T] (or one row [T]) -> [R, out_frames]. h / first: a plan's own float32
    table and window starts in place of the full H."""
    o, n, _, width = geometry(orig, new, W, rolloff)
    x2 = np.atleast_2d(np.asarray(x, np.float64))
    if h is None:
        h, first = table(orig, new, W, rolloff), np.zeros(n, np.int64)
    y = _apply(x2, o, n, width, np.asarray(h, np.float64), first, out_frames(orig, new, x2.shape[1]))
    return y if np.ndim(x) > 1 else y[0]


def bound(h32, first, x, orig, new, W=6, rolloff=0.99):
    """Per output, taps * 2^-23 * sum |h| |x|: the bound taps * u / (1 - taps * u) of a dot product in float32, u = 2^-24,
    doubled; the fmaf chain has one rounding per term where that bound allows two."""
    o, n, _, width = geometry(orig, new, W, rolloff)
    x2 = np.atleast_2d(np.asarray(x, np.float64))
    h = np.abs(np.asarray(h32, np.float64))
    return h.shape[1] * 2.0 ** -23 * _apply(np.abs(x2), o, n, width, h, first, out_frames(orig, new, x2.shape[1]))


# ---- the host build ---------------------------------------------------------------------------------------------------
def build_resample_sim():
    so = os.path.join(SIM_DIR, "libresample_sim.so")
    csrc = os.path.join(ROOT, "saprobe-alac_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, "resample_sim.cpp"), os.path.join(csrc, "alac_resample.h"), os.path.join(csrc, "alac_waveform.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-fwrapv", "-fPIC", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-shared", "-o", so,
                               srcs[0]])
    L = ctypes.CDLL(so)
    vp, u32, u64, dbl = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
    L.resample_sim_plan.argtypes = [u32, u32, u32, dbl, vp, vp, u64, vp, u64]
    L.resample_sim_run.argtypes = [u32, u32, u32, dbl, vp, u64, u64, u64, vp, u64, ctypes.c_int]
    L.resample_sim_out_frames.restype, L.resample_sim_out_frames.argtypes = u64, [u32, u32, u64]
    L.resample_sim_stage_floats.restype = u32
    L.resample_sim_stage_need.restype, L.resample_sim_stage_need.argtypes = u64, [u32, u32, u32, dbl]
    return L


def sim_plan(S, orig, new, W=6, rolloff=0.99):
    """-> (info dict, h32 [n][taps], first [n]) of the host build's plan, or None where it has none."""
    info = np.zeros(5, np.uint32)
    if S.resample_sim_plan(orig, new, W, rolloff, info.ctypes.data, None, 0, None, 0) != 0:
        return None
    o, n, width, taps, tile_out = (int(v) for v in info)
    h = np.zeros((n, taps), np.float32)
    first = np.zeros(n, np.int32)
    assert S.resample_sim_plan(orig, new, W, rolloff, info.ctypes.data, h.ctypes.data, h.size, first.ctypes.data, first.size) == 0
    return dict(o=o, n=n, width=width, taps=taps, tile_out=tile_out), h, first


# ---- the sweep's inputs and buffers, shared by the CPU and the GPU suite ---------------------------------------------
SENTINEL = 0xC3C3A5A5  # as a float about -391.3: nothing a filter of gain 1 makes of inputs in [-1, 1]


def signal(rng, rows, T):
    """[rows, T] float32: int16 and int24 values scaled by 2^-15 / 2^-23 in turn, the last row full-scale alternating +-1."""
    x = np.zeros((rows, T), np.float32)
    for r in range(rows):
        if r % 2 == 0:
            x[r] = rng.integers(-32768, 32768, T).astype(np.float32) * np.float32(2.0 ** -15)
        else:
            x[r] = rng.integers(-(1 << 23), 1 << 23, T).astype(np.float32) * np.float32(2.0 ** -23)
    x[rows - 1] = np.where(np.arange(T) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return x


def boundary_frames(info, orig, new):
    """Input lengths around the plan: 1, 2, width - 1, width, the two whose output lands one short of and one past a tile
    boundary, and about 3 000."""
    tile = info["tile_out"]
    short = max(t for t in range(1, 4 * tile * orig // new + 8) if out_frames(orig, new, t) <= tile - 1)
    past = min(t for t in range(1, 4 * tile * orig // new + 8) if out_frames(orig, new, t) >= tile + 1)
    return sorted({1, 2, max(info["width"] - 1, 1), info["width"], short, past, 3001})


def layout(rows, T, frames, in_off, out_off):
    """Odd row strides and guard elements: -> (in_stride, in_lead, in_elems, out_stride, out_lead, out_elems); the tensors
    start in_lead / out_lead elements into 16-byte-aligned buffers, that is in_off / out_off elements behind a boundary."""
    in_stride = T + 1 + T % 2
    out_stride = frames + 1 + frames % 2
    in_lead, out_lead = 4 + in_off, 8 + out_off
    return in_stride, in_lead, in_lead + (rows - 1) * in_stride + T, out_stride, out_lead, out_lead + rows * out_stride + 8


def expected_image(y32, elems, out_lead, out_stride):
    """The whole output buffer as uint32: the rows' columns [0, frames) at their places, the sentinel everywhere else."""
    want = np.full(elems, SENTINEL, np.uint32)
    for r in range(y32.shape[0]):
        want[out_lead + r * out_stride: out_lead + r * out_stride + y32.shape[1]] = y32[r].view(np.uint32)
    return want
