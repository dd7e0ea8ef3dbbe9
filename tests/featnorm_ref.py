"""TEST HELPER: the feature normalisation pass (csrc/alac_featnorm.h) restated in numpy float32, the shared cases of its CPU and
GPU tests, the buffers they run over, and the float64 bounds of its sums.

reference() follows the header's order: each chunk of tile_frames frames a loop over the frames (vectorised over the bins) from
+0.0, the chunks' sums added in chunk order from +0.0, one float32 division by the count, the deviations' squares summed the same
way, 1 / sqrt in float32. numpy's float32 +, -, *, / and sqrt are correctly rounded, as g++'s are, so the host build must give
these bits."""
import ctypes
import math
import os

import numpy as np

from tests import host_build

ROOT = host_build.ROOT
STATS = {"none": 0, "mean": 1, "mean_var": 2, "max": 3}
F32 = np.float32
U = 2.0 ** -24  # the unit roundoff of float32


def tile_frames_of(bins):
    """alacfn::tile_frames_of"""
    tf = 64
    while tf > 1 and bins * (tf | 1) + 256 > 12800:
        tf //= 2
    return tf


def clamp_lengths(lengths, rows, frames):
    if lengths is None:
        return [frames] * rows
    return [min(max(int(n), 0), frames) for n in lengths]


def chunk_sum(v, tf):
    """v [n, bins] float32 -> the header's sum over the frames"""
    total = np.zeros(v.shape[1], F32)
    for c in range(0, v.shape[0], tf):
        acc = np.zeros(v.shape[1], F32)
        for f in range(c, min(c + tf, v.shape[0])):
            acc = acc + v[f]
        total = total + acc
    return total


def largest(v):
    """The largest value that is no NaN, +0.0 above -0.0; -inf where there is none"""
    k = v.reshape(-1).view(np.int32).copy()
    k = k[~np.isnan(v.reshape(-1))]
    if not k.size:
        return F32(-np.inf)
    k = k ^ ((k >> 31) & 0x7fffffff)
    m = np.array([k.max()], np.int32)
    return (m ^ ((m >> 31) & 0x7fffffff)).view(F32)[0]


def reference(x, lengths, stat, shift=None, scale=None, var_floor=1e-20, range_=0.0, pad=0.0, tf=None):
    """x [rows, frames, bins] float32 -> (y of the same shape, stats [rows, 2, bins])"""
    rows, frames, bins = x.shape
    tf = tf or tile_frames_of(bins)
    y = np.full(x.shape, F32(pad), F32)
    stats = np.zeros((rows, 2, bins), F32)
    with np.errstate(all="ignore"):
        for r, n in enumerate(clamp_lengths(lengths, rows, frames)):
            if n == 0:
                continue
            v = x[r, :n]
            if stat in ("mean", "mean_var"):
                m = chunk_sum(v, tf) / F32(n)
                s = v - m
                stats[r, 0], stats[r, 1] = m, F32(1.0)
                if stat == "mean_var":
                    var = chunk_sum(s * s, tf) / F32(n)
                    var = np.where(var < F32(var_floor), F32(var_floor), var)
                    rstd = F32(1.0) / np.sqrt(var)
                    s = s * rstd
                    stats[r, 1] = rstd
            elif stat == "max":
                M = largest(v)
                c = M - F32(range_)
                s = np.where(v < c, c, v)
                stats[r, 0, 0] = M
            else:
                s = v
            if shift is not None:
                s = s - np.asarray(shift, F32)
            if scale is not None:
                s = s * np.asarray(scale, F32)
            y[r, :n] = s
    return y, stats


# ---- the float64 bounds --------------------------------------------------------------------------------------------------
REF64 = 2.0 ** -53  # per operation of the float64 reference itself: its n + 2 (mean) or n + 4 (variance) roundings are added


def gamma(k):
    return k * U / (1.0 - k * U)


def mean_bound(v, tf):
    """|m_b - m64_b| <= gamma(tf + K) * sum|x| / n for the valid frames v [n, bins]: a chunk's chain is at most tf - 1 additions, the
    chunks' K more, the division one more rounding: every term passes through at most tf + K roundings"""
    n = v.shape[0]
    K = math.ceil(n / tf)
    return (gamma(tf + K) + REF64 * (n + 2)) * np.abs(v.astype(np.float64)).sum(axis=0) / n


def var_bound(v, m32, tf):
    """|v_b - v64_b| for v64 the float64 variance about the float64 mean, v_b the header's about its own float32 mean m32. With d =
    x - m32 (one rounding), q = d * d (one more) and the sum and division as in mean_bound, each term d64^2 passes through at
    most 2 + 1 + tf + K roundings of relative size u: gamma(tf + K + 3) * sum(d64^2) / n. Moving the centre from m64 to m32
    changes the exact sum of squares by n (m32 - m64)^2 exactly, so by at most mean_bound^2 per frame."""
    n = v.shape[0]
    K = math.ceil(n / tf)
    d = v.astype(np.float64) - m32.astype(np.float64)
    return (gamma(tf + K + 3) + REF64 * (n + 4)) * (d * d).sum(axis=0) / n + mean_bound(v, tf) ** 2


# ---- buffers -------------------------------------------------------------------------------------------------------------
def lay_out(x, layout, row_gap=0, inner_gap=0, lead=0, fill=np.nan):
    """The logical x [rows, frames, bins] placed in a flat float32 buffer of `fill`: layout "frames" [rows][frames][bins] with
    inner_gap elements between frames, "bins" [rows][bins][frames] with inner_gap between bins; row_gap elements between rows,
    `lead` in front, 8 behind -> (buffer, the writable strided view [rows, frames, bins] into it, (row, frame, bin) strides in
    elements)"""
    rows, frames, bins = x.shape
    if layout == "frames":
        fs, bs = bins + inner_gap, 1
        extent = (frames - 1) * fs + bins
    else:
        fs, bs = 1, frames + inner_gap
        extent = (bins - 1) * bs + frames
    rs = extent + row_gap
    buf = np.full(lead + rows * rs + 8, fill, F32)
    view = np.lib.stride_tricks.as_strided(buf[lead:], x.shape, (4 * rs, 4 * fs, 4 * bs))
    view[...] = x
    return buf, view, (rs, fs, bs)


def outside(buf, view_of):
    """The elements of buf that the view does not cover (view_of(buffer) -> the strided view)"""
    mask = np.ones(buf.shape, bool)
    view_of(mask)[...] = False
    return buf[mask]


def view_like(buf, lead, shape, strides):
    return np.lib.stride_tricks.as_strided(buf[lead:], shape, tuple(buf.itemsize * s for s in strides))


# ---- the cases -----------------------------------------------------------------------------------------------------------
BINS = (1, 23, 80, 129)
# Above 192 bins the kernels run other code: 193 is the first count with tile_frames 32, 257 the first with two finishing blocks
# (the second holds one bin), 513 and 1025 are spectrograms of n_fft 1024 and 2048, 4096 is the limit (tile_frames 2, SpecAugment's
# tile_out 1)
WIDE_BINS = (193, 257, 513, 1025, 4096)


def frames_of(tf):
    return (1, tf - 1, tf, tf + 1, 2 * tf + 3)


def lengths_of(frames):
    """Six rows: nothing, one frame, a middle value, everything, and the two values that clamp"""
    return [0, 1, (frames + 1) // 2, frames, -5, frames + 7]


def features(rng, rows, frames, bins):
    """Log-mel-like values: a per-bin level in [-12, 2] plus noise"""
    level = rng.uniform(-12.0, 2.0, (1, 1, bins))
    return (level + rng.normal(0.0, 1.5, (rows, frames, bins))).astype(F32)


MODES = {
    "none": dict(stat="none"),
    "none_pad": dict(stat="none", pad=-3.5),
    "mean": dict(stat="mean"),
    "mean_var": dict(stat="mean_var"),
    "mean_var_floor": dict(stat="mean_var", var_floor=4.0),
    "max": dict(stat="max", range_=8.0),
    "affine": dict(stat="none", affine=True),
    "mean_affine": dict(stat="mean", affine=True, pad=-1.0),
    "whisper": dict(stat="max", range_=8.0, shift=-4.0, scale=0.25),
}


def mode_args(name, bins, rng=None):
    """-> the keyword arguments of reference() and host_run() for MODES[name] at `bins` bins"""
    m = dict(MODES[name])
    rng = rng or np.random.default_rng(bins)
    if m.pop("affine", False):
        m["shift"] = rng.uniform(-10.0, 2.0, bins).astype(F32)
        m["scale"] = rng.uniform(0.2, 3.0, bins).astype(F32)
    for k in ("shift", "scale"):
        if k in m and np.ndim(m[k]) == 0:
            m[k] = np.full(bins, m[k], F32)
    return m


# ---- the host build ------------------------------------------------------------------------------------------------------
def build_featnorm_sim():
    L = host_build.shared("featnorm_sim.cpp", "libfeatnorm_sim.so", host_build.SIM_FP)
    vp, u32, u64, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
    L.featnorm_sim_plan.argtypes = [u32, u32, f32, f32, vp]
    L.featnorm_sim_run.argtypes = [u32, u32, f32, f32, f32, vp, vp, vp, u64, u64, u64, u64, u64, vp, vp, u64, u64, u64, vp]
    return L


def build_featnorm_shim(pkg):
    """tests/host_sim/featnorm_shim.cpp over host/feature_norm.hpp, linked with the library"""
    L = host_build.shared("featnorm_shim.cpp", "libfeatnorm_shim.so", host_build.SHIM, host_build.library(pkg))
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    L.featnorm_shim_create.restype = ctypes.c_long
    L.featnorm_shim_create.argtypes = [vp, vp, u64, vp, u64]
    L.featnorm_shim_run.restype = ctypes.c_long
    L.featnorm_shim_run.argtypes = [vp, vp, vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]
    L.featnorm_shim_sizes.argtypes = [vp]
    L.featnorm_shim_last_error.restype = ctypes.c_char_p
    return L


def sim_plan(L, bins, stat="mean", var_floor=1e-20, range_=0.0):
    info = np.zeros(2, np.uint32)
    rc = L.featnorm_sim_plan(bins, STATS[stat], var_floor, range_, info.ctypes.data)
    return rc, {"tile_frames": int(info[0]), "lds_bytes": int(info[1])}


def host_run(L, bins, in_ptr, in_strides, rows, frames, lengths, out_ptr, out_strides, stats=None, stat="mean", shift=None,
             scale=None, var_floor=1e-20, range_=0.0, pad=0.0):
    """featnorm_sim_run over raw pointers -> its return code"""
    ln = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
    sh = None if shift is None else np.ascontiguousarray(shift, F32)
    sc = None if scale is None else np.ascontiguousarray(scale, F32)
    return L.featnorm_sim_run(bins, STATS[stat], var_floor, range_, pad, None if sh is None else sh.ctypes.data,
                              None if sc is None else sc.ctypes.data, in_ptr, *in_strides, rows, frames,
                              None if ln is None else ln.ctypes.data, out_ptr, *out_strides,
                              None if stats is None else stats.ctypes.data)


def host_values(L, x, lengths, layout="frames", **mode):
    """The host build over a dense copy of x in `layout` -> (y [rows, frames, bins], stats)"""
    rows, frames, bins = x.shape
    buf, view, st = lay_out(x, layout)
    obuf, oview, ost = lay_out(np.zeros_like(x), layout)
    stats = np.full((rows, 2, bins), 77.0, F32)
    rc = host_run(L, bins, view.ctypes.data, st, rows, frames, lengths, oview.ctypes.data, ost, stats, **mode)
    assert rc == 0, rc
    return oview.copy(), stats


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
