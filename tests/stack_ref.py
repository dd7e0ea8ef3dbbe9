"""TEST HELPER: the frame stacking pass (csrc/alac_stack.h) restated in numpy float32, the shared cases of its CPU and GPU tests,
the host build, and the float64 bound of its delta chains.

reference() follows the header: the weight tables as exact integer numerators over (sum j^2)^k rounded to float32 once, each d_k
the chain acc = fma(w_i, x[clamp(t + i)], acc) over i = -M_k .. M_k from +0.0 with the taps of weight zero skipped, then the
gather y[g][(c, k, b)] = d_k[clamp(g * stride + c - left)][b]. fma32 is a correctly rounded float32 fused multiply-add out of
float64 arithmetic (the product of two float32 is exact in float64; the sum is rounded to odd before it is rounded to float32),
so the host build, whose fmaf is the C library's, must give these bits."""
import ctypes

import numpy as np

from tests import featnorm_ref as fr
from tests import host_build

ROOT = host_build.ROOT
F32 = np.float32
U = 2.0 ** -24
LDS_FLOATS = 6400  # alacst::kLdsFloats

# (order, window, left, right, stride); window is read with order > 0 only
PARAMS = ((0, 2, 0, 0, 1), (1, 1, 0, 0, 1), (1, 2, 0, 0, 1), (2, 2, 0, 0, 1), (2, 3, 1, 1, 1), (0, 2, 3, 3, 6), (0, 2, 0, 4, 3),
          (0, 2, 5, 0, 2), (2, 2, 3, 3, 6), (1, 8, 16, 16, 64))
BINS = fr.BINS
WIDE_BINS = fr.WIDE_BINS
clamp_lengths, lengths_of, same_bits, lay_out, outside, view_like, features = (
    fr.clamp_lengths, fr.lengths_of, fr.same_bits, fr.lay_out, fr.outside, fr.view_like, fr.features)


def param_id(ps):
    return "o%dw%dl%dr%ds%d" % ps


def columns_of(ps, bins):
    order, _, left, right, _ = ps
    return (left + right + 1) * (order + 1) * bins


def accepted(ps, bins):
    """what alacgpu_stack_create takes: the ranges, and at most 4096 output columns"""
    order, window, left, right, stride = ps
    return (1 <= bins <= 4096 and 0 <= order <= 2 and (order == 0 or 1 <= window <= 8) and 0 <= left <= 16 and 0 <= right <= 16
            and 1 <= stride <= 64 and columns_of(ps, bins) <= 4096)


def plan_of(ps, bins):
    """alacst::plan_of"""
    order, window, left, right, stride = ps
    K, C, M = order + 1, left + right + 1, order * window
    tb = bins
    while K * tb * ((C + 2 * M) | 1) > LDS_FLOATS:
        tb = (tb + 1) // 2
    T = 1
    while T < 64 and K * tb * ((T * stride + C + 2 * M) | 1) <= LDS_FLOATS:
        T += 1
    tile_in = (T - 1) * stride + C + 2 * M
    return dict(columns=C * K * bins, tile_out=T, tile_in=tile_in, tile_bins=tb, lds_bytes=4 * ((K * tb * (tile_in | 1) + 3) & ~3),
                w1_entries=2 * window + 1 if order >= 1 else 0, w2_entries=4 * window + 1 if order >= 2 else 0)


def frames_of(ps, bins):
    t = plan_of(ps, bins)["tile_in"]
    return tuple(f for f in (1, t - 1, t, t + 1, 2 * t + 3) if f >= 1)


def numerators(order, window):
    """-> ([the integer numerators of w_1, .. w_order], sum j^2): w_k = numerators / (sum j^2)^k"""
    norm = 2 * sum(j * j for j in range(1, window + 1))
    tabs, prev = [], [1]
    for k in range(1, order + 1):
        Mp, M = (k - 1) * window, k * window
        cur = [0] * (2 * M + 1)
        for i in range(-Mp, Mp + 1):
            for j in range(-window, window + 1):
                cur[i + j + M] += j * prev[i + Mp]
        tabs.append(cur)
        prev = cur
    return tabs, norm


def weights(order, window, dtype=F32):
    tabs, norm = numerators(order, window)
    return [(np.array(t, np.float64) / float(norm ** (k + 1))).astype(dtype) for k, t in enumerate(tabs)]


def fma32(a, b, c):
    """float32 a * b + c rounded once, elementwise"""
    p = a.astype(np.float64) * b.astype(np.float64)  # exact
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)  # TwoSum: s + err is the exact sum
    inexact = err != 0
    t = np.where(inexact & ((err > 0) != (s > 0)), np.nextafter(s, 0.0), s)  # truncated towards zero
    bits = t.view(np.int64).copy()
    bits[inexact] |= 1  # rounded to odd at 53 bits: rounding that to 24 bits is rounding the exact sum
    return bits.view(np.float64).astype(F32)


def delta(v, k, window, w):
    """v [n, bins] float32 -> d_k of every frame"""
    n, M = v.shape[0], k * window
    idx = np.arange(n)
    acc = np.zeros(v.shape, F32)
    for i in range(-M, M + 1):
        if w[i + M] == 0:
            continue
        acc = fma32(np.full(v.shape, w[i + M], F32), v[np.clip(idx + i, 0, n - 1)], acc)
    return acc


def gather(d, n, ps, bins, y_row):
    """d = [d_0 .. d_order] of a row's n valid frames -> the row's first ceil(n / stride) output frames into y_row"""
    order, _, left, right, stride = ps
    K, C = order + 1, left + right + 1
    m = -(-n // stride)
    g = np.arange(m)
    for c in range(C):
        idx = np.clip(g * stride + c - left, 0, n - 1)
        for k in range(K):
            y_row[:m, (c * K + k) * bins:(c * K + k + 1) * bins] = d[k][idx]
    return m


def reference(x, lengths, ps, pad=0.0):
    """x [rows, frames, bins] float32 -> (y [rows, G, D] float32, out_lengths int32 [rows])"""
    order, window, left, right, stride = ps
    rows, frames, bins = x.shape
    G = -(-frames // stride)
    y = np.full((rows, G, columns_of(ps, bins)), F32(pad), F32)
    out_len = np.zeros(rows, np.int32)
    w = weights(order, window)
    for r, n in enumerate(clamp_lengths(lengths, rows, frames)):
        out_len[r] = -(-n // stride)
        if n:
            v = x[r, :n]
            gather([v] + [delta(v, k, window, w[k - 1]) for k in range(1, order + 1)], n, ps, bins, y[r])
    return y, out_len


def reference64(v, ps):
    """One row's valid frames v [n, bins] -> (y64 [m, D] in float64 with the exact weights, the bound's sum |w_i| |x_i| per element,
    the taps per element): order 0 columns have a sum of 0"""
    order, window, left, right, stride = ps
    n, bins = v.shape
    v64 = v.astype(np.float64)
    idx = np.arange(n)
    d, mag, taps = [v64], [np.zeros_like(v64)], [np.zeros_like(v64)]
    for k, w in enumerate(weights(order, window, np.float64), 1):
        M = k * window
        acc, a = np.zeros_like(v64), np.zeros_like(v64)
        for i in range(-M, M + 1):
            xi = v64[np.clip(idx + i, 0, n - 1)]
            acc += w[i + M] * xi
            a += abs(w[i + M]) * np.abs(xi)
        d.append(acc)
        mag.append(a)
        taps.append(np.full_like(v64, np.count_nonzero(w)))
    m = -(-n // stride)
    out = [np.zeros((m, columns_of(ps, bins))) for _ in range(3)]
    for o, src in zip(out, (d, mag, taps)):
        gather(src, n, ps, bins, o)
    return out


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the host build ------------------------------------------------------------------------------------------------------
def build_stack_sim():
    L = host_build.shared("stack_sim.cpp", "libstack_sim.so", host_build.SIM_FP)
    vp, u32, u64, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
    L.stack_sim_plan.argtypes = [u32] * 6 + [vp, vp]
    L.stack_sim_run.argtypes = [u32] * 6 + [f32, vp, u64, u64, u64, u64, u64, vp, vp, u64, u64, u64, vp]
    return L


def build_stack_shim(pkg):
    """tests/host_sim/stack_shim.cpp over host/frame_stack.hpp, linked with the library"""
    L = host_build.shared("stack_shim.cpp", "libstack_shim.so", host_build.SHIM, host_build.library(pkg))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.stack_shim_create.restype = ctypes.c_long
    L.stack_shim_create.argtypes = [vp]
    L.stack_shim_run.restype = ctypes.c_long
    L.stack_shim_run.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]
    L.stack_shim_sizes.argtypes = [vp]
    L.stack_shim_last_error.restype = ctypes.c_char_p
    return L


INFO = ("columns", "tile_out", "tile_in", "tile_bins", "lds_bytes", "w1_entries", "w2_entries")


def sim_plan(L, ps, bins):
    """-> (return code, the plan's numbers, [w_1, w_2])"""
    info, w = np.zeros(7, np.uint32), np.zeros(50, F32)
    rc = L.stack_sim_plan(bins, ps[0], ps[1], ps[2], ps[3], ps[4], info.ctypes.data, w.ctypes.data)
    pl = dict(zip(INFO, (int(v) for v in info)))
    return rc, pl, [w[:pl["w1_entries"]], w[pl["w1_entries"]:pl["w1_entries"] + pl["w2_entries"]]]


def host_run(L, ps, bins, in_ptr, in_strides, rows, frames, lengths, out_ptr, out_strides, out_lengths=None, pad=0.0):
    """stack_sim_run over raw pointers -> its return code"""
    ln = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
    return L.stack_sim_run(bins, ps[0], ps[1], ps[2], ps[3], ps[4], pad, in_ptr, *in_strides, rows, frames,
                           None if ln is None else ln.ctypes.data, out_ptr, *out_strides,
                           None if out_lengths is None else out_lengths.ctypes.data)


def host_values(L, x, lengths, ps, in_layout="frames", out_layout="frames", pad=0.0):
    """The host build over a dense copy of x in in_layout -> (y [rows, G, D], out_lengths)"""
    rows, frames, bins = x.shape
    G = -(-frames // ps[4])
    _, view, st = lay_out(x, in_layout)
    _, oview, ost = lay_out(np.zeros((rows, G, columns_of(ps, bins)), F32), out_layout)
    out_len = np.full(rows, -77, np.int32)
    rc = host_run(L, ps, bins, view.ctypes.data, st, rows, frames, lengths, oview.ctypes.data, ost, out_len, pad)
    assert rc == 0, rc
    return oview.copy(), out_len
