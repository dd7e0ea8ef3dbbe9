"""TEST HELPER: the SpecAugment pass (csrc/alac_specaug.h) restated in numpy, the shared cases of its CPU and GPU tests and the
host build.

The definition (include/alacgpu.h). Input float32 x[r][f][b] with n_r = clamp(lengths[r], 0, frames) valid frames
per row; the output has the same shape. Parameters: bins 1..4096, freq_masks (nf) 0..8, freq_width (Fw) 0..bins, time_masks (nt)
0..16, time_width (Tw) 0..65535, time_ratio_q16 (q) 0..65536, warp (W) 0..256, mask_value, pad_value. Per call: seed (uint64),
row_base (uint64), ids (int64 per row, optional); row r's identity is id = ids[r] as uint64, or row_base + r.

* Random words: Philox4x32-10 with Random123's constants (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9,
  0xBB67AE85), key (seed low, seed high); word j of a row is output word j % 4 of the block at counter (id low, id high, j // 4,
  0). A draw from [0, m) is (word * m) >> 32. A row consumes P = 2 + 2 nf + 2 nt words whatever n_r is.
* Words 0, 1: the warp, only where W > 0 and n_r > 2 W: c = W + draw(n_r - 2 W), w = c - W + 1 + draw(2 W); otherwise c = w = 0
  and the row is copied. Output frames [0, w) are the source frames [0, c) resampled linearly, output frames [w, n_r) the source
  frames [c, n_r), each segment on its own.
* Output frame t of a segment of a source frames and b output frames: num = (2 t + 1) a - b; num <= 0: i0 = 0, lq = 0; else i0 =
  num // (2 b), lq = ((num % (2 b)) << 23) // (2 b); i1 = min(i0 + 1, a - 1). Where lq == 0 or i1 == i0, y = x[i0] copied; else y =
  fma(lq * 2^-23, x[i1] - x[i0], x[i0]) in float32.
* Words 2 + 2 i, 3 + 2 i: frequency mask i, fw = draw(Fw + 1), f0 = draw(bins - fw + 1), bins [f0, f0 + fw). The 2 nt words behind
  them: time mask i, cap = min(Tw, (n_r * q) >> 16), tw = draw(cap + 1), t0 = draw(n_r - tw + 1), frames [t0, t0 + tw). Masks are in
  output coordinates, behind the warp; an element under any mask is mask_value.
* Every frame f >= n_r is pad_value. The resolved draws of a row are P int32: c, w, then (start, width) per mask in word order.

fma32 is stack_ref's correctly rounded float32 fused multiply-add, so the host build, whose fmaf is the C library's, must give
these bits; the draws are integers."""
import ctypes

import numpy as np

from tests import featnorm_ref as fr
from tests import host_build
from tests.stack_ref import fma32

ROOT = host_build.ROOT
F32 = np.float32
U = 2.0 ** -24
IMAGE_FLOATS = 6016  # alacsa::kImageFloats
M64 = (1 << 64) - 1
BINS = fr.BINS
WIDE_BINS = fr.WIDE_BINS
clamp_lengths, same_bits, lay_out, outside, view_like, features = (fr.clamp_lengths, fr.same_bits, fr.lay_out, fr.outside, fr.view_like,
                                                                   fr.features)

# (freq_masks, freq_width, time_masks, time_width, time_ratio_q16, warp); freq_width is cut to the bins (for_bins)
PARAMS = {"noop": (0, 0, 0, 0, 65536, 0), "masks": (2, 10, 2, 20, 65536, 0), "warp": (0, 0, 0, 0, 65536, 5),
          "all": (2, 10, 2, 20, 13107, 5), "max": (8, 4096, 16, 65535, 65536, 256)}


def for_bins(ps, bins):
    return (ps[0], min(ps[1], bins), ps[2], ps[3], ps[4], ps[5])


def tile_out_of(bins):
    """alacsa::tile_out_of"""
    T = 64
    while T > 1 and bins * (T | 1) > IMAGE_FLOATS:
        T -= 1
    return T


def plan_of(ps, bins):
    T = tile_out_of(bins)
    image = (bins * (T | 1) + 3) & ~3
    return dict(draws=2 + 2 * ps[0] + 2 * ps[2], tile_out=T, lds_bytes=4 * ((image + 3 * T + 52 + (bins + 31) // 32 + 3) & ~3))


def frames_of(bins):
    T = tile_out_of(bins)
    return tuple(sorted({f for f in (1, 2, T - 1, T, T + 1, 3 * T + 5) if f >= 1}))


def lengths_of(frames, W):
    """Seven rows: a negative count, nothing, one frame, the longest row that is not warped, the shortest that is, everything, more"""
    return [-3, 0, 1, 2 * W, 2 * W + 1, frames, frames + 9]


def accepted(ps, bins):
    nf, Fw, nt, Tw, q, W = ps
    return 1 <= bins <= 4096 and 0 <= nf <= 8 and 0 <= Fw <= bins and 0 <= nt <= 16 and 0 <= Tw <= 65535 and 0 <= q <= 65536 and 0 <= W <= 256


# ---- the random words ----------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    c, (k0, k1) = list(counter), key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def words_of(seed, ident, count):
    out = []
    for blk in range((count + 3) // 4):
        out += philox4x32_10([ident & 0xFFFFFFFF, (ident >> 32) & 0xFFFFFFFF, blk, 0], (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return out[:count]


def draw(word, m):
    return (word * m) >> 32


def draws_of(ps, bins, n, seed, ident):
    """The resolved draws of a row of n valid frames -> P integers: c, w, then (start, width) per mask in word order"""
    nf, Fw, nt, Tw, q, W = ps
    wd = words_of(seed, ident, 2 + 2 * nf + 2 * nt)
    out = [0, 0]
    if W > 0 and n > 2 * W:
        c = W + draw(wd[0], n - 2 * W)
        out = [c, c - W + 1 + draw(wd[1], 2 * W)]
    for i in range(nf):
        fw = draw(wd[2 + 2 * i], Fw + 1)
        out += [draw(wd[3 + 2 * i], bins - fw + 1), fw]
    cap = min(Tw, (n * q) >> 16)
    for i in range(nt):
        tw = draw(wd[2 + 2 * nf + 2 * i], cap + 1)
        out += [draw(wd[3 + 2 * nf + 2 * i], n - tw + 1), tw]
    return out


# ---- the warp ------------------------------------------------------------------------------------------------------------
def segment_plan(a, b):
    """a source frames -> b output frames: (i0, i1, lq) per output frame, as Python integers"""
    plan = []
    for t in range(b):
        num = (2 * t + 1) * a - b
        i0, lq = (0, 0) if num <= 0 else (num // (2 * b), ((num % (2 * b)) << 23) // (2 * b))
        plan.append((i0, min(i0 + 1, a - 1), lq))
    return plan


def row_plan(n, c, w):
    """-> int64 arrays i0, i1, lq over the row's n output frames, the indices in the row's own frames"""
    if w == 0:
        plan = [(t, t, 0) for t in range(n)]
    else:
        plan = segment_plan(c, w) + [(c + i0, c + i1, lq) for i0, i1, lq in segment_plan(n - c, n - w)]
    a = np.array(plan, np.int64).reshape(n, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def warped(v, c, w):
    """v [n, bins] float32 -> the warped row, float32"""
    i0, i1, lq = row_plan(v.shape[0], c, w)
    x0, x1 = v[i0], v[i1]
    copy = ((lq == 0) | (i1 == i0))[:, None] & np.ones(v.shape, bool)
    with np.errstate(all="ignore"):
        lam = np.broadcast_to((lq.astype(F32) * F32(2.0 ** -23))[:, None], v.shape)
        safe0, safe1 = np.where(copy, F32(0), x0), np.where(copy, F32(0), x1)
        y = fma32(np.ascontiguousarray(lam), safe1 - safe0, safe0)
    return np.where(copy, x0, y)


def reference(x, lengths, ps, seed, row_base=0, ids=None, mask_value=0.0, pad_value=0.0):
    """x [rows, frames, bins] float32 -> (y of the same shape, draws int32 [rows, P])"""
    rows, frames, bins = x.shape
    nf = ps[0]
    y = np.full(x.shape, F32(pad_value), F32)
    P = 2 + 2 * ps[0] + 2 * ps[2]
    draws = np.zeros((rows, P), np.int32)
    for r, n in enumerate(clamp_lengths(lengths, rows, frames)):
        ident = (int(ids[r]) if ids is not None else row_base + r) & M64
        d = draws_of(ps, bins, n, seed, ident)
        draws[r] = d
        if n == 0:
            continue
        out = warped(x[r, :n], d[0], d[1])
        for i in range(nf):
            out[:, d[2 + 2 * i]:d[2 + 2 * i] + d[3 + 2 * i]] = F32(mask_value)
        for i in range(nf, nf + ps[2]):
            out[d[2 + 2 * i]:d[2 + 2 * i] + d[3 + 2 * i]] = F32(mask_value)
        y[r, :n] = out
    return y, draws


# ---- the host build ------------------------------------------------------------------------------------------------------
def build_specaug_sim():
    L = host_build.shared("specaug_sim.cpp", "libspecaug_sim.so", host_build.SIM_FP)
    vp, u64, f32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_float
    L.specaug_sim_philox.argtypes = [vp, vp, vp]
    L.specaug_sim_plan.argtypes = [vp, vp]
    L.specaug_sim_run.argtypes = [vp, f32, f32, vp, u64, u64, u64, u64, u64, vp, u64, u64, vp, vp, u64, u64, u64, vp]
    return L


def build_specaug_shim(pkg):
    """tests/host_sim/specaug_shim.cpp over host/spec_augment.hpp, linked with the library"""
    L = host_build.shared("specaug_shim.cpp", "libspecaug_shim.so", host_build.SHIM, host_build.library(pkg))
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    L.specaug_shim_create.restype = ctypes.c_long
    L.specaug_shim_create.argtypes = [vp]
    L.specaug_shim_run.restype = ctypes.c_long
    L.specaug_shim_run.argtypes = [vp, vp, vp, sz, sz, vp, u64, u64, vp, vp, vp, vp, vp]
    L.specaug_shim_sizes.argtypes = [vp]
    L.specaug_shim_last_error.restype = ctypes.c_char_p
    return L


def config_words(ps, bins):
    return np.array([bins, ps[0], ps[1], ps[2], ps[3], ps[4], ps[5]], np.int64).astype(np.uint32)


def sim_philox(L, counter, key):
    c, k, out = np.array(counter, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    L.specaug_sim_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return [int(v) for v in out]


def sim_plan(L, ps, bins):
    """-> (return code, the plan's numbers)"""
    info, cfg = np.zeros(3, np.uint32), config_words(ps, bins)
    rc = L.specaug_sim_plan(cfg.ctypes.data, info.ctypes.data)
    return rc, dict(zip(("draws", "tile_out", "lds_bytes"), (int(v) for v in info)))


def host_run(L, ps, bins, in_ptr, in_strides, rows, frames, lengths, seed, out_ptr, out_strides, draws=None, row_base=0, ids=None,
             mask_value=0.0, pad_value=0.0):
    """specaug_sim_run over raw pointers -> its return code"""
    ln = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
    idv = None if ids is None else np.ascontiguousarray(ids, np.int64)
    cfg = config_words(ps, bins)
    return L.specaug_sim_run(cfg.ctypes.data, mask_value, pad_value, in_ptr, *in_strides, rows, frames,
                             None if ln is None else ln.ctypes.data, seed, row_base, None if idv is None else idv.ctypes.data, out_ptr,
                             *out_strides, None if draws is None else draws.ctypes.data)


def host_values(L, x, lengths, ps, seed, in_layout="frames", out_layout="frames", **kw):
    """The host build over a dense copy of x in in_layout -> (y [rows, frames, bins], draws [rows, P])"""
    rows, frames, bins = x.shape
    _, view, st = lay_out(x, in_layout)
    _, oview, ost = lay_out(np.zeros_like(x), out_layout)
    draws = np.full((rows, 2 + 2 * ps[0] + 2 * ps[2]), -77, np.int32)
    rc = host_run(L, ps, bins, view.ctypes.data, st, rows, frames, lengths, seed, oview.ctypes.data, ost, draws, **kw)
    assert rc == 0, rc
    return oview.copy(), draws
