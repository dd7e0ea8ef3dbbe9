"""TEST HELPER: the waveform augmentation pass (csrc/alac_waveaug.h) restated in numpy, the shared cases of its CPU and GPU tests
and the host build.

The definition (include/alacgpu.h). Input float32 x[r][t], rows x T, n_r = clamp(lengths[r], 0, T) valid samples per
row; the output has the same shape. The bank z[k][u], N x Tn, m_k = clamp(noise_lengths[k], 0, Tn). A parameter set here is
cfg = (snr_lo_q8, snr_hi_q8, gain_lo_q8, gain_hi_q8, noise_prob_q16, clamp) with dither and pad_value beside it.

* Tables: snr_amp[i] = float32(10^(-(snr_lo_q8 + i) / 5120)), gain_amp[i] = float32(10^((gain_lo_q8 + i) / 5120)), in double.
* Random words: Philox4x32-10, key (seed low, seed high), id = ids[r] as uint64 or row_base + r. The row's word j is output word
  j % 4 of the block at (id low, id high, j // 4, 2); the dither of sample t is the block at (id low, id high, t, 3).
* Five words per row: applied = N > 0 and draw(w0, 65536) < noise_prob_q16; k = draw(w1, N); o = draw(w2, m_k), m_k == 0 clears
  applied, k and o; snr_i = draw(w3, snr_hi_q8 - snr_lo_q8 + 1); gain_i = draw(w4, gain_hi_q8 - gain_lo_q8 + 1); draw(w, m) =
  (w * m) >> 32. z_t = z[k][(o + t) % m_k].
* Energies over t < n_r in the fixed order: chunks of TILE samples; per chunk 256 lanes chain acc = fma(v, v, acc) over the
  samples of index = l mod 256 in increasing order from +0.0; acc[l] += acc[l + s] for s = 128 .. 1; chunks in order from +0.0.
* a = gain_amp[gain_i]; b = (sqrt(Ex / En) * snr_amp[snr_i]) * a in float32 where applied, Ex > 0, En > 0, both finite; else 0.
* t < n_r: v = a * x_t; b != 0: v = fma(b, z_t, v); dither != 0: v = fma(dither, g_t, v); clamp by comparisons. t >= n_r: pad_value.
* g_t: the block's halves h0 .. h7 (low half of word 0 first), s = (h0 + h1 + h2 + h3) - (h4 + h5 + h6 + h7), g = float32(s) * KSCALE.

fma32 is stack_ref's correctly rounded float32 fused multiply-add, so the host build, whose fmaf is the C library's, must give
these bits; fma here hands it the finite operands and rounds the double a b + c where one is infinite or NaN.

The shared cases of the second look (tests/test_waveaug_paths_host.py holds the host build to reference() over them,
tests/test_gpu_waveaug_paths.py the kernels to the host build): long_rows_case, clip_case, edge_cases."""
import ctypes
import functools
import math

import numpy as np

from tests import host_build
from tests.featnorm_ref import clamp_lengths, same_bits
from tests.stack_ref import fma32

ROOT = host_build.ROOT
F32 = np.float32
U = 2.0 ** -24
TILE = 4096
LANES = 256
M64 = (1 << 64) - 1
KSCALE = F32(1.0 / math.sqrt((2 ** 32 - 1) * 2.0 / 3.0))  # 0x1.3988e2p-16
ROW_STREAM, DITHER_STREAM = 2, 3
SEED = 0x1234_5678_9ABC_DEF1  # of the shared cases; the two test files use the same
u64 = np.uint64
MASK = u64(0xFFFFFFFF)

# (snr_lo_q8, snr_hi_q8, gain_lo_q8, gain_hi_q8, noise_prob_q16, clamp), dither
PARAMS = {"noop": ((0, 0, 0, 0, 0, 0), 0.0), "gain": ((0, 0, -6 * 256, 3 * 256, 0, 0), 0.0),
          "noise": ((5 * 256, 20 * 256, 0, 0, 65536, 0), 0.0), "dither": ((0, 0, 0, 0, 0, 0), 0.1),
          "all": ((-3 * 256, 15 * 256 + 7, -6 * 256 - 1, 3 * 256, 52429, 1), 0.01)}
SAMPLES = (1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)


def lengths_of(T):
    return [-2, 0, 1, T - 1, T, T + 9]


def accepted(cfg, dither=0.0):
    ok = all(-16384 <= lo <= hi <= 16384 and hi - lo <= 16384 for lo, hi in (cfg[0:2], cfg[2:4]))
    return ok and 0 <= cfg[4] <= 65536 and cfg[5] in (0, 1) and math.isfinite(dither) and dither >= 0


def tables(cfg):
    snr = np.array([math.pow(10.0, -(cfg[0] + i) / 5120.0) for i in range(cfg[1] - cfg[0] + 1)], np.float64).astype(F32)
    gain = np.array([math.pow(10.0, (cfg[2] + i) / 5120.0) for i in range(cfg[3] - cfg[2] + 1)], np.float64).astype(F32)
    return snr, gain


# ---- the random words ----------------------------------------------------------------------------------------------------
def philox_blocks(c0, c1, c2, c3, seed):
    """Philox4x32-10 over arrays of counters (broadcast against each other) -> uint64 array [..., 4] of the blocks' words"""
    c = [np.asarray(v, u64) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = u64(seed & 0xFFFFFFFF), u64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = u64(0xD2511F53) * c[0], u64(0xCD9E8D57) * c[2]
        c = [(p1 >> u64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> u64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + u64(0x9E3779B9)) & MASK, (k1 + u64(0xBB67AE85)) & MASK
    return np.stack(c, axis=-1)


def philox4x32_10(counter, key):
    return [int(v) for v in philox_blocks(*counter, key[0] | (key[1] << 32))]


def row_words(seed, idents):
    """idents (Python ints or an array, as uint64) -> uint64 [rows, 8]: the two blocks of stream 2"""
    idents = np.asarray([i & M64 for i in idents] if not isinstance(idents, np.ndarray) else idents, u64)
    lo, hi = idents & MASK, idents >> u64(32)
    return np.concatenate([philox_blocks(lo, hi, blk, ROW_STREAM, seed) for blk in (0, 1)], axis=-1)


def dither_variates(seed, ident, t):
    """g of the samples t (an integer array) of the row `ident`, float32"""
    ident &= M64
    w = philox_blocks(ident & 0xFFFFFFFF, ident >> 32, np.asarray(t, u64), DITHER_STREAM, seed).astype(np.int64)
    lo, hi = w & 0xFFFF, w >> 16
    s = (lo[..., 0] + hi[..., 0] + lo[..., 1] + hi[..., 1]) - (lo[..., 2] + hi[..., 2] + lo[..., 3] + hi[..., 3])
    return s.astype(F32) * KSCALE


def draws_of(cfg, words, noise_rows, noise_T, noise_lengths):
    """One row's eight words -> (applied, k, o, m, snr_i, gain_i)"""
    w = [int(v) for v in words]
    N = noise_rows
    applied = int(N > 0 and (w[0] * 65536) >> 32 < cfg[4])
    k = (w[1] * N) >> 32
    m = 0
    if N > 0:
        m = noise_T if noise_lengths is None else min(max(int(noise_lengths[k]), 0), noise_T)
    o = (w[2] * m) >> 32
    if m == 0:
        applied = k = 0
    return applied, k, o, m, (w[3] * (cfg[1] - cfg[0] + 1)) >> 32, (w[4] * (cfg[3] - cfg[2] + 1)) >> 32


# ---- the energies --------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """fmaf over float32 arrays of one shape: fma32 where every operand is finite. fma32's error terms are NaN where one is not;
    there the double a b + c, rounded, is fmaf's own answer: the product of two floats is exact in double and cannot overflow, so
    the sum is an infinity or a NaN exactly where fmaf's is (which NaN is the platform's choice: compare with same_or_nan)"""
    with np.errstate(all="ignore"):
        r = fma32(a, b, c)
        odd = ~(np.isfinite(a) & np.isfinite(b) & np.isfinite(c))
        if odd.any():
            r[odd] = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)[odd]
    return r


def same_or_nan(a, b):
    """same_bits, but a NaN equals any NaN: x86 and gfx950 may differ in the sign and the payload of a NaN they generate"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def energy(v):
    """v float32 [n] -> the header's sum of squares, float32"""
    total = F32(0.0)
    for c0 in range(0, len(v), TILE):
        ch = v[c0:c0 + TILE]
        ch = np.concatenate([ch, np.zeros(-len(ch) % LANES, F32)]).reshape(-1, LANES)  # fma(0, 0, acc) is acc
        acc = np.zeros(LANES, F32)
        with np.errstate(all="ignore"):
            for line in ch:
                acc = fma(line, line, acc)
            s = LANES // 2
            while s:
                acc[:s] = acc[:s] + acc[s:2 * s]
                s //= 2
            total = F32(total + acc[0])
    return total


def chain_length(n):
    """The additions on the longest path from a sample to Ex: the lane's chain, the tree's 8, the chunks"""
    return min(n, TILE) // LANES + (1 if min(n, TILE) % LANES else 0) + 8 + (n + TILE - 1) // TILE


def reference(x, lengths, cfg, seed, noise=None, noise_lengths=None, row_base=0, ids=None, dither=0.0, pad_value=0.0):
    """x [rows, T] float32 -> (y of the same shape, draws int32 [rows, 5], stats float32 [rows, 4])"""
    rows, T = x.shape
    N, Tn = (0, 0) if noise is None or noise.size == 0 else noise.shape
    snr, gain = tables(cfg)
    draws, stats = np.zeros((rows, 5), np.int32), np.zeros((rows, 4), F32)
    idents = [(int(ids[r]) if ids is not None else row_base + r) & M64 for r in range(rows)]
    words = row_words(seed, idents)
    for r, n in enumerate(clamp_lengths(lengths, rows, T)):
        applied, k, o, m, si, gi = draws_of(cfg, words[r], N, Tn, noise_lengths)
        draws[r] = (applied, k, o, cfg[0] + si, cfg[2] + gi)
        v = x[r, :n]
        ex = energy(v)
        z = noise[k][(o + np.arange(n)) % m] if applied else None
        en = energy(z) if applied else F32(0.0)
        a = gain[gi]
        b = F32(0.0)
        if applied and ex > 0 and en > 0 and np.isfinite(ex) and np.isfinite(en):
            with np.errstate(all="ignore"):
                b = F32(F32(np.sqrt(F32(ex / en))) * snr[si]) * a
        stats[r] = (ex, en, a, b)
    return formula(x, lengths, cfg, seed, draws, stats, noise, noise_lengths, row_base, ids, dither, pad_value), draws, stats


def formula(x, lengths, cfg, seed, draws, stats, noise=None, noise_lengths=None, row_base=0, ids=None, dither=0.0, pad_value=0.0):
    """The output out of given draws (k and o) and stats (a and b): v = a x; b != 0: fma(b, z, v); dither != 0: fma(dither, g, v);
    clamp; pad_value from n_r on"""
    rows, T = x.shape
    y = np.full(x.shape, F32(pad_value), F32)
    for r, n in enumerate(clamp_lengths(lengths, rows, T)):
        ident = (int(ids[r]) if ids is not None else row_base + r) & M64
        a, b = F32(stats[r][2]), F32(stats[r][3])
        v = x[r, :n]
        with np.errstate(all="ignore"):
            out = a * v
            if b != 0:
                k, o = int(draws[r][1]), int(draws[r][2])
                m = noise.shape[1] if noise_lengths is None else min(max(int(noise_lengths[k]), 0), noise.shape[1])
                out = fma(np.full(n, b, F32), noise[k][(o + np.arange(n)) % m], out)
            if dither != 0:
                out = fma(np.full(n, dither, F32), dither_variates(seed, ident, np.arange(n)), out)
            if cfg[5]:
                out = np.where(out < -1, F32(-1), np.where(out > 1, F32(1), out))
        y[r, :n] = out
    return y


# ---- buffers -------------------------------------------------------------------------------------------------------------
def lay_out(x, gap=0, lead=0, fill=np.nan):
    """The logical x [rows, T] in a flat float32 buffer of `fill` whose row 0 starts `lead` elements behind a 16-byte boundary, rows
    T + gap apart, 8 elements behind the last -> (buffer, the offset of row 0 in it, the writable view [rows, T], the row stride)"""
    rows, T = x.shape
    rs = T + gap
    buf = np.full(4 + lead + rows * rs + 8, fill, F32)
    off = (-(buf.ctypes.data // 4) % 4) + lead
    view = np.lib.stride_tricks.as_strided(buf[off:], (rows, T), (4 * rs, 4))
    view[...] = x
    return buf, off, view, rs


def outside(buf, off, shape, rs):
    mask = np.ones(buf.shape, bool)
    np.lib.stride_tricks.as_strided(mask[off:], shape, (rs, 1))[...] = False
    return buf[mask]


def waves(rng, rows, T, scale=0.3):
    return (scale * rng.standard_normal((rows, T))).astype(F32)


# ---- the shared cases of the second look ---------------------------------------------------------------------------------
# Each is a dict: x [rows, T], lengths, cfg, dither, bank, bl (the bank's lengths), row_base. They are built once per process.
CLIP_LENGTHS = (3, 5, 100, 255, 256, 300, 1000, TILE - 1)
LONG_T = 513 * TILE + 5
SPECIALS = np.array([-0.0, 1.0, -1.0, np.nextafter(F32(1), F32(2)), np.nextafter(F32(-1), F32(-2))], F32)


@functools.lru_cache(maxsize=None)
def long_rows_case():
    """Six rows of up to 513 chunks under the "all" set: the finish kernel walks the partials 256 chunks at a time, so the lengths
    stand on both sides of its first and second block edge; o + t0 and the dither counters pass 2^21. row_base is the first at
    which every row with a sample draws noise and both clips are drawn, found from the draws alone"""
    rng = np.random.default_rng(4300)
    cfg, dither = PARAMS["all"]
    lengths = [LONG_T, 256 * TILE, 256 * TILE + 1, 0, 257 * TILE - 1, 512 * TILE + 1]
    bl = [5000, 257]
    for row_base in range(1000):
        d = [draws_of(cfg, w, 2, 5000, bl) for w in row_words(SEED, [row_base + r for r in range(6)])]
        if all(e[0] for e in d) and {e[1] for e in d} == {0, 1}:
            break
    return dict(x=waves(rng, 6, LONG_T), lengths=lengths, cfg=cfg, dither=dither, bank=waves(rng, 2, 5000, 0.1), bl=bl, row_base=row_base)


@functools.lru_cache(maxsize=None)
def clip_case(m):
    """Both clips m samples long under a noise probability of 1, at T = 2 tile + 3: for m < tile every work item of stage_noise
    walks the clip in steps of 256 mod m, chunk 1 starts at (o + 4096) mod m, and the last chunk is short"""
    rng = np.random.default_rng(4200 + m)
    T = 2 * TILE + 3
    return dict(x=waves(rng, 6, T), lengths=lengths_of(T), cfg=(5 * 256, 20 * 256, -6 * 256, 3 * 256, 65536, 0), dither=0.0,
                bank=waves(rng, 2, TILE, 0.1), bl=[m, m], row_base=11)


@functools.lru_cache(maxsize=None)
def edge_cases(clamp):
    """name -> case. Edge values inside the valid samples, under noise at probability 1, dither 0.01, clamp 0 / 1, T = tile + 7.
    "rows": a bank of ordinary amplitude under rows of amplitude 1e-20 (the squares are subnormal, Ex is normal), 1e-23 (Ex is
    subnormal), 3e19 (Ex = +Inf, so b = 0), an ordinary row with one NaN sample (Ex = NaN, b = 0, the sample stays NaN through the
    clamp), one with a +Inf sample in its second chunk, and one that starts with -0.0, 1, -1 and the floats next above 1 and next
    below -1. "bank ...": ordinary rows under one clip of amplitude 3e19, with a NaN sample, with a +Inf sample, with the
    special values; "tiny ...": rows and clip both of amplitude 1e-20, and both 1e-23, so that En is built of subnormals too.
    Left out on purpose: an ordinary row under a clip of amplitude around 1e-20. There sqrt(Ex / En) overflows, the header
    yields b = +Inf by its own definition, and fma32 cannot take an infinite factor; no audio reaches that case"""
    rng = np.random.default_rng(4100 + clamp)
    T = TILE + 7
    base = dict(cfg=(5 * 256, 20 * 256, -6 * 256, 3 * 256, 65536, clamp), dither=0.01, row_base=11)
    x = waves(rng, 6, T)
    x[0], x[1], x[2] = waves(rng, 1, T, 1e-20)[0], waves(rng, 1, T, 1e-23)[0], waves(rng, 1, T, 3e19)[0]
    x[3, 1234], x[4, TILE + 4], x[5, :5] = np.nan, np.inf, SPECIALS
    cases = {"rows": dict(base, x=x, lengths=[T, T - 1, T, T, T, 300], bank=waves(rng, 2, 3000, 0.1), bl=[3000, 257])}
    plain, lengths, m = waves(rng, 6, T), [T, 700, T - 1, 257, T, 1000], 700
    clips = {"bank 3e19": waves(rng, 1, m, 3e19), "bank nan": waves(rng, 1, m, 0.1), "bank inf": waves(rng, 1, m, 0.1),
             "bank specials": waves(rng, 1, m, 0.1)}
    clips["bank nan"][0, 333], clips["bank inf"][0, 400], clips["bank specials"][0, :5] = np.nan, np.inf, SPECIALS
    for name, clip in clips.items():
        cases[name] = dict(base, x=plain, lengths=lengths, bank=clip, bl=[m])
    for scale in (1e-20, 1e-23):
        cases["tiny %g" % scale] = dict(base, x=waves(rng, 6, T, scale), lengths=lengths, bank=waves(rng, 1, m, scale), bl=[m])
    return cases


def case_kw(case):
    """The keywords of reference, formula and host_values that a case sets"""
    return dict(row_base=case["row_base"], dither=case["dither"])


# ---- the host build ------------------------------------------------------------------------------------------------------
def build_waveaug_sim():
    L = host_build.shared("waveaug_sim.cpp", "libwaveaug_sim.so", host_build.SIM_FP)
    vp, q, f32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_float
    L.waveaug_sim_philox.argtypes = [vp, vp, vp]
    L.waveaug_sim_plan.argtypes = [vp, f32, vp, vp, vp]
    L.waveaug_sim_run.argtypes = [vp, f32, f32, vp, q, q, q, vp, vp, q, q, q, vp, q, q, vp, vp, q, vp, vp]
    return L


def build_waveaug_shim(pkg):
    """tests/host_sim/waveaug_shim.cpp over host/wave_augment.hpp, linked with the library"""
    L = host_build.shared("waveaug_shim.cpp", "libwaveaug_shim.so", host_build.SHIM, host_build.library(pkg))
    vp, sz, q = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    L.waveaug_shim_create.restype = ctypes.c_long
    L.waveaug_shim_create.argtypes = [vp]
    L.waveaug_shim_run.restype = ctypes.c_long
    L.waveaug_shim_run.argtypes = [vp, vp, sz, sz, sz, vp, vp, sz, sz, sz, vp, q, q, vp, vp, sz, vp, vp, vp, vp]
    L.waveaug_shim_sizes.argtypes = [vp]
    L.waveaug_shim_last_error.restype = ctypes.c_char_p
    return L


def config_words(cfg):
    return np.array(cfg, np.int64).astype(np.int32)


def sim_philox(L, counter, key):
    c, k, out = np.array(counter, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    L.waveaug_sim_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return [int(v) for v in out]


def sim_plan(L, cfg, dither=0.0):
    """-> (return code, info dict, snr table, gain table)"""
    info, words = np.zeros(5, np.uint32), config_words(cfg)
    rc = L.waveaug_sim_plan(words.ctypes.data, dither, info.ctypes.data, None, None)
    if rc:
        return rc, None, None, None
    snr, gain = np.zeros(int(info[2]), F32), np.zeros(int(info[3]), F32)
    L.waveaug_sim_plan(words.ctypes.data, dither, info.ctypes.data, snr.ctypes.data, gain.ctypes.data)
    return rc, dict(zip(("tile", "draws", "snr_entries", "gain_entries", "lds_bytes"), (int(v) for v in info))), snr, gain


def ptr(a):
    return None if a is None else a.ctypes.data


def host_run(L, cfg, in_ptr, in_rs, rows, T, lengths, seed, out_ptr, out_rs, noise_ptr=None, noise_rs=0, noise_rows=0, noise_T=0,
             noise_lengths=None, draws=None, stats=None, row_base=0, ids=None, dither=0.0, pad_value=0.0):
    """waveaug_sim_run over raw pointers -> its return code"""
    ln = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
    nl = None if noise_lengths is None else np.ascontiguousarray(noise_lengths, np.int32)
    idv = None if ids is None else np.ascontiguousarray(ids, np.int64)
    words = config_words(cfg)
    return L.waveaug_sim_run(words.ctypes.data, dither, pad_value, in_ptr, in_rs, rows, T, ptr(ln), noise_ptr, noise_rs, noise_rows,
                             noise_T, ptr(nl), seed, row_base, ptr(idv), out_ptr, out_rs, ptr(draws), ptr(stats))


def host_values(L, x, lengths, cfg, seed, noise=None, noise_lengths=None, want_stats=True, **kw):
    """The host build over dense copies -> (y [rows, T], draws [rows, 5], stats [rows, 4] or None)"""
    rows, T = x.shape
    xin, y = np.ascontiguousarray(x), np.zeros(x.shape, F32)
    draws, stats = np.full((rows, 5), -77, np.int32), (np.full((rows, 4), -77.0, F32) if want_stats else None)
    nz = None if noise is None else np.ascontiguousarray(noise)
    N, Tn = (0, 0) if nz is None else nz.shape
    rc = host_run(L, cfg, xin.ctypes.data, T, rows, T, lengths, seed, y.ctypes.data, T, ptr(nz), Tn, N, Tn, noise_lengths, draws, stats,
                  **kw)
    assert rc == 0, rc
    return y, draws, stats
