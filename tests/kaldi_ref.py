"""Kaldi's fbank and MFCC features restated in numpy float64 STEP BY STEP (cut frames, remove the mean, pre-emphasise, window,
pad, numpy.fft.rfft), independently of csrc/alac_fbank.h, which folds those steps into its basis; the case
table of both suites; and the host build of that header (tests/host_sim/fbank_sim.cpp) for the tests.

    W = frame length, h = frame shift, N = next power of two >= W (round_to_power_of_two) else W, K = N / 2 + 1
    snip_edges: F = 1 + (T - W) / h, frame f reads x[f h + n]; otherwise F = (T + h / 2) / h, frame f reads the reflected x
    (index i < 0 is -1 - i, i >= T is 2 T - 1 - i) at f h - (W / 2 - h / 2) + n; no frame for T < W
    per frame: v = scale x; v -= mean(v); energy = sum v^2; y[n] = v[n] - c v[n - 1], v[-1] = v[0]; y *= window; zeros up to N
    p = |rfft(y)|^2;  mel = fb p, fb = Kaldi's get_mel_banks in double, rounded to float32;  ln(max(., 2^-23))
    MFCC = lifter[c] * sum_m D[c][m] logmel[m]; htk_compat moves column 0 to the end, and where that is C0 (no use_energy)
    it leaves as sqrt(2) C0: D's row 0 is sqrt(2 / M) there"""
import ctypes
import math

import numpy as np

from tests import host_build
from tests import mel_ref as mr

ROOT = mr.ROOT
U = mr.U
EPS = 2.0 ** -23
WINDOWS = {"hanning": 0, "hamming": 1, "povey": 2, "rectangular": 3, "blackman": 4}
LAYOUTS = {"frames": 0, "bins": 1}
LOG_ULPS = 2.0 * 2.23  # twice what DESIGN.md §14 measured for the device's logf against float64, in float32 ulps
LDS_FLOATS = 16384
OFFSETS = mr.OFFSETS


class Cfg:
    """One parameter set of the handle, lengths in samples."""

    def __init__(self, rate, W, h, mels=23, ceps=0, pow2=True, snip=True, dc=True, window="povey", log=True, energy=False, htk=False,
                 log_energy=True, layout="frames", pre=0.97, blackman=0.42, low=20.0, high=0.0, efloor=1.0, scale=1.0, lifter=22.0):
        self.rate, self.W, self.h, self.mels, self.ceps = rate, W, h, mels, ceps
        self.pow2, self.snip, self.dc, self.window, self.log = pow2, snip, dc, window, log
        self.energy, self.htk, self.log_energy, self.layout = energy, htk, log_energy, layout
        self.pre, self.blackman, self.low, self.high, self.efloor, self.scale, self.lifter = pre, blackman, low, high, efloor, scale, lifter

    @property
    def N(self):
        return 1 << (self.W - 1).bit_length() if self.pow2 else self.W

    @property
    def K(self):
        return self.N // 2 + 1

    @property
    def cols(self):
        return self.ceps if self.ceps else self.mels + int(self.energy)

    @property
    def pad(self):
        return 0 if self.snip else self.W // 2 - self.h // 2

    def with_(self, **kw):
        c = Cfg.__new__(Cfg)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c

    def prelog(self):
        """The same pass with nothing logged: fbank without use_log_fbank, the energy column as the sum itself"""
        return self.with_(ceps=0, log=False, log_energy=False)

    def words(self, dither=0.0, vtln=1.0, use_power=1, raw_energy=1):
        """-> (uint32[16], float64[9]) as tests/host_sim/fbank_sim.cpp reads them"""
        return (np.array([self.rate, self.W, self.h, int(self.pow2), self.mels, self.ceps, int(self.snip), int(self.dc),
                          WINDOWS[self.window], int(self.log), int(self.energy), raw_energy, int(self.htk), use_power,
                          int(self.log_energy), LAYOUTS[self.layout]], np.uint32),
                np.array([self.pre, self.blackman, self.low, self.high, self.efloor, self.scale, self.lifter, dither, vtln], np.float64))

    def kwargs(self):
        """The keyword arguments of pkg.KaldiFeatures"""
        return dict(sample_rate=self.rate, frame_length=self.W, frame_shift=self.h, num_mel_bins=self.mels, num_ceps=self.ceps,
                    round_to_power_of_two=self.pow2, snip_edges=self.snip, remove_dc_offset=self.dc, window_type=self.window,
                    use_log_fbank=self.log, use_energy=self.energy, htk_compat=self.htk, log_energy=self.log_energy,
                    layout=self.layout, preemphasis_coefficient=self.pre, blackman_coeff=self.blackman, low_freq=self.low,
                    high_freq=self.high, energy_floor=self.efloor, scale=self.scale, cepstral_lifter=self.lifter)


# ---- the definition, step by step --------------------------------------------------------------------------------------
def window(cfg):
    W = cfg.W
    if W == 1 or cfg.window == "rectangular":
        return np.ones(W)
    a = 2.0 * np.pi / (W - 1)
    n = np.arange(W)
    if cfg.window == "hanning":
        return 0.5 - 0.5 * np.cos(a * n)
    if cfg.window == "hamming":
        return 0.54 - 0.46 * np.cos(a * n)
    if cfg.window == "povey":
        return (0.5 - 0.5 * np.cos(a * n)) ** 0.85
    return cfg.blackman - 0.5 * np.cos(a * n) + (0.5 - cfg.blackman) * np.cos(2 * a * n)


def out_frames(cfg, T):
    if T < cfg.W:
        return 0
    return 1 + (T - cfg.W) // cfg.h if cfg.snip else (T + cfg.h // 2) // cfg.h


def length_for(cfg, F):
    """The shortest T >= W with out_frames(T) == F; where the shortest row, T = W, already has more frames, that row"""
    T = cfg.W + (F - 1) * cfg.h if cfg.snip else max(cfg.W, F * cfg.h - cfg.h // 2)
    assert out_frames(cfg, T) == F or (T == cfg.W and out_frames(cfg, T) > F), (T, F, out_frames(cfg, T))
    return T


def frame_index(cfg, T):
    """[F, W] indices into a row of T samples, Kaldi's reflection resolved"""
    F = out_frames(cfg, T)
    idx = np.arange(F)[:, None] * cfg.h - cfg.pad + np.arange(cfg.W)[None, :]
    if not cfg.snip:
        idx = np.where(idx < 0, -1 - idx, idx)
        idx = np.where(idx >= T, 2 * T - 1 - idx, idx)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < T), "a frame reaches outside the row"
    return idx


def raw_frames(cfg, x):
    """x [R, T] float32 -> [R, F, W] float64, not yet scaled"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    return x[:, frame_index(cfg, x.shape[1])]


def stepwise(cfg, x):
    """-> (power [R, F, K], energy [R, F] before its log), float64, one step after the other"""
    v = raw_frames(cfg, x) * cfg.scale
    if cfg.dc:
        v = v - v.mean(axis=-1, keepdims=True)
    energy = (v * v).sum(axis=-1)
    if cfg.pre != 0.0:
        prev = np.concatenate([v[..., :1], v[..., :-1]], axis=-1)
        v = v - cfg.pre * prev
    v = v * window(cfg)
    spec = np.fft.rfft(v, n=cfg.N, axis=-1)  # pads with zeros up to N
    return spec.real ** 2 + spec.imag ** 2, energy


def mel_of(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def mel_banks(cfg):
    """get_mel_banks in float64 -> [M, K]; the bins from N / 2 on weigh 0"""
    M, N, K = cfg.mels, cfg.N, cfg.K
    nyquist = 0.5 * cfg.rate
    high = cfg.high + nyquist if cfg.high <= 0.0 else cfg.high
    assert 0.0 <= cfg.low < nyquist and 0.0 < high <= nyquist and cfg.low < high
    m_low, m_high = float(mel_of(cfg.low)), float(mel_of(high))
    delta = (m_high - m_low) / (M + 1)
    b = np.arange(M)[:, None]
    left, centre, right = m_low + b * delta, m_low + (b + 1) * delta, m_low + (b + 2) * delta
    mk = mel_of((cfg.rate / N) * np.arange(N // 2))[None, :]
    w = np.maximum(0.0, np.minimum((mk - left) / (centre - left), (right - mk) / (right - centre)))
    fb = np.zeros((M, K))
    fb[:, :N // 2] = w
    return fb


def folded(cfg):
    """The folded basis in float64 [2][K][W], as the issue defines it: what the plan's tables must be within one float32 ulp of"""
    W, N, K, c = cfg.W, cfg.N, cfg.K, cfg.pre
    r = (np.arange(K, dtype=np.int64)[:, None] * np.arange(W, dtype=np.int64)[None, :]) % N
    ang = 2.0 * np.pi * r / N
    out = []
    for A in (window(cfg)[None, :] * np.cos(ang), window(cfg)[None, :] * np.sin(ang)):
        G = A.copy()
        G[:, :-1] -= c * A[:, 1:]
        G[:, 0] -= c * A[:, 0]
        if cfg.dc:
            G = G - G.sum(axis=1, keepdims=True) / W
        out.append(cfg.scale * G)
    return np.stack(out)


def dct_matrix(cfg):
    """[ceps, M]; row 0 is sqrt(1 / M), or sqrt(2 / M) where C0 itself leaves in the last column (htk_compat without use_energy:
    Kaldi and torchaudio multiply it by sqrt(2) there), so that arrange only permutes"""
    M = cfg.mels
    D = math.sqrt(2.0 / M) * np.cos(np.pi * (np.arange(M)[None, :] + 0.5) * np.arange(cfg.ceps)[:, None] / M)
    D[0] = math.sqrt((2.0 if cfg.htk and not cfg.energy else 1.0) / M)
    return D


def lifter(cfg):
    c = np.arange(cfg.ceps)
    return 1.0 + 0.5 * cfg.lifter * np.sin(np.pi * c / cfg.lifter) if cfg.lifter != 0.0 else np.ones(cfg.ceps)


def log_energy64(cfg, e):
    v = np.log(np.maximum(e, EPS))
    return np.maximum(v, math.log(cfg.efloor)) if cfg.efloor > 0.0 else v


def arrange(cfg, body, energy):
    """body [R, F, n] and energy [R, F] -> [R, F, cols]: the energy column first, or last with htk_compat; for MFCC it takes
    coefficient 0's place, which htk_compat moves to the end"""
    if cfg.ceps:
        if cfg.energy:
            body = np.concatenate([energy[..., None], body[..., 1:]], axis=-1)
        return np.concatenate([body[..., 1:], body[..., :1]], axis=-1) if cfg.htk else body
    if not cfg.energy:
        return body
    return np.concatenate([body, energy[..., None]] if cfg.htk else [energy[..., None], body], axis=-1)


def features64(cfg, x, fb=None):
    """The whole definition in float64 -> [R, F, cols] (fb: a dense [M, K] filterbank in place of the float32-rounded
    restatement)"""
    p, e = stepwise(cfg, x)
    fb = np.asarray(mel_banks(cfg).astype(np.float32) if fb is None else fb, np.float64)
    mel = np.einsum("mk,rfk->rfm", fb, p)
    if cfg.log_energy:
        e = log_energy64(cfg, e)
    if cfg.ceps:
        body = np.einsum("cm,rfm->rfc", dct_matrix(cfg), np.log(np.maximum(mel, EPS))) * lifter(cfg)
    else:
        body = np.log(np.maximum(mel, EPS)) if cfg.log else mel
    return arrange(cfg, body, e)


def dense_fb(plan):
    fb = np.zeros((plan["num_mel_bins"], plan["n_freqs"]), np.float32)
    for m in range(plan["num_mel_bins"]):
        fb[m, plan["first"][m]:plan["first"][m] + plan["taps"]] = plan["fb"][m]
    return fb


# ---- the ceilings ------------------------------------------------------------------------------------------------------
def prelog_bounds(cfg, plan, x):
    """The ceilings of the float32 chains against the step-by-step restatement, u = 2^-24 (DESIGN.md §14's, with W + 1 for N: the
    chain's W roundings and the folded table's own), for a cfg with nothing logged:
        e_r = (W + 1) u sum |C x|, e_i likewise;  dp = (2 |re| e_r + 2 |im| e_i + e_r^2 + e_i^2)(1 + 2 u) + 2 u p
        dmel = sum fb dp + taps u sum fb (p + dp)
        energy: dm = (W + 1) u sum |x| / W (the float32 mean), d = x - mean;
                de = scale^2 ((W + 2) u sum d^2 + 2 dm sum |d| + W dm^2)
    -> (ref [R, F, cols], lim [R, F, cols])"""
    assert not cfg.ceps and not cfg.log and not cfg.log_energy
    B = np.asarray(plan["basis"], np.float64)
    fr = raw_frames(cfg, x)
    W = cfg.W
    spec_in = stepwise(cfg, x)
    p, e = spec_in
    # |re|, |im| of the restatement: from the folded float64 tables, which agree with the steps to 1e-15 of the largest bin
    Fd = folded(cfg)
    re = np.einsum("kn,rfn->rfk", Fd[0], fr)
    im = np.einsum("kn,rfn->rfk", Fd[1], fr)
    er = (W + 1) * U * np.einsum("kn,rfn->rfk", np.abs(B[0]), np.abs(fr))
    ei = (W + 1) * U * np.einsum("kn,rfn->rfk", np.abs(B[1]), np.abs(fr))
    dp = (2 * np.abs(re) * er + 2 * np.abs(im) * ei + er * er + ei * ei) * (1 + 2 * U) + 2 * U * p
    fb = np.asarray(dense_fb(plan), np.float64)
    mel = np.einsum("mk,rfk->rfm", fb, p)
    dmel = np.einsum("mk,rfk->rfm", fb, dp) + plan["taps"] * U * np.einsum("mk,rfk->rfm", fb, p + dp)
    mean = fr.mean(axis=-1, keepdims=True) if cfg.dc else np.zeros(fr.shape[:-1] + (1,))
    d = np.abs(fr - mean)
    dm = ((W + 1) * U * np.abs(fr).sum(axis=-1) / W) if cfg.dc else np.zeros(fr.shape[:-1])
    de = cfg.scale ** 2 * ((W + 2) * U * (d * d).sum(axis=-1) + 2 * dm * d.sum(axis=-1) + W * dm * dm)
    return arrange(cfg, mel, e), arrange(cfg, dmel, de)


def assert_within(got, ref, lim, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    ok = err <= lim
    assert ok.all(), "%s: error %g above the ceiling %g (value %g)" % (what, err[~ok][0], lim[~ok][0], ref[~ok][0])
    return float((err / np.maximum(lim, 1e-300)).max())


def log_of_prelog(cfg, pre32):
    """What a logging pass must give, in float64, from the SAME build's pre-log values pre32 [R, F, M (+ 1)] (cfg.prelog()'s
    output): -> (want [R, F, cols], lim [R, F, cols], exact [R, F, cols] bool: where the value is pinned bit for bit)."""
    pre = np.asarray(pre32, np.float64)
    M = cfg.mels
    if cfg.energy:
        e, mel = (pre[..., M], pre[..., :M]) if cfg.htk else (pre[..., 0], pre[..., 1:])
    else:
        e, mel = np.zeros(pre.shape[:-1]), pre
    # the floors: at or below eps the result is ln(eps) itself; an energy the floor raises is ln(energy_floor) itself
    le = log_energy64(cfg, e)
    e_exact = (e <= EPS) | ((le <= math.log(cfg.efloor)) if cfg.efloor > 0.0 else False)
    e_lim = LOG_ULPS * spacing32(le)
    if not cfg.log_energy:
        le, e_exact, e_lim = e, np.ones(e.shape, bool), np.zeros(e.shape)
    lm = np.log(np.maximum(mel, EPS))
    lm_lim = np.where(mel <= EPS, 0.0, LOG_ULPS * spacing32(lm))
    if cfg.ceps:
        D = dct_matrix(cfg).astype(np.float32).astype(np.float64)
        L = lifter(cfg).astype(np.float32).astype(np.float64)
        body = np.einsum("cm,rfm->rfc", D, lm) * L
        lim = (np.einsum("cm,rfm->rfc", np.abs(D), lm_lim) + M * U * np.einsum("cm,rfm->rfc", np.abs(D), np.abs(lm))) * np.abs(L)
        exact = np.zeros(body.shape, bool)
    elif cfg.log:
        body, lim, exact = lm, lm_lim, mel <= EPS
    else:
        body, lim, exact = mel, np.zeros(mel.shape), np.ones(mel.shape, bool)
    return arrange(cfg, body, le), arrange(cfg, lim, e_lim), arrange(cfg, exact, e_exact).astype(bool)


def spacing32(v64):
    w32 = np.abs(np.asarray(v64, np.float64).astype(np.float32))
    return np.spacing(np.maximum(w32, np.float32(2.0 ** -126))).astype(np.float64)


def check_logged(cfg, got32, pre32, what):
    """got32 [R, F, cols] of a logging pass against log_of_prelog -> the largest error / bound among the values not pinned"""
    want, lim, exact = log_of_prelog(cfg, pre32)
    pinned = want.astype(np.float32)
    same = got32.view(np.uint32) == pinned.view(np.uint32)
    assert same[exact].all(), "%s: a floored or unlogged value is not exact" % what
    err = np.abs(got32.astype(np.float64) - want)
    ok = (err <= lim) | exact
    assert ok.all(), "%s: error %g above the bound %g" % (what, err[~ok][0], lim[~ok][0])
    free = ~exact & (lim > 0)
    return float((err[free] / lim[free]).max()) if free.any() else 0.0


# ---- the LDS rule --------------------------------------------------------------------------------------------------------
def lds_rule(cfg):
    """tile_frames: 64 halved down to 4 until the tile's floats fit 64 KB: the staging image (or the mel tile in its place, with
    fbank's energy column), the power tile [tile_frames][K | 1], tile_frames of energy, and MFCC's [num_ceps][tile_frames]"""
    def need(tf):
        a = (tf - 1) * cfg.h + cfg.W + 3 if cfg.h <= cfg.W else tf * cfg.W
        a = max(a, (cfg.mels + (1 if cfg.energy and not cfg.ceps else 0)) * tf)
        a = (a + 3) // 4 * 4
        return a + tf * (cfg.K | 1) + (tf if cfg.energy else 0) + cfg.ceps * tf
    tf = 64
    while tf > 4 and need(tf) > LDS_FLOATS:
        tf //= 2
    return tf, need(tf)


# ---- the host build ------------------------------------------------------------------------------------------------------
def build_fbank_sim():
    L = host_build.shared("fbank_sim.cpp", "libfbank_sim.so", host_build.SIM_FP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.fbank_sim_plan.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64]
    L.fbank_sim_run.argtypes = [vp, vp, vp, u64, u64, u64, vp, u64, u64, ctypes.c_int]
    L.fbank_sim_out_frames.restype, L.fbank_sim_out_frames.argtypes = u64, [vp, vp, u64]
    L.fbank_sim_lds_floats.restype = ctypes.c_uint32
    return L


def build_fbank_shim(pkg):
    """tests/host_sim/fbank_shim.cpp over host/kaldi_features.hpp, linked with the library"""
    L = host_build.shared("fbank_shim.cpp", "libfbank_shim.so", host_build.SHIM, host_build.library(pkg))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.fbank_shim_run.restype = ctypes.c_long
    L.fbank_shim_run.argtypes = [vp, vp, sz, sz, sz, vp, sz, sz, vp, vp, vp]
    L.fbank_shim_last_error.restype = ctypes.c_char_p
    return L


INFO = ("frame_length", "frame_shift", "n_fft", "n_freqs", "num_mel_bins", "taps", "num_ceps", "cols", "tile_frames", "lds_bytes")
TABLES = ("basis", "fb", "first", "dct", "lifter")


def sim_plan(S, cfg, **refused):
    """-> dict of the host build's plan (INFO and TABLES), or None where it has none"""
    w, d = cfg.words(**refused)
    info = np.zeros(10, np.uint32)
    if S.fbank_sim_plan(w.ctypes.data, d.ctypes.data, info.ctypes.data, None, 0, None, 0, None, 0, None, 0, None, 0) != 0:
        return None
    out = {k: int(v) for k, v in zip(INFO, info)}
    b = np.zeros((2, out["n_freqs"], out["frame_length"]), np.float32)
    fb = np.zeros((out["num_mel_bins"], out["taps"]), np.float32)
    first = np.zeros(out["num_mel_bins"], np.int32)
    dct = np.zeros((out["num_ceps"], out["num_mel_bins"]), np.float32)
    lif = np.zeros(out["num_ceps"], np.float32)
    assert S.fbank_sim_plan(w.ctypes.data, d.ctypes.data, info.ctypes.data, b.ctypes.data, b.size, fb.ctypes.data, fb.size,
                            first.ctypes.data, first.size, dct.ctypes.data, dct.size, lif.ctypes.data, lif.size) == 0
    out.update(basis=b, fb=fb, first=first, dct=dct, lifter=lif)
    return out


def same_plan(a, b):
    return all(a[k] == b[k] for k in INFO) and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in TABLES)


def sim_out_frames(S, cfg, T):
    w, d = cfg.words()
    return S.fbank_sim_out_frames(w.ctypes.data, d.ctypes.data, T)


# ---- buffers, shared by the CPU and the GPU suite ------------------------------------------------------------------------
def out_shape(cfg, F):
    """(lines, length) of a row's output: F lines of cols (frames), or cols lines of F (bins)"""
    return (F, cfg.cols) if cfg.layout == "frames" else (cfg.cols, F)


def layout(cfg, rows, T, in_off=0, out_off=0, pad=0):
    """mr.layout for this pass: odd strides and guard elements; pad widens the inner (frame or bin) stride"""
    lines, length = out_shape(cfg, out_frames(cfg, T))
    return mr.layout(rows, T, lines, length, in_off, out_off, pad)


def sim_image(S, cfg, x, in_off=0, out_off=0, pad=0, guard=0):
    """The rows x laid out with an odd stride in_off elements behind a 16-byte boundary, NaN between them, the pass of the host
    build into a sentinel-filled buffer -> (image uint32, layout)"""
    rows, T = x.shape
    lay = layout(cfg, rows, T, in_off, out_off, pad)
    in_stride, in_lead, in_elems, row_stride, inner, out_lead, out_elems = lay
    src = mr.aligned(in_elems, 0x7FC00000)
    for r in range(rows):
        src[in_lead + r * in_stride: in_lead + r * in_stride + T] = x[r].view(np.uint32)
    img = mr.aligned(out_elems, mr.SENTINEL)
    w, d = cfg.words()
    rc = S.fbank_sim_run(w.ctypes.data, d.ctypes.data, src.ctypes.data + 4 * in_lead, in_stride, rows, T, img.ctypes.data + 4 * out_lead,
                         row_stride, inner, guard)
    assert rc == 0, rc
    return img.copy(), lay


def values_of(img, lay, cfg, rows, T, what=""):
    """[rows, F, cols] float32 out of an image of either layout, and a check that everything outside it is the sentinel"""
    lines, length = out_shape(cfg, out_frames(cfg, T))
    got = mr.rows_of(img, rows, lines, length, lay[5], lay[3], lay[4])
    assert np.array_equal(img, mr.expected_image(got, img.size, lay[5], lay[3], lay[4])), what + ": outside the output"
    return got if cfg.layout == "frames" else np.ascontiguousarray(got.transpose(0, 2, 1))


def image_of(cfg, y, elems, lay):
    """The whole buffer a pass must leave: y [rows, F, cols] at its places, the sentinel everywhere else"""
    y = y if cfg.layout == "frames" else np.ascontiguousarray(y.transpose(0, 2, 1))
    return mr.expected_image(np.ascontiguousarray(y), elems, lay[5], lay[3], lay[4])


def host_values(S, cfg, x):
    img, lay = sim_image(S, cfg, x)
    return values_of(img, lay, cfg, x.shape[0], x.shape[1])


def signal(rng, rows, T, offset=0.0):
    """mr.signal, optionally on a DC offset (clipped to [-1, 1])"""
    x = mr.signal(rng, rows, T)
    return np.clip(x + np.float32(offset), -1.0, 1.0).astype(np.float32) if offset else x


_LIBM = ctypes.CDLL("libm.so.6")
_LIBM.fmaf.restype = ctypes.c_float
_LIBM.fmaf.argtypes = [ctypes.c_float] * 3


def fmaf32(a, b, c):
    """libm's fmaf, elementwise over float32 arrays: one rounding, as the device's"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    out = np.array([_LIBM.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())], np.float32)
    return out.reshape(a.shape)


def impulse_expected(cfg, plan, T, j):
    """[F, M] float32 of a row of +0.0 with 1.0 at j, remove_dc_offset off and nothing logged, bit for bit from the tables alone:
    every fmaf with a zero sample leaves its accumulator as it is, so re and im of a frame are the entries under the impulse, or,
    where the reflection shows j more than once, their float32 sum in the order of n; p = fmaf(im, im, float32(re * re)); then
    the mel chain over q upwards from +0.0f. -> (want, frames that see j more than once)"""
    B = plan["basis"]
    idx = frame_index(cfg, T)
    M, taps, K = plan["num_mel_bins"], plan["taps"], cfg.K
    want = np.zeros((idx.shape[0], M), np.float32)
    twice = 0
    one = np.float32(1.0)
    for f in range(idx.shape[0]):
        ns = np.nonzero(idx[f] == j)[0]
        if not len(ns):
            continue
        twice += len(ns) >= 2
        re, im = np.zeros(K, np.float32), np.zeros(K, np.float32)
        for n in ns:
            re, im = fmaf32(B[0][:, n], one, re), fmaf32(B[1][:, n], one, im)
        p = fmaf32(im, im, re * re)  # float32 * float32 in numpy: the product rounded on its own
        acc = np.zeros(M, np.float32)
        for q in range(taps):
            acc = fmaf32(plan["fb"][:, q], p[plan["first"] + q], acc)
        want[f] = acc
    return want, twice


def impulse_cfg(cfg):
    """cfg as the impulse checks run it: no DC removal, nothing logged, no energy column, no DCT"""
    return cfg.with_(dc=False, log=False, energy=False, ceps=0, log_energy=False)


# ---- the parameter cases, shared by the CPU and the GPU suite ------------------------------------------------------------
# name -> (Cfg, tile_frames by the LDS rule). The path each case runs is the issue's table's.
W10 = Cfg(8000, 10, 4)
MF13 = Cfg(8000, 50, 20, ceps=13)
E_SCALE_FLOOR = 2.0 ** 30  # at scale 32768 the energy of a frame whose unscaled sum of squares is 1: mr.signal has both kinds
CASES = {
    "w8": (Cfg(8000, 8, 4, mels=4), 64),                                  # W = N
    "w10": (W10, 64),                                                     # W < N, one block and a tail of 2
    "w3": (Cfg(8000, 3, 1), 64),                                          # tail loop alone
    "w7": (Cfg(8000, 7, 3, pow2=False), 64),                              # odd N, K = 4
    "ns10": (Cfg(8000, 10, 4, snip=False), 64),                           # pad 3
    "ns9": (Cfg(8000, 9, 5, snip=False), 64),                             # pad 2, odd W
    "h37": (Cfg(8000, 16, 37), 64),                                       # h > W
    "h37ns": (Cfg(8000, 16, 37, snip=False), 64),                         # h > W, negative pad
    "hanning": (W10.with_(window="hanning"), 64),
    "hamming": (W10.with_(window="hamming"), 64),
    "rectangular": (W10.with_(window="rectangular"), 64),
    "blackman": (W10.with_(window="blackman"), 64),
    "nodc": (W10.with_(dc=False), 64),
    "c0": (W10.with_(pre=0.0), 64),
    "scale": (W10.with_(scale=32768.0), 64),
    "e_first_1": (W10.with_(energy=True, efloor=1.0), 64),
    "e_first_0": (W10.with_(energy=True, efloor=0.0), 64),
    "e_last_1": (W10.with_(energy=True, htk=True, efloor=1.0), 64),
    "e_last_0": (W10.with_(energy=True, htk=True, efloor=0.0), 64),
    "asr": (Cfg(16000, 400, 160, mels=80), 32),                           # the ASR front end, N 512
    "k48": (Cfg(48000, 1200, 480, mels=128), 8),                          # N 2048
    "full": (Cfg(48000, 2048, 2048, pow2=False), 4),                      # dft_blocks<4>
    "manymels": (Cfg(16000, 64, 16, mels=2048), 4),                       # output tile above the staging
    "mfcc13": (Cfg(8000, 50, 20, ceps=13), 64),                           # lifter 22
    "mfcc13_l0": (Cfg(8000, 50, 20, ceps=13, lifter=0.0), 64),            # no lifter
    "mfcc23": (Cfg(8000, 50, 20, ceps=23), 64),                           # num_ceps = M
    "mfcc_e_htk": (Cfg(8000, 50, 20, ceps=13, energy=True, htk=True), 64),
    "mfcc_htk": (MF13.with_(htk=True), 64),                               # C0 last, times sqrt(2)
    "mfcc_e": (MF13.with_(energy=True), 64),                              # energy in column 0, no permutation
    "mfcc_ns": (MF13.with_(snip=False), 64),                              # MFCC over reflected frames
    "mfcc_c1": (Cfg(8000, 50, 20, ceps=1), 64),                           # cols 1
    "mfcc_asr": (Cfg(16000, 400, 160, mels=23, ceps=13), 32),             # torchaudio's default MFCC
    "mfcc_hires": (Cfg(16000, 400, 160, mels=40, ceps=40, energy=True, htk=True, snip=False), 32),  # ceps = M, everything on
    "mfcc_full": (Cfg(48000, 2048, 2048, pow2=False, ceps=13, energy=True), 4),  # c_off behind a full tile
    "mfcc_many": (Cfg(16000, 64, 16, mels=2048, ceps=1024), 4),           # DCT chains of 2048, 4096 items per tile
    "m1": (W10.with_(mels=1), 64),                                        # cols 1 in store_frames
    "m2e": (W10.with_(mels=2, energy=True), 64),                          # cols 3
    "e_nodc": (W10.with_(energy=True, dc=False), 64),                     # mean = 0
    "e_ns9": (Cfg(8000, 9, 5, snip=False, energy=True), 64),              # energy of reflected frames
    "e_h37": (Cfg(8000, 16, 37, energy=True, htk=True), 64),              # h > W: fs = W, sh = 0
    "e_h37ns": (Cfg(8000, 16, 37, energy=True, snip=False), 64),
    "e_scale": (W10.with_(energy=True, scale=32768.0, efloor=E_SCALE_FLOOR), 64),  # scale2; energies on both sides of the floor
    "e_full": (Cfg(48000, 2048, 2048, pow2=False, energy=True), 4),       # sums of 2048 per work item
    "e_many_first": (Cfg(16000, 64, 16, mels=2048, energy=True), 4),      # mel_off = tile_frames, output tile above the staging
    "e_many_last": (Cfg(16000, 64, 16, mels=2048, energy=True, htk=True), 4),
    "e_asr": (Cfg(16000, 400, 160, mels=80, energy=True), 32),
}
# the LDS rule leaves this one nothing: 16 516 floats at tile_frames 4
NO_LDS = Cfg(16000, 64, 16, mels=2048, ceps=2048)
SMALL = [k for k, (c, _) in CASES.items() if c.W <= 64 and c.mels <= 128]
IMPULSE_CASES = ["w8", "w10", "w3", "w7", "ns10", "ns9", "h37", "h37ns"]


def case_lengths(cfg, tf):
    """T for F = tile_frames - 1, tile_frames, tile_frames + 1 and 1 (without snip_edges and h < W the shortest row, T = W, has
    more than one frame: then that row)"""
    return [length_for(cfg, F) for F in (tf - 1, tf, tf + 1, 1)]


def impulse_batch(name):
    """-> (cfg for impulses, T, positions): every j in the first 3 W and the last 2 W samples at T = length_for(tile_frames + 3)"""
    cfg, tf = CASES[name]
    cfg = impulse_cfg(cfg)
    T = length_for(cfg, tf + 3)
    js = sorted(set(range(0, min(T, 3 * cfg.W))) | set(range(max(0, T - 2 * cfg.W), T)))
    return cfg, T, js


# ---- checks that both suites run: `run(cfg, x)` is a build's pass, x [R, T] float32 -> [R, F, cols] float32 ----------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


ARRANGE_MFCC = Cfg(8000, 50, 20, ceps=13, scale=32768.0)


def check_arrangement(run):
    """Where use_energy and htk_compat put the columns, from a build's own outputs alone (no restatement): one signal through the
    four handles (use_energy, htk_compat) of MFCC (W 50, h 20, F 65, 13 ceps, scale 32768) and of fbank (w10). With A the plain
    MFCC: htk_compat alone gives A's columns 1..12 bit for bit and then sqrt(2) A[..., 0] within both passes' bounds (a missing
    factor is 0.41 |C0|, which the input keeps above 100 bounds in every frame); use_energy alone A's columns 1..12 behind the
    energy column of the fbank pass; both, A's 1..12 and then that energy. fbank: the mel columns and the energy column are the
    same bits wherever they stand. -> the largest error / bound of the sqrt(2) C0 column"""
    base = ARRANGE_MFCC
    x = signal(np.random.default_rng(33), 3, length_for(base, 65))
    A = run(base, x)
    H = run(base.with_(htk=True), x)
    E = run(base.with_(energy=True), x)
    EH = run(base.with_(energy=True, htk=True), x)
    assert A.shape == H.shape == E.shape == EH.shape == (3, 65, 13)
    pre = run(base.prelog(), x)
    lim_a = log_of_prelog(base, pre)[1]
    lim_h = log_of_prelog(base.with_(htk=True), pre)[1]
    lim = lim_a[..., 0] * math.sqrt(2.0) + lim_h[..., 12]
    c0 = A[..., 0].astype(np.float64)
    assert (0.4 * np.abs(c0) > 100.0 * lim).all(), "the input does not separate C0 from sqrt(2) C0"
    assert same_bits(H[..., :12], A[..., 1:])
    err = np.abs(H[..., 12].astype(np.float64) - math.sqrt(2.0) * c0)
    worst = np.unravel_index((err / lim).argmax(), err.shape)
    assert (err <= lim).all(), "htk_compat: the last column is not sqrt(2) C0: off by %g, bound %g" % (err[worst], lim[worst])
    fb_e = Cfg(8000, 50, 20, energy=True, scale=32768.0)
    energy = run(fb_e, x)[..., 0]
    assert same_bits(E[..., 1:], A[..., 1:]) and same_bits(E[..., 0], energy)
    assert same_bits(EH[..., :12], A[..., 1:]) and same_bits(EH[..., 12], energy)
    assert len(np.unique(energy)) > 100 and not same_bits(energy, A[..., 0])
    # fbank over w10
    y = signal(np.random.default_rng(34), 3, length_for(W10, 65))
    P = run(W10, y)
    assert same_bits(run(W10.with_(htk=True), y), P)
    first, last = run(W10.with_(energy=True), y), run(W10.with_(energy=True, htk=True), y)
    assert first.shape == last.shape == (3, 65, 24)
    assert same_bits(first[..., 1:], P) and same_bits(last[..., :23], P) and same_bits(first[..., 0], last[..., 23])
    assert len(np.unique(first[..., 0])) > 50
    return float((err / lim).max())


SPECIAL_CASES = ["w10", "e_first_1", "e_first_0", "ns9", "asr"]
LOG_EPS32 = np.float32(math.log(EPS))


def special_input(name):
    """-> (cfg, T, mr.special_rows at T = length_for(tile_frames + 2))"""
    cfg, tf = CASES[name]
    T = length_for(cfg, tf + 2)
    return cfg, T, mr.special_rows(np.random.default_rng(tf + cfg.W), T)


def check_special_unlogged(cfg, T, x, P):
    """P [6, F, cols] = the unlogged pass over mr.special_rows: rows 0, 1 and 3 finite, zeros give +0.0 in every column, and in
    the rows with one infinity / one NaN exactly the frames that read that sample are non-finite, in every column"""
    assert np.isfinite(P[[0, 1, 3]]).all()
    assert not P[0].view(np.uint32).any(), "zeros do not give +0.0"
    assert not (P[np.isfinite(P)] < 0).any() and not np.isneginf(P).any()
    idx = frame_index(cfg, T)
    for r, at in ((4, T // 3), (5, 2 * T // 3)):
        reads = (idx == at).any(axis=1)
        assert reads.any() and (~reads).any()
        assert np.isfinite(P[r][~reads]).all() and not np.isfinite(P[r][reads]).any(), "row %d" % r
    assert np.isposinf(P).any() and np.isnan(P).any()


def check_special_logged(cfg, got, P, what):
    """got = the logging fbank pass of cfg over the input whose unlogged pass gave P (same build, same columns): +inf where P is,
    a NaN exactly where P is one, and the finite values as kr.check_logged holds them (float32(ln 2^-23) bit for bit where P <=
    2^-23) -> the largest error / bound"""
    assert not cfg.ceps and got.shape == P.shape
    inf, nan = np.isposinf(P), np.isnan(P)
    assert np.isposinf(got[inf]).all(), what + ": the log of +inf"
    assert np.array_equal(np.isnan(got), nan), what + ": the log of a NaN"
    fin = ~(inf | nan)
    want, lim, exact = log_of_prelog(cfg, np.where(fin, P, np.float32(1.0)))
    pinned = want.astype(np.float32)
    assert (got.view(np.uint32) == pinned.view(np.uint32))[exact & fin].all(), what + ": a floored value is not exact"
    mels = np.ones(P.shape, bool)
    if cfg.energy:
        mels[..., cfg.mels if cfg.htk else 0] = False
    low = fin & mels & (P <= np.float32(EPS))
    if cfg.log:
        assert low.any() and (got[low].view(np.uint32) == LOG_EPS32.view(np.uint32)).all(), what + ": at or below 2^-23"
    err = np.abs(got.astype(np.float64) - want)
    free = fin & ~exact
    assert (err[free] <= lim[free]).all(), what + ": a log above its bound"
    return float((err[free] / lim[free]).max())


def check_silence_mfcc(run, name):
    """A row of zeros through an MFCC case: every log-mel is ln(2^-23), so the coefficients are the DCT of a constant (C0 =
    sqrt(M) ln(2^-23), the others 0 but for the table's rounding) within kr.log_of_prelog's bound, and the energy column is the
    floor, bit for bit"""
    cfg, tf = CASES[name]
    x = np.zeros((2, length_for(cfg, tf + 2)), np.float32)
    pre = run(cfg.prelog(), x)
    assert not pre.view(np.uint32).any()
    got = run(cfg, x)
    share = check_logged(cfg, got, pre, name + " silence")
    want = np.einsum("cm,m->c", dct_matrix(cfg), np.full(cfg.mels, math.log(EPS))) * lifter(cfg)
    want = arrange(cfg, np.broadcast_to(want, got.shape), np.zeros(got.shape[:2]))
    lim = log_of_prelog(cfg, pre)[1] + U * np.abs(want) * 2  # the table's own rounding of D and of the lifter
    body = np.ones(got.shape[-1], bool)
    if cfg.energy:
        e_col = cfg.ceps - 1 if cfg.htk else 0
        body[e_col] = False
        floor = np.float32(math.log(cfg.efloor)) if cfg.efloor > 0.0 else LOG_EPS32
        assert (got[..., e_col].view(np.uint32) == floor.view(np.uint32)).all()
    assert (np.abs(got.astype(np.float64) - want)[..., body] <= lim[..., body]).all()
    return share


def check_constant(run, sim_plan_of):
    """A row of constant 0.5 with DC removal, where Kaldi has exact zeros behind the mean's removal and the folded tables leave
    their rounding: unlogged within kr.prelog_bounds at scale 1 and 32768 -> {scale: the largest mel value}"""
    out = {}
    for scale in (1.0, 32768.0):
        cfg = CASES["e_first_1"][0].with_(scale=scale).prelog()
        x = np.full((1, length_for(cfg, 66)), 0.5, np.float32)
        got = run(cfg, x)
        ref, lim = prelog_bounds(cfg, sim_plan_of(cfg), x)
        assert not ref.any(), "the restatement has exact zeros"
        assert_within(got, ref, lim, "constant 0.5 at scale %g" % scale)
        assert not got[..., 0].view(np.uint32).any(), "the energy of a constant is +0.0"
        out[scale] = float(got[..., 1:].max())
    return out
