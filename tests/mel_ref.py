"""The spectrogram pass restated in numpy float64, independently of csrc/alac_mel.h, and the host build of
that header for the tests.

    K = N / 2 + 1;  w = periodic Hann of W samples at offset (N - W) / 2 within N ([1.0] for W = 1, as torch.hann_window)
    C[k][n] = w[n] cos(2 pi ((k n) mod N) / N), S likewise with sin, each rounded to float32 once
    center: F = 1 + (T - (N & 1)) / h (torch.stft pads N / 2 on each side), frame f reads the reflected x at f h - N / 2 + n;
    otherwise F = 1 + (T - N) / h, x at f h + n
    p[f][k] = (sum_n C[k][n] x)^2 + (sum_n S[k][n] x)^2;  mel = fb^T p, fb = torchaudio's melscale_fbanks in double
    log: s log(max(v, floor)), s = 10 for db"""
import ctypes
import math

import numpy as np

from tests import host_build

ROOT = host_build.ROOT

SCALES = {None: 0, "htk": 1, "slaney": 2}
LOGS = {None: 0, "ln": 1, "log10": 2, "db": 3}
U = 2.0 ** -24


class Cfg:
    """One parameter set, with the defaults of the Python entries resolved."""

    def __init__(self, sample_rate, n_fft, hop_length=None, win_length=None, n_mels=None, mel_scale="htk", norm=None, f_min=0.0,
                 f_max=None, center=True, log=None, floor=1e-10):
        self.sample_rate, self.n_fft = sample_rate, n_fft
        self.win_length = n_fft if win_length is None else win_length
        self.hop_length = self.win_length // 2 if hop_length is None else hop_length
        self.n_mels = n_mels
        self.mel_scale = mel_scale if n_mels is not None else None
        self.norm = norm if n_mels is not None else None
        self.f_min = float(f_min)
        self.f_max = float(sample_rate / 2 if f_max is None else f_max)
        self.center, self.log, self.floor = bool(center), log, float(floor)

    @property
    def K(self):
        return self.n_fft // 2 + 1

    @property
    def bins(self):
        return self.n_mels if self.n_mels is not None else self.K

    def with_(self, **kw):
        c = Cfg.__new__(Cfg)
        c.__dict__.update(self.__dict__)
        c.__dict__.update(kw)
        return c

    def words(self):
        """-> (uint32[9], float64[3]) as tests/host_sim/mel_sim.cpp reads them"""
        return (np.array([self.sample_rate, self.n_fft, self.win_length, self.hop_length, self.n_mels or 0, int(self.center),
                          1 if self.norm == "slaney" else 0, SCALES[self.mel_scale], LOGS[self.log]], np.uint32),
                np.array([self.f_min, self.f_max, self.floor], np.float64))

    def kwargs(self):
        """The keyword arguments of pkg.MelSpectrogram"""
        return dict(sample_rate=self.sample_rate, n_fft=self.n_fft, win_length=self.win_length, hop_length=self.hop_length,
                    f_min=self.f_min, f_max=self.f_max, n_mels=self.n_mels, center=self.center, norm=self.norm,
                    mel_scale=self.mel_scale or "htk", log=self.log, floor=self.floor)


# ---- the definition ----------------------------------------------------------------------------------------------------
def window(N, W):
    w = np.zeros(N)
    off = (N - W) // 2
    w[off:off + W] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W) if W > 1 else 1.0  # torch.hann_window(1) is [1.0]
    return w


def basis(N, W):
    """-> float64 [2][K][N]: C and S in double, not yet rounded"""
    K = N // 2 + 1
    r = (np.arange(K, dtype=np.int64)[:, None] * np.arange(N, dtype=np.int64)[None, :]) % N
    ang = 2.0 * np.pi * r / N
    w = window(N, W)
    return np.stack([w[None, :] * np.cos(ang), w[None, :] * np.sin(ang)])


def basis32(N, W):
    return basis(N, W).astype(np.float32)


def out_frames(cfg, T):
    if cfg.center:
        return 1 + (T - cfg.n_fft % 2) // cfg.hop_length if T > cfg.n_fft // 2 else 0
    return 1 + (T - cfg.n_fft) // cfg.hop_length if T >= cfg.n_fft else 0


def frames_of(cfg, x):
    """x [R, T] -> the frames [R, F, N] float64, the reflection resolved: every index lies in [0, T) after it"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    T = x.shape[1]
    F = out_frames(cfg, T)
    idx = np.arange(F)[:, None] * cfg.hop_length + np.arange(cfg.n_fft)[None, :]
    if cfg.center:
        idx = idx - cfg.n_fft // 2
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= T, 2 * (T - 1) - idx, idx)
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < T), "a frame reaches outside the row"
    return x[:, idx]


def power64(cfg, x, tables=None):
    """The power spectrogram in float64 [R, K, F] over the float32-rounded basis (tables: a plan's own [2][K][N])."""
    B = np.asarray(basis32(cfg.n_fft, cfg.win_length) if tables is None else tables, np.float64)
    fr = frames_of(cfg, x)
    re = np.einsum("kn,rfn->rkf", B[0], fr)
    im = np.einsum("kn,rfn->rkf", B[1], fr)
    return re * re + im * im


def hz_to_mel(f, scale):
    if scale == "htk":
        return 2595.0 * math.log10(1.0 + f / 700.0)
    if f >= 1000.0:
        return 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)
    return f / (200.0 / 3.0)


def mel_to_hz(m, scale):
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    if m >= 15.0:
        return 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))
    return (200.0 / 3.0) * m


def fbanks(cfg):
    """torchaudio.functional.melscale_fbanks(K, f_min, f_max, n_mels, sample_rate, norm, mel_scale) in float64 -> [K, n_mels];
    the two outer points are f_min and f_max themselves."""
    K, M = cfg.K, cfg.n_mels
    all_freqs = np.linspace(0, cfg.sample_rate // 2, K)
    m_min, m_max = hz_to_mel(cfg.f_min, cfg.mel_scale), hz_to_mel(cfg.f_max, cfg.mel_scale)
    step = (m_max - m_min) / (M + 1)
    pts = np.array([mel_to_hz(m_min + i * step, cfg.mel_scale) for i in range(M + 2)])
    pts[0], pts[-1] = cfg.f_min, cfg.f_max
    f_diff = pts[1:] - pts[:-1]
    slopes = pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    if cfg.norm == "slaney":
        fb = fb * (2.0 / (pts[2:M + 2] - pts[:M]))[None, :]
    return fb


def windows_of(fb32):
    """first[m] and taps of a float32 filterbank [K, M] as the plan keeps them, and the windows fbw [M, taps]"""
    K, M = fb32.shape
    first, run = np.zeros(M, np.int32), np.zeros(M, np.int64)
    for m in range(M):
        nz = np.nonzero(fb32[:, m])[0]
        if len(nz):
            assert nz[-1] - nz[0] + 1 == len(nz), "filter %d is not one run" % m
            first[m], run[m] = nz[0], len(nz)
    taps = max(1, int(run.max()))
    first = np.minimum(first, K - taps).astype(np.int32)
    fbw = np.stack([fb32[first[m]:first[m] + taps, m] for m in range(M)])
    return first, taps, fbw


def dense_fb(plan, K):
    """A plan's windows as the dense [K, n_mels] float32 matrix"""
    fb = np.zeros((K, plan["n_mels"]), np.float32)
    for m in range(plan["n_mels"]):
        fb[plan["first"][m]:plan["first"][m] + plan["taps"], m] = plan["fb"][m]
    return fb


def mel64(cfg, x, tables=None, fb=None):
    """[R, n_mels, F] float64: fb^T over power64 (fb: a plan's dense float32 filterbank in place of the rounded restatement)."""
    fb = np.asarray(fbanks(cfg).astype(np.float32) if fb is None else fb, np.float64)
    return np.einsum("km,rkf->rmf", fb, power64(cfg, x, tables))


def log64(cfg, v):
    if cfg.log is None:
        return v
    fl = float(np.float32(cfg.floor))
    v = np.maximum(np.asarray(v, np.float64), fl)
    return np.log(v) if cfg.log == "ln" else (10.0 if cfg.log == "db" else 1.0) * np.log10(v)


def bounds(cfg, x, tables, fb=None, taps=0):
    """The derived ceilings of the float32 chains against the restatement on the same tables, u = 2^-24:
        e_r = N u sum |C x|, e_i likewise;  dp = (2 |re| e_r + 2 |im| e_i + e_r^2 + e_i^2)(1 + 2 u) + 2 u p
        dmel = sum fb dp + taps u sum fb (p + dp)
    -> (dp [R, K, F], dmel [R, M, F] or None)"""
    B = np.asarray(tables, np.float64)
    fr = frames_of(cfg, x)
    N = cfg.n_fft
    re = np.einsum("kn,rfn->rkf", B[0], fr)
    im = np.einsum("kn,rfn->rkf", B[1], fr)
    er = N * U * np.einsum("kn,rfn->rkf", np.abs(B[0]), np.abs(fr))
    ei = N * U * np.einsum("kn,rfn->rkf", np.abs(B[1]), np.abs(fr))
    p = re * re + im * im
    dp = (2 * np.abs(re) * er + 2 * np.abs(im) * ei + er * er + ei * ei) * (1 + 2 * U) + 2 * U * p
    if fb is None:
        return dp, None
    fb = np.asarray(fb, np.float64)
    dmel = np.einsum("km,rkf->rmf", fb, dp) + taps * U * np.einsum("km,rkf->rmf", fb, p + dp)
    return dp, dmel


def ulps32(got32, want64):
    """|got - want| in units of the float32 spacing at want (float64), elementwise"""
    want64 = np.asarray(want64, np.float64)
    w32 = np.abs(want64.astype(np.float32))
    spacing = np.spacing(np.maximum(w32, np.float32(2.0 ** -126))).astype(np.float64)
    return np.abs(np.asarray(got32, np.float64) - want64) / spacing


def whisper_post(logmel):
    """Whisper's post-processing of a log10 mel tensor [..., n_mels, F] in numpy float32: drop the last frame, clamp below
    (the row's maximum over [n_mels, frames]) - 8, then (x + 4) / 4."""
    x = np.asarray(logmel, np.float32)[..., :-1]
    top = x.max(axis=(-2, -1), keepdims=True)
    x = np.maximum(x, top - np.float32(8.0))
    return (x + np.float32(4.0)) / np.float32(4.0)


# ---- the host build ---------------------------------------------------------------------------------------------------
def build_mel_sim():
    L = host_build.shared("mel_sim.cpp", "libmel_sim.so", host_build.SIM_FP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.mel_sim_plan.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, u64]
    L.mel_sim_run.argtypes = [vp, vp, vp, u64, u64, u64, vp, u64, u64, ctypes.c_int]
    L.mel_sim_out_frames.restype, L.mel_sim_out_frames.argtypes = u64, [vp, vp, u64]
    L.mel_sim_lds_floats.restype = ctypes.c_uint32
    return L


def build_mel_shim(pkg):
    """tests/host_sim/mel_shim.cpp over host/mel_spectrogram.hpp, linked with the library"""
    L = host_build.shared("mel_shim.cpp", "libmel_shim.so", host_build.SHIM, host_build.library(pkg))
    vp, u32, sz, dbl, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_double, ctypes.c_int
    L.mel_shim_run.restype = ctypes.c_long
    L.mel_shim_run.argtypes = [u32, u32, u32, u32, dbl, dbl, u32, i, i, i, i, dbl, vp, sz, sz, sz, vp, sz, sz, vp, vp, vp, sz, vp, sz,
                               vp, sz, vp]
    L.mel_shim_last_error.restype = ctypes.c_char_p
    return L


INFO = ("n_fft", "win_length", "hop_length", "n_freqs", "n_mels", "taps", "bins", "tile_frames", "lds_bytes")


def sim_plan(S, cfg):
    """-> dict of the host build's plan (INFO, basis [2][K][N], fb [n_mels][taps], first [n_mels]), or None where it has none"""
    w, d = cfg.words()
    info = np.zeros(9, np.uint32)
    if S.mel_sim_plan(w.ctypes.data, d.ctypes.data, info.ctypes.data, None, 0, None, 0, None, 0) != 0:
        return None
    out = {k: int(v) for k, v in zip(INFO, info)}
    b = np.zeros((2, out["n_freqs"], out["n_fft"]), np.float32)
    fb = np.zeros((out["n_mels"], out["taps"]), np.float32)
    first = np.zeros(out["n_mels"], np.int32)
    assert S.mel_sim_plan(w.ctypes.data, d.ctypes.data, info.ctypes.data, b.ctypes.data, b.size, fb.ctypes.data, fb.size,
                          first.ctypes.data, first.size) == 0
    out.update(basis=b, fb=fb, first=first)
    return out


def sim_out_frames(S, cfg, T):
    w, d = cfg.words()
    return S.mel_sim_out_frames(w.ctypes.data, d.ctypes.data, T)


# ---- buffers, shared by the CPU and the GPU suite ---------------------------------------------------------------------
SENTINEL = 0xC3C3A5A5  # as a float about -391.3: no power and no mel value (those are >= 0 or NaN)


def aligned(elems, fill=None):
    """A uint32 array of `elems` elements on a 16-byte boundary."""
    own = np.zeros(elems + 8, np.uint32)
    off = (-own.ctypes.data // 4) % 4
    a = own[off:off + elems]
    assert a.ctypes.data % 16 == 0
    if fill is not None:
        a[:] = fill
    return a


def layout(rows, T, bins, F, in_off, out_off, bin_pad=0):
    """Odd strides and guard elements: -> (in_stride, in_lead, in_elems, row_stride, bin_stride, out_lead, out_elems); the
    tensors start in_lead / out_lead elements into 16-byte-aligned buffers, in_off / out_off elements behind a boundary."""
    in_stride = T + 1 + T % 2
    bin_stride = F + bin_pad
    row_stride = (bins - 1) * bin_stride + F + 1 + (bins * F) % 2
    in_lead, out_lead = 4 + in_off, 8 + out_off
    return in_stride, in_lead, in_lead + (rows - 1) * in_stride + T, row_stride, bin_stride, out_lead, out_lead + rows * row_stride + 8


def expected_image(y32, elems, out_lead, row_stride, bin_stride):
    """The whole output buffer as uint32: y32 [rows, bins, F] at its places, the sentinel everywhere else."""
    want = np.full(elems, SENTINEL, np.uint32)
    R, B, F = y32.shape
    for r in range(R):
        for b in range(B):
            at = out_lead + r * row_stride + b * bin_stride
            want[at:at + F] = y32[r, b].view(np.uint32)
    return want


def rows_of(img, rows, bins, F, out_lead, row_stride, bin_stride):
    """[rows, bins, F] float32 out of a buffer image"""
    return np.stack([np.stack([img[out_lead + r * row_stride + b * bin_stride:][:F] for b in range(bins)])
                     for r in range(rows)]).view(np.float32)


def sim_image(S, cfg, x, in_off=0, out_off=0, bin_pad=0, guard=0):
    """The rows x laid out with an odd stride in_off elements behind a 16-byte boundary, NaN between them, the pass of the host
    build into a sentinel-filled buffer -> (image uint32, layout)"""
    rows, T = x.shape
    F = out_frames(cfg, T)
    lay = layout(rows, T, cfg.bins, F, in_off, out_off, bin_pad)
    in_stride, in_lead, in_elems, row_stride, bin_stride, out_lead, out_elems = lay
    src = aligned(in_elems, 0x7FC00000)
    for r in range(rows):
        src[in_lead + r * in_stride: in_lead + r * in_stride + T] = x[r].view(np.uint32)
    img = aligned(out_elems, SENTINEL)
    w, d = cfg.words()
    rc = S.mel_sim_run(w.ctypes.data, d.ctypes.data, src.ctypes.data + 4 * in_lead, in_stride, rows, T, img.ctypes.data + 4 * out_lead,
                       row_stride, bin_stride, guard)
    assert rc == 0, rc
    return img.copy(), lay


def signal(rng, rows, T):
    """[rows, T] float32 in [-1, 1]: int16 values scaled by 2^-15, noise shaped over five decades, the last row alternating +-1"""
    x = np.zeros((rows, T), np.float32)
    for r in range(rows):
        if r % 2 == 0:
            x[r] = rng.integers(-32768, 32768, T).astype(np.float32) * np.float32(2.0 ** -15)
        else:
            x[r] = (rng.uniform(-1, 1, T) * np.exp(rng.uniform(-12.0, 0.0, T))).astype(np.float32)
    if rows > 1:
        x[rows - 1] = np.where(np.arange(T) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return x


def special_rows(rng, T):
    """[6, T] float32 outside the audio range: 0 zeros; 1 float32 denormals; 2 values up to 1e30 of alternating sign in blocks
    (their powers overflow to inf); 3 a signal with -0.0 scattered in it; 4 the signal with one +inf; 5 the signal with one NaN"""
    x = np.zeros((6, T), np.float32)
    tiny = rng.integers(1, 1 << 23, T).astype(np.uint32) | (rng.integers(0, 2, T).astype(np.uint32) << 31)  # exponent field 0
    x[1] = tiny.view(np.float32)
    x[2] = (rng.uniform(0.01, 1, T) * np.where((np.arange(T) // 37) % 2 == 0, 1.0, -1.0)).astype(np.float32) * np.float32(1e30)
    sig = rng.uniform(-1, 1, T).astype(np.float32)
    x[3] = np.where(rng.random(T) < 0.3, np.float32(-0.0), sig)
    x[4] = sig
    x[4, T // 3] = np.inf
    x[5] = sig
    x[5, 2 * T // 3] = np.nan
    return x


def impulse_expected(cfg, basis32_, T, j, amp=1.0):
    """The power spectrogram [K, F] float32 of a row of +0.0 with amp at index j, bit for bit, from the table alone: every
    fmaf with a zero sample leaves its accumulator as it is, so re and im of a frame are the entries under j times amp (amp a
    power of two: exact), or, where the reflected margins show j more than once, their float32 sum taken in the order of n, one
    rounding per fmaf; p = fmaf(im, im, float32(re * re)), evaluated in float64, which holds im * im exactly.
    -> (want, the number of frames that see j more than once)"""
    B = np.asarray(basis32_, np.float64)
    N, h, F = cfg.n_fft, cfg.hop_length, out_frames(cfg, T)
    want = np.zeros((cfg.K, F), np.float32)
    twice = 0
    for f in range(F):
        idx = f * h + np.arange(N) - (N // 2 if cfg.center else 0)
        if cfg.center:
            idx = np.where(idx < 0, -idx, idx)
            idx = np.where(idx >= T, 2 * (T - 1) - idx, idx)
        assert idx.min() >= 0 and idx.max() < T
        ns = np.nonzero(idx == j)[0]
        if not len(ns):
            continue
        twice += len(ns) >= 2
        re, im = np.zeros(cfg.K), np.zeros(cfg.K)
        for n in ns:  # the sum of two float32 is exact in float64, so each step rounds once, as the fmaf does
            re = (re + B[0][:, n] * amp).astype(np.float32).astype(np.float64)
            im = (im + B[1][:, n] * amp).astype(np.float32).astype(np.float64)
        want[:, f] = (im * im + (re * re).astype(np.float32).astype(np.float64)).astype(np.float32)
    return want, twice


def length_for(cfg, F):
    """The shortest T with out_frames(T) == F"""
    if cfg.center:
        return max((F - 1) * cfg.hop_length + cfg.n_fft % 2, cfg.n_fft // 2 + 1)
    return cfg.n_fft + (F - 1) * cfg.hop_length


# ---- the parameter cases, shared by the CPU and the GPU suite ---------------------------------------------------------
CASES = {
    "tiny": Cfg(16000, 16, 4, 12, n_mels=5, mel_scale="htk"),
    "whisper80": Cfg(16000, 400, 160, 400, n_mels=80, mel_scale="slaney", norm="slaney"),
    "htk128": Cfg(16000, 400, 160, 400, n_mels=128, mel_scale="htk"),  # four filters without a weight
    "n1024": Cfg(44100, 1024, 256, 1024, n_mels=128, mel_scale="htk"),
    "uncentred": Cfg(16000, 64, 24, 48, n_mels=10, mel_scale="slaney", center=False),
}
OFFSETS = [(0, 0), (1, 3), (2, 1), (3, 2)]  # (out_off, in_off): every misalignment of either side once

# Parameter sets at the edges of csrc/alac_mel.h, each with the tile_frames its plan has (asserted where a case is used) and
# the path it reaches: N < 4 skips the prefetch block of dft_blocks, N % 4 != 0 runs its tail, even K makes KP = K + 1 and the
# last bin pair whole, hop > N takes the other branch of stage_tile and make_tile, tile_frames 4 runs dft_blocks<4>.
SLANEY = dict(mel_scale="slaney", norm="slaney")
EDGE_CASES = {
    "n2": (Cfg(8000, 2, 1, 2), 64),                                                  # N < 4, K = 2
    "n3": (Cfg(8000, 3, 1, 3, n_mels=2), 64),                                        # odd N < 4
    "n6u": (Cfg(8000, 6, 2, 6, n_mels=2, center=False), 64),                         # even K, a tail of 2
    "n7": (Cfg(8000, 7, 3, 7, n_mels=3), 64),                                        # one block of 4, a tail of 3
    "n10": (Cfg(8000, 10, 3, 10, n_mels=4, mel_scale="slaney"), 64),                 # loop once + block + tail, even K
    "n15": (Cfg(8000, 15, 4, 9), 64),                                                # odd N, a short window at an odd offset
    "w1": (Cfg(8000, 8, 3, 1), 64),                                                  # win_length 1
    "hop37": (Cfg(8000, 16, 37, 16, n_mels=3), 64),                                  # hop > N staging
    "hop37u": (Cfg(8000, 16, 37, 16, n_mels=3, center=False), 64),
    "onemel": (Cfg(16000, 64, 16, 64, n_mels=1), 64),                                # taps 31: the 8-wide loop and its tail
    "band": (Cfg(16000, 128, 32, 128, n_mels=12, f_min=300.0, f_max=3400.0, **SLANEY), 64),  # windows off both ends
    "overtop": (Cfg(16000, 64, 16, 64, n_mels=6, f_max=12000.0), 64),  # f_max above sample_rate / 2: the last filter is cut off
                                                                       # at the last bin, a short run whose window is clamped
    "manymels": (Cfg(16000, 16, 4, 16, n_mels=2048), 4),      # dft_blocks<4>, cheap; the output tile far above the staging
    "n512h512": (Cfg(16000, 512, 512, n_mels=40), 16),                               # hop = N
    "n2048h512": (Cfg(48000, 2048, 512, n_mels=64), 8),                              # tile_frames 8, 55 KB of LDS
    "n2046u": (Cfg(48000, 2046, 700, 2000, n_mels=32, center=False, **SLANEY), 8),   # even K at size, 60 608 bytes of LDS
    "n2048h2048": (Cfg(48000, 2048, 2048), 4),                                       # <4> at size, power only
    "n2048h5000": (Cfg(48000, 2048, 5000), 4),                                       # <4> with hop > N
    "n2047": (Cfg(48000, 2047, 1024, n_mels=16), 4),                                 # odd N at size, taps 360
}
SMALL_EDGES = [k for k, (c, _) in EDGE_CASES.items() if c.n_fft <= 128]
LARGE_EDGES = [k for k, (c, _) in EDGE_CASES.items() if c.n_fft > 128]


def edge_lengths(cfg, tf):
    """T for F = tile_frames + 1, the shortest row, and F = tile_frames (n_fft above 128: the first two only)"""
    Ts = [length_for(cfg, tf + 1), cfg.n_fft // 2 + 1 if cfg.center else cfg.n_fft, length_for(cfg, tf)]
    return Ts if cfg.n_fft <= 128 else Ts[:2]


def values_of(img, lay, cfg, rows, T, what=""):
    """[rows, bins, F] float32 out of an image, and a check that everything outside it is the sentinel"""
    got = rows_of(img, rows, cfg.bins, out_frames(cfg, T), lay[5], lay[3], lay[4])
    assert np.array_equal(img, expected_image(got, img.size, lay[5], lay[3], lay[4])), what + ": outside the output"
    return got


def ceiling_share(cfg, plan, x, got, what=""):
    """got [rows, bins, F] against the float64 restatement on the plan's tables: asserts the ceilings of bounds(), -> the largest
    error / ceiling"""
    if cfg.n_mels is None:
        ref = power64(cfg, x, plan["basis"])
        lim, _ = bounds(cfg, x, plan["basis"])
    else:
        dense = dense_fb(plan, cfg.K)
        ref = mel64(cfg, x, plan["basis"], dense)
        _, lim = bounds(cfg, x, plan["basis"], dense, plan["taps"])
    err = np.abs(got.astype(np.float64) - ref)
    ok = err <= lim
    assert ok.all(), "%s: error %g above the ceiling %g" % (what, err[~ok][0], lim[~ok][0])
    return float((err / np.maximum(lim, 1e-300)).max())


def impulse_rows(T, js):
    """[len(js), T] float32 of +0.0, row r with 1.0 at js[r]"""
    x = np.zeros((len(js), T), np.float32)
    x[np.arange(len(js)), js] = 1.0
    return x


def power_only(cfg):
    return cfg.with_(n_mels=None, mel_scale=None, norm=None)


IMPULSE_CASES = ["n2", "n3", "n6u", "n7", "n10", "n15", "tiny", "hop37", "hop37u", "n2048h2048", "n2048h512"]
EDGE_N = list(range(0, 9)) + list(range(1019, 1029)) + list(range(2039, 2048))  # a frame's n at the window's edges and its middle


def impulse_batch(name):
    """-> (cfg without a mel stage, tile_frames, T, the impulses' positions): every j in [0, 3 n_fft) and [T - 2 n_fft, T) at T =
    length_for(tile_frames + 3); for the cases of n_fft 2048 the positions frame 5 reads at the n of EDGE_N."""
    cfg, tf = EDGE_CASES[name] if name in EDGE_CASES else (CASES[name], 64)
    cfg = power_only(cfg)
    T = length_for(cfg, tf + 3)
    N = cfg.n_fft
    if N == 2048:
        js = [5 * cfg.hop_length - N // 2 + n for n in EDGE_N]
    else:
        js = sorted(set(range(0, 3 * N)) | set(range(T - 2 * N, T)))
    assert 0 <= min(js) and max(js) < T
    return cfg, tf, T, js


def impulse_image(cfg, basis, T, js):
    """[len(js), K, F] float32 of impulse_expected per row, the rows that see their impulse twice, the rows without a power"""
    want, twice = zip(*(impulse_expected(cfg, basis, T, j) for j in js))
    want = np.stack(want)
    return want, sum(t > 0 for t in twice), sum(not w.any() for w in want)
