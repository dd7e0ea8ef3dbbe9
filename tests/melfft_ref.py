"""The spectrogram pass with transform="fft" restated in numpy float64, independently of csrc/alac_melfft.h,
its derived ceilings, the host build of that header, and the cases both suites run.

    v = frames_of(cfg, x) * w32 (the window of the handle's fft_plan);  X = np.fft.rfft(v);  p = |X|^2
    mel = fb^T p (mel_ref.fbanks rounded to float32, or the plan's own windows);  log: mel_ref.log64

The ceiling, u = 2^-24: a pass of radix r adds at most g(r) u sqrt(r) ||z|| to the error of a frame's vector, the later passes
carry it on with their norms, so behind the last pass ||dZ|| <= u sum g(r) sqrt(M) ||v||; the split step takes two entries of Z
with weights of modulus at most 1 each and adds its own roundings (4 u (|A| + |B|), |A| + |B| <= sqrt(N) ||v||), the window product
1 u ||v|| carried through |X[k]| <= sqrt(N) ||v||:
    eta = u (sum over the passes of g(r) + 4 + 1),  g = {2: 5, 3: 10, 4: 6, 5: 15}
    |dX[k]| <= e = eta sqrt(N) ||v||_2
    dp = (2 |X| e + e^2)(1 + 2 u) + 2 u p;   dmel = sum fb dp + taps u sum fb (p + dp)"""
import ctypes

import numpy as np

from tests import host_build
from tests import mel_ref
from tests.mel_ref import Cfg, U

ROOT = mel_ref.ROOT

G = {2: 5.0, 3: 10.0, 4: 6.0, 5: 15.0}
SPLIT_SHARE, WINDOW_SHARE = 4.0, 1.0
ROOTS = 8  # floats in front of the passes' twiddles


# ---- the definition ----------------------------------------------------------------------------------------------------
def size_ok(N):
    if N < 2 or N % 2 or N > 2048:
        return False
    m = N // 2
    for r in (2, 3, 5):
        while m % r == 0:
            m //= r
    return m == 1


def window64(N, W):
    return mel_ref.window(N, W)


def twiddle64(N, radices):
    """The twiddle table in float64 as include/alacgpu.h lays it out: roots, per pass [L][r - 1] pairs, then N / 2 + 1 pairs"""
    out = [-0.5, np.sin(2 * np.pi / 3), np.cos(2 * np.pi / 5), np.sin(2 * np.pi / 5), np.cos(4 * np.pi / 5), np.sin(4 * np.pi / 5), 0.0, 0.0]
    L = 1
    for r in radices:
        n = L * r
        for k in range(L):
            for q in range(1, r):
                ang = 2.0 * np.pi * ((q * k) % n) / n
                out += [np.cos(ang), -np.sin(ang)]
        L = n
    for k in range(N // 2 + 1):
        ang = 2.0 * np.pi * k / N
        out += [np.cos(ang), -np.sin(ang)]
    return np.array(out, np.float64)


def spectrum64(cfg, x, w32):
    """-> (X [R, F, K] complex128, ||v||_2 [R, F]) of the frames times the float32 window, in float64"""
    v = mel_ref.frames_of(cfg, x) * np.asarray(w32, np.float64)
    return np.fft.rfft(v, axis=-1), np.sqrt((v * v).sum(axis=-1))


def eta(radices):
    return U * (sum(G[r] for r in radices) + SPLIT_SHARE + WINDOW_SHARE)


def reference(cfg, x, plan):
    """-> (ref [R, bins, F] float64 before the log, ceiling of the same shape) for a plan dict (radix, window, fb, first, taps)"""
    X, norm = spectrum64(cfg, x, plan["window"])
    p = (X.real ** 2 + X.imag ** 2).transpose(0, 2, 1)  # [R, K, F]
    e = (eta(plan["radix"]) * np.sqrt(cfg.n_fft) * norm)[:, None, :]
    dp = (2 * np.abs(X).transpose(0, 2, 1) * e + e * e) * (1 + 2 * U) + 2 * U * p
    if cfg.n_mels is None:
        return p, dp
    fb = np.asarray(mel_ref.dense_fb(plan, cfg.K), np.float64)
    mel = np.einsum("km,rkf->rmf", fb, p)
    dmel = np.einsum("km,rkf->rmf", fb, dp) + plan["taps"] * U * np.einsum("km,rkf->rmf", fb, p + dp)
    return mel, dmel


def share(cfg, plan, x, got, what=""):
    """got [R, bins, F] (before the log) against reference(): asserts the ceiling, -> the largest error / ceiling"""
    ref, lim = reference(cfg, x, plan)
    err = np.abs(got.astype(np.float64) - ref)
    ok = err <= lim
    assert ok.all(), "%s: error %g above the ceiling %g (%d of %d)" % (what, err[~ok][0], lim[~ok][0], (~ok).sum(), ok.size)
    return float((err / np.maximum(lim, 1e-300)).max())


# ---- the host build ---------------------------------------------------------------------------------------------------
def build_melfft_sim():
    L = host_build.shared("melfft_sim.cpp", "libmelfft_sim.so", host_build.SIM_FP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.melfft_sim_plan.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64]
    L.melfft_sim_run.argtypes = [vp, vp, vp, u64, u64, u64, vp, u64, u64, ctypes.c_int]
    return L


def build_melfft_shim(pkg):
    """tests/host_sim/melfft_shim.cpp over host/mel_spectrogram.hpp, linked with the library"""
    L = host_build.shared("melfft_shim.cpp", "libmelfft_shim.so", host_build.SHIM, host_build.library(pkg))
    vp, u32, sz, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int
    L.melfft_shim_run.restype = ctypes.c_long
    L.melfft_shim_run.argtypes = [u32, u32, u32, u32, u32, i, u32, vp, sz, sz, sz, vp, sz, sz, vp, vp, sz, vp, sz]
    L.melfft_shim_last_error.restype = ctypes.c_char_p
    return L


FFT_INFO = ("transform", "tile_frames", "lds_bytes", "batch_frames", "pitch", "n_passes")


def sim_plan(S, cfg):
    """-> dict of the host build's FFT plan (FFT_INFO, radix, window [N], twiddle, n_mels, taps, fb, first), or None where it
    has none"""
    w, d = cfg.words()
    info = np.zeros(18, np.uint32)
    if S.melfft_sim_plan(w.ctypes.data, d.ctypes.data, info.ctypes.data, None, 0, None, 0, None, 0, None, 0) != 0:
        return None
    out = {k: int(v) for k, v in zip(FFT_INFO, info)}
    out["radix"] = [int(r) for r in info[6:6 + out["n_passes"]]]
    out["n_mels"], out["taps"] = int(info[16]), int(info[17])
    win = np.zeros(int(info[14]), np.float32)
    tw = np.zeros(int(info[15]), np.float32)
    fb = np.zeros((out["n_mels"], out["taps"]), np.float32)
    first = np.zeros(out["n_mels"], np.int32)
    assert S.melfft_sim_plan(w.ctypes.data, d.ctypes.data, info.ctypes.data, win.ctypes.data, win.size, tw.ctypes.data, tw.size,
                             fb.ctypes.data, fb.size, first.ctypes.data, first.size) == 0
    out.update(window=win, twiddle=tw, fb=fb, first=first)
    return out


def sim_image(S, cfg, x, in_off=0, out_off=0, bin_pad=0, guard=0):
    """mel_ref.sim_image's pattern over the FFT build: the rows x laid out with an odd stride in_off elements behind a 16-byte
    boundary, NaN between them, one pass into a sentinel-filled buffer -> (image uint32, layout)"""
    rows, T = x.shape
    F = mel_ref.out_frames(cfg, T)
    lay = mel_ref.layout(rows, T, cfg.bins, F, in_off, out_off, bin_pad)
    in_stride, in_lead, in_elems, row_stride, bin_stride, out_lead, out_elems = lay
    src = mel_ref.aligned(in_elems, 0x7FC00000)
    for r in range(rows):
        src[in_lead + r * in_stride: in_lead + r * in_stride + T] = x[r].view(np.uint32)
    img = mel_ref.aligned(out_elems, mel_ref.SENTINEL)
    w, d = cfg.words()
    rc = S.melfft_sim_run(w.ctypes.data, d.ctypes.data, src.ctypes.data + 4 * in_lead, in_stride, rows, T,
                          img.ctypes.data + 4 * out_lead, row_stride, bin_stride, guard)
    assert rc == 0, rc
    return img.copy(), lay


# ---- the cases, shared by the CPU and the GPU suite: name -> (Cfg, tile_frames of its FFT plan, batch_frames, radices) -------
SL = dict(mel_scale="slaney", norm="slaney")


def _both(name, tf, batch, radix, *a, **kw):
    """a case centred and, with the suffix u, not"""
    return {name: (Cfg(*a, **kw), tf, batch, radix), name + "u": (Cfg(*a, center=False, **kw), tf, batch, radix)}


FFT_CASES = {}
for _c in (
        _both("n2", 64, 64, [], 8000, 2, 1, 2),                                    # M = 1: no pass
        _both("n4", 64, 64, [2], 8000, 4, 1, 4),                                   # each radix alone
        _both("n6", 64, 64, [3], 8000, 6, 2, 6, n_mels=2),
        _both("n8", 64, 64, [4], 8000, 8, 3, 8, n_mels=3),
        _both("n10", 64, 64, [5], 8000, 10, 3, 10, n_mels=4, mel_scale="slaney"),
        _both("n10w7", 64, 64, [5], 8000, 10, 3, 7),                               # a short window at an odd offset
        _both("w1", 64, 64, [4], 8000, 8, 3, 1),                                   # win_length 1
        _both("n12", 64, 64, [3, 2], 8000, 12, 5, 12, n_mels=3),                   # every two distinct radices
        _both("n20", 64, 64, [5, 2], 8000, 20, 7, 16, n_mels=4),
        _both("n24", 64, 64, [3, 4], 8000, 24, 8, 24, n_mels=5),
        _both("n30", 64, 64, [5, 3], 8000, 30, 11, 30, n_mels=5),
        _both("n40", 64, 64, [5, 4], 8000, 40, 13, 40, n_mels=6),
        _both("n16", 64, 64, [4, 2], 8000, 16, 4, 12, n_mels=5),
        _both("n32", 64, 64, [4, 4], 8000, 32, 8, 32, n_mels=6),                   # a repeated radix
        _both("n100", 64, 64, [5, 5, 2], 16000, 100, 40, 100, n_mels=10),
        _both("n36", 64, 64, [3, 3, 2], 8000, 36, 9, 36, n_mels=6),
        _both("hop37", 64, 64, [4, 2], 8000, 16, 37, 16, n_mels=3),                # hop > N staging
        _both("onemel", 64, 64, [4, 4, 2], 16000, 64, 16, 64, n_mels=1),
        _both("whisper", 16, 16, [5, 5, 4, 2], 16000, 400, 160, 400, n_mels=80, f_max=8000.0, **SL),
        _both("n512h512", 8, 8, [4, 4, 4, 4], 16000, 512, 512, 512, n_mels=40),
        _both("n1024", 8, 8, [4, 4, 4, 4, 2], 44100, 1024, 256, 1024, n_mels=128),
        _both("n1536", 4, 4, [3, 4, 4, 4, 4], 48000, 1536, 384, 1536, n_mels=64),  # a 3 at size
        {"n2000u": (Cfg(48000, 2000, 700, 1900, n_mels=32, center=False, **SL), 4, 2, [5, 5, 5, 4, 2])},
        _both("n2048h512", 4, 4, [4, 4, 4, 4, 4], 48000, 2048, 512, 2048, n_mels=64),
        _both("n2048h2048", 4, 1, [4, 4, 4, 4, 4], 48000, 2048, 2048, 2048),       # the transform buffer holds one frame
        _both("n2048h5000", 4, 1, [4, 4, 4, 4, 4], 48000, 2048, 5000, 2048)):
    FFT_CASES.update(_c)
SMALL = [k for k, c in FFT_CASES.items() if c[0].n_fft <= 128]
LARGE = [k for k, c in FFT_CASES.items() if c[0].n_fft > 128]


def lengths(cfg, tf):
    """T for F = tile_frames - 1, tile_frames, tile_frames + 1, 1 and the shortest row (the last two may coincide)"""
    Ts = [mel_ref.length_for(cfg, tf - 1), mel_ref.length_for(cfg, tf), mel_ref.length_for(cfg, tf + 1), mel_ref.length_for(cfg, 1),
          cfg.n_fft // 2 + 1 if cfg.center else cfg.n_fft]
    return sorted(set(Ts), reverse=True)


def offsets(cfg):
    return mel_ref.OFFSETS if cfg.n_fft <= 128 else [mel_ref.OFFSETS[1], mel_ref.OFFSETS[3]]


def runs_of(name):
    """The passes of a case: (rows, T, (out_off, in_off)) — rows 1 and 3 in turn, every length, the offsets dealt over them so that
    each occurs"""
    cfg, tf = FFT_CASES[name][:2]
    offs = offsets(cfg)
    out = []
    for i, T in enumerate(lengths(cfg, tf)):
        for j, off in enumerate(offs if cfg.n_fft <= 128 else [offs[i % len(offs)]]):
            out.append((1 if (i + j) % 2 else 3, T, off))
    return out


def impulse_batch(name):
    """-> (cfg without a mel stage, T, the impulses' positions): every j of the first 3 N and last 2 N samples at T =
    length_for(tile_frames + 3) for N <= 32; for N = 2048 the positions frame 5 of tile_frames + 8 reads at the n of mel_ref.EDGE_N"""
    cfg, tf = FFT_CASES[name][:2]
    cfg = mel_ref.power_only(cfg)
    N = cfg.n_fft
    T = mel_ref.length_for(cfg, tf + (8 if N == 2048 else 3))
    if N == 2048:
        js = [5 * cfg.hop_length - (N // 2 if cfg.center else 0) + n for n in mel_ref.EDGE_N]
    else:
        js = sorted(set(range(0, min(3 * N, T))) | set(range(max(T - 2 * N, 0), T)))
    assert 0 <= min(js) and max(js) < T
    return cfg, T, js


IMPULSE_CASES = [k for k, c in FFT_CASES.items() if c[0].n_fft <= 32 and c[0].win_length > 1] + ["n2048h2048", "n2048h512"]
