"""The Kaldi feature pass with transform="fft" (DESIGN.md §15b): its derived ceilings against tests/kaldi_ref.py's step-by-step
float64 restatement, independently of csrc/alac_fbankfft.h; the host build of that header (tests/host_sim/fbankfft_sim.cpp); and
the cases both suites run.

The ceiling, u = 2^-24. x is the raw frame, W samples; everything is relative to x, not to z: with a DC offset the cancellation in
x - mean is the point.
    mean    P = 256 / tile_frames classes: a sample passes ceil(W / P) - 1 additions of its class (the first one, to +0.0, is
            exact), log2(P) of the tree and the division: D = ceil(W / P) + log2(P) roundings,
            dm = ((1 + u)^D - 1) sum |x| / W;  0 without remove_dc_offset
    v       dv[n] = dm (1 + u) + u |v[n]|;  0 without remove_dc_offset (v = x)
    y       dy[n] = (dv[n] + |c32| dv[n - 1] + |c32 - c| |v[n - 1]|)(1 + u) + u |y[n]|;  dv[n] where c32 = 0
    z       dz[n] = (|ws[n]| dy[n] + |ws[n] - scale win[n]| |y[n]|)(1 + u) + u |z[n]|, ws the plan's own float32 table
    X       eta_fft = u (sum over the passes of g(r) + 4), g = melfft_ref.G (passes and split, §14a);
            |dX[k]| <= e = eta_fft sqrt(N) (||z||_2 + ||dz||_2) + sqrt(N) ||dz||_2
    p, mel  dp = (2 |X| e + e^2)(1 + 2 u) + 2 u p;   dmel = sum fb dp + taps u sum fb (p + dp)     (mel_ref.bounds' form)
    energy  kaldi_ref.prelog_bounds' (the same function computes it, so the same ceiling holds)"""
import ctypes
import math

import numpy as np

from tests import host_build
from tests import kaldi_ref as kr
from tests import mel_ref as mr
from tests import melfft_ref as fr

ROOT = kr.ROOT
U = kr.U
Cfg = kr.Cfg
THREADS = 256


# ---- the definition's numbers -----------------------------------------------------------------------------------------
def radices_of(N):
    """The passes of N / 2: the 5s, the 3s, the 4s, then a 2"""
    m, out = N // 2, []
    for r in (5, 3, 4, 2):
        while m % r == 0:
            out.append(r)
            m //= r
    assert m == 1
    return out


def lds_rule(cfg):
    """-> (tile_frames, batch_frames, floats): 64 halved down to 4 with batch_frames = tile_frames until the tile fits 64 KB, then
    only batch_frames halves down to 1. The staging image (or the output tile in its place), the power tile [tile_frames][K | 1]
    rounded up to 4, tile_frames of energy, MFCC's [num_ceps][tile_frames], 256 sums with remove_dc_offset, and batch_frames x
    pitch complex"""
    M = cfg.N // 2
    pitch = (M + ((M - 1) >> 4)) | 1

    def need(tf, batch):
        a = (tf - 1) * cfg.h + cfg.W + 3 if cfg.h <= cfg.W else tf * cfg.W
        a = max(a, (cfg.mels + (1 if cfg.energy and not cfg.ceps else 0)) * tf)
        a = (a + 3) // 4 * 4
        pt = (tf * (cfg.K | 1) + 3) // 4 * 4
        return a + pt + (tf if cfg.energy else 0) + cfg.ceps * tf + (THREADS if cfg.dc else 0) + 2 * batch * pitch
    tf = 64
    while tf > 4 and need(tf, tf) > kr.LDS_FLOATS:
        tf //= 2
    batch = tf
    while batch > 1 and need(tf, batch) > kr.LDS_FLOATS:
        batch //= 2
    return tf, batch, need(tf, batch)


# ---- the ceilings -----------------------------------------------------------------------------------------------------
def eta_fft(radices):
    return U * (sum(fr.G[r] for r in radices) + fr.SPLIT_SHARE)


def reference(cfg, plan, x):
    """cfg with nothing logged, plan = sim_plan's or KaldiFeatures.plan() merged with fft_plan() (window, radix, tile_frames, fb,
    first, taps) -> (ref [R, F, cols] float64 = kr.features64 over the plan's filterbank, lim of the same shape)"""
    assert not cfg.ceps and not cfg.log and not cfg.log_energy
    W, N = cfg.W, cfg.N
    fb32 = kr.dense_fb(plan)
    ref = kr.features64(cfg, x, fb=fb32)
    xr = kr.raw_frames(cfg, x)  # [R, F, W]
    ax = np.abs(xr)
    P = THREADS // plan["tile_frames"]
    D = -(-W // P) + int(math.log2(P))
    if cfg.dc:
        mean = xr.mean(axis=-1, keepdims=True)
        dm = (((1 + U) ** D - 1) * ax.sum(axis=-1, keepdims=True) / W)
        v = xr - mean
        dv = dm * (1 + U) + U * np.abs(v)
    else:
        v, dv = xr, np.zeros(xr.shape)
    c = cfg.pre
    c32 = float(np.float32(c))
    if c32 != 0.0:
        vp = np.concatenate([v[..., :1], v[..., :-1]], axis=-1)
        dvp = np.concatenate([dv[..., :1], dv[..., :-1]], axis=-1)
        y = v - c * vp
        dy = (dv + abs(c32) * dvp + abs(c32 - c) * np.abs(vp)) * (1 + U) + U * np.abs(y)
    else:
        y, dy = v, dv
    sw = cfg.scale * kr.window(cfg)
    ws = np.asarray(plan["window"][:W], np.float64)
    z = sw * y
    dz = (np.abs(ws) * dy + np.abs(ws - sw) * np.abs(y)) * (1 + U) + U * np.abs(z)
    zn = np.sqrt((z * z).sum(axis=-1))
    dzn = np.sqrt((dz * dz).sum(axis=-1))
    e = (eta_fft(plan["radix"]) * math.sqrt(N) * (zn + dzn) + math.sqrt(N) * dzn)[..., None]
    X = np.fft.rfft(z, n=N, axis=-1)
    p = X.real ** 2 + X.imag ** 2
    dp = (2 * np.abs(X) * e + e * e) * (1 + 2 * U) + 2 * U * p
    fb = np.asarray(fb32, np.float64)
    dmel = np.einsum("mk,rfk->rfm", fb, dp) + plan["taps"] * U * np.einsum("mk,rfk->rfm", fb, p + dp)
    # the energy: kr.prelog_bounds' ceiling of alacfb::energy_tile
    mean_e = xr.mean(axis=-1, keepdims=True) if cfg.dc else np.zeros(xr.shape[:-1] + (1,))
    d = np.abs(xr - mean_e)
    dme = ((W + 1) * U * ax.sum(axis=-1) / W) if cfg.dc else np.zeros(xr.shape[:-1])
    de = cfg.scale ** 2 * ((W + 2) * U * (d * d).sum(axis=-1) + 2 * dme * d.sum(axis=-1) + W * dme * dme)
    return ref, kr.arrange(cfg, dmel, de)


def share(cfg, plan, x, got, what=""):
    """got [R, F, cols] float32 with nothing logged against reference(): asserts the ceiling -> the largest error / ceiling"""
    ref, lim = reference(cfg, plan, x)
    return kr.assert_within(got, ref, lim, what)


# ---- the host build -----------------------------------------------------------------------------------------------------
def build_fbankfft_sim():
    L = host_build.shared("fbankfft_sim.cpp", "libfbankfft_sim.so", host_build.SIM_FP)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.fbankfft_sim_plan.argtypes = [vp, vp, vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64]
    L.fbankfft_sim_run.argtypes = [vp, vp, vp, u64, u64, u64, vp, u64, u64, ctypes.c_int]
    return L


def build_fbankfft_shim(pkg):
    """tests/host_sim/fbankfft_shim.cpp over host/kaldi_features.hpp, linked with the library"""
    L = host_build.shared("fbankfft_shim.cpp", "libfbankfft_shim.so", host_build.SHIM, host_build.library(pkg))
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    L.fbankfft_shim_run.restype = ctypes.c_long
    L.fbankfft_shim_run.argtypes = [vp, u32, vp, sz, sz, sz, vp, sz, sz, vp, vp, vp, vp, vp, vp]
    L.fbankfft_shim_last_error.restype = ctypes.c_char_p
    return L


FFT_INFO = fr.FFT_INFO
PLACES = ("a_floats", "p_floats", "e_off", "c_off", "s_off", "b_off", "parts")
TABLES = ("fb", "first", "dct", "lifter")  # what an FFT plan shares with the direct one


def sim_plan(S, cfg, **refused):
    """-> dict of the host build's FFT plan (kr.INFO, FFT_INFO, radix, PLACES, window [N], twiddle, fb, first, dct, lifter), or None
    where it has none"""
    w, d = cfg.words(**refused)
    info = np.zeros(33, np.uint32)
    if S.fbankfft_sim_plan(w.ctypes.data, d.ctypes.data, info.ctypes.data, *([None, 0] * 6)) != 0:
        return None
    out = {k: int(v) for k, v in zip(kr.INFO, info)}
    out.update({k: int(v) for k, v in zip(FFT_INFO, info[10:])})
    out["radix"] = [int(r) for r in info[16:16 + out["n_passes"]]]
    out.update({k: int(v) for k, v in zip(PLACES, info[26:])})
    win = np.zeros(int(info[24]), np.float32)
    tw = np.zeros(int(info[25]), np.float32)
    fb = np.zeros((out["num_mel_bins"], out["taps"]), np.float32)
    first = np.zeros(out["num_mel_bins"], np.int32)
    dct = np.zeros((out["num_ceps"], out["num_mel_bins"]), np.float32)
    lif = np.zeros(out["num_ceps"], np.float32)
    assert S.fbankfft_sim_plan(w.ctypes.data, d.ctypes.data, info.ctypes.data, win.ctypes.data, win.size, tw.ctypes.data, tw.size,
                               fb.ctypes.data, fb.size, first.ctypes.data, first.size, dct.ctypes.data, dct.size, lif.ctypes.data,
                               lif.size) == 0
    out.update(window=win, twiddle=tw, fb=fb, first=first, dct=dct, lifter=lif)
    return out


def handle_plan(kf):
    """A KaldiFeatures handle's plan() and fft_plan() as one dict of sim_plan's keys (without PLACES)"""
    out = dict(kf.plan())
    out.update(kf.fft_plan())
    return out


def same_plan(lib, sim):
    """The library's plan (handle_plan) against the host build's"""
    numbers = all(lib[k] == sim[k] for k in kr.INFO + FFT_INFO + ("radix",))
    return numbers and lib["basis"].size == 0 and all(
        np.array_equal(lib[k].view(np.uint32), sim[k].view(np.uint32)) for k in TABLES + ("window", "twiddle"))


def sim_image(S, cfg, x, in_off=0, out_off=0, pad=0, guard=0):
    """kr.sim_image over the FFT build"""
    rows, T = x.shape
    lay = kr.layout(cfg, rows, T, in_off, out_off, pad)
    in_stride, in_lead, in_elems, row_stride, inner, out_lead, out_elems = lay
    src = mr.aligned(in_elems, 0x7FC00000)
    for r in range(rows):
        src[in_lead + r * in_stride: in_lead + r * in_stride + T] = x[r].view(np.uint32)
    img = mr.aligned(out_elems, mr.SENTINEL)
    w, d = cfg.words()
    rc = S.fbankfft_sim_run(w.ctypes.data, d.ctypes.data, src.ctypes.data + 4 * in_lead, in_stride, rows, T,
                            img.ctypes.data + 4 * out_lead, row_stride, inner, guard)
    assert rc == 0, rc
    return img.copy(), lay


def host_values(S, cfg, x, guard=0):
    img, lay = sim_image(S, cfg, x, guard=guard)
    return kr.values_of(img, lay, cfg, x.shape[0], x.shape[1])


# ---- the cases, shared by the CPU and the GPU suite: name -> (Cfg, tile_frames, batch_frames, radices) ----------------------
def _case(cfg):
    tf, batch, _ = lds_rule(cfg)
    return cfg, tf, batch, radices_of(cfg.N)


FROM_KALDI = ["w8", "w10", "w3", "ns10", "ns9", "h37", "h37ns", "hanning", "hamming", "rectangular", "blackman", "nodc", "c0", "scale",
              "e_first_1", "e_first_0", "e_last_1", "e_last_0", "mfcc13", "mfcc_htk", "mfcc_e_htk", "mfcc_ns", "asr", "k48", "full",
              "manymels"]
FFT_CASES = {k: _case(kr.CASES[k][0]) for k in FROM_KALDI}
FFT_CASES.update({
    "w2": _case(Cfg(8000, 2, 1, mels=1)),                         # N 2: no pass
    "w7r": _case(Cfg(8000, 7, 3, mels=4)),                        # W 7 rounded to N 8
    "n6": _case(Cfg(8000, 6, 2, mels=3, pow2=False)),             # radix 3
    "n10": _case(Cfg(8000, 10, 4, mels=4, pow2=False)),           # 5
    "n12": _case(Cfg(8000, 12, 5, mels=5, pow2=False)),           # 3 2
    "n30": _case(Cfg(8000, 30, 11, mels=8, pow2=False)),          # 5 3
    "n50": _case(Cfg(8000, 50, 20, pow2=False)),                  # 5 5
    "n400": _case(Cfg(16000, 400, 160, mels=80, pow2=False)),     # 5 5 4 2
    "b2": _case(Cfg(48000, 2048, 512, pow2=False)),               # 1 < batch_frames < tile_frames: a batch filled in part
})
# what the rule and the radices must come to where the issue names them
PINNED = {"w2": (64, 64, []), "w3": (64, 64, [2]), "w8": (64, 64, [4]), "w10": (64, 64, [4, 2]), "w7r": (64, 64, [4]),
          "n6": (64, 64, [3]), "n10": (64, 64, [5]), "n12": (64, 64, [3, 2]), "n30": (64, 64, [5, 3]), "n50": (64, 64, [5, 5]),
          "n400": (16, 16, [5, 5, 4, 2]), "asr": (16, 16, [4, 4, 4, 4]), "k48": (4, 4, [4, 4, 4, 4, 4]), "full": (4, 1, [4, 4, 4, 4, 4]),
          "manymels": (4, 4, [4, 4, 2]), "b2": (4, 2, [4, 4, 4, 4, 4])}
SMALL = [k for k, c in FFT_CASES.items() if c[0].W <= 64 and c[0].mels <= 128]
IMPULSE_CASES = [k for k, c in FFT_CASES.items() if c[0].W <= 16 and not c[0].ceps and not c[0].energy]
REFUSED = [Cfg(8000, 1, 1), Cfg(8000, 7, 3, pow2=False), Cfg(8000, 14, 3, pow2=False), Cfg(8000, 22, 5, pow2=False)]


def case_runs(name):
    """The inputs of a case, the same in both suites so that their ceiling shares are the same numbers: (k, rows, T, x) at F =
    tile_frames - 1, tile_frames, tile_frames + 1 and 1 (or the shortest row); rows 1 and 3 for the small cases and at tile_frames
    + 1, else 1; the rows of 3 on a DC offset of 0.3"""
    cfg, tf = FFT_CASES[name][:2]
    rng = np.random.default_rng(len(name) + cfg.W)
    for k, T in enumerate(kr.case_lengths(cfg, tf)):
        for rows in (1, 3) if name in SMALL or k == 2 else (1,):
            yield k, rows, T, kr.signal(rng, rows, T, 0.3 if rows == 3 else 0.0)


def impulse_batch(name):
    """kr.impulse_batch over FFT_CASES: -> (cfg for impulses, T, positions)"""
    cfg, tf = FFT_CASES[name][:2]
    cfg = kr.impulse_cfg(cfg)
    T = kr.length_for(cfg, tf + 3)
    js = sorted(set(range(0, min(T, 3 * cfg.W))) | set(range(max(0, T - 2 * cfg.W), T)))
    return cfg, T, js


def check_constant(run, plan_of):
    """A row of constant 0.5 with DC removal at scale 1 and 32768 (W 10: the classes' sums, the tree and the quotient are exact):
    every unlogged mel column is +0.0 and the energy is +0.0; logged, every mel column is float32(ln 2^-23)"""
    for scale in (1.0, 32768.0):
        cfg = kr.CASES["e_first_1"][0].with_(scale=scale)
        x = np.full((1, kr.length_for(cfg, 66)), 0.5, np.float32)
        got = run(cfg.prelog(), x)
        assert got.shape == (1, 66, 24) and not got.view(np.uint32).any(), "a constant row is not +0.0 at scale %g" % scale
        logged = run(cfg.with_(energy=False), x)
        assert (logged.view(np.uint32) == kr.LOG_EPS32.view(np.uint32)).all(), "the log of a constant row at scale %g" % scale
