"""The resampler restated in numpy float64, independently of csrc/alac_resample.h, and the host build of
that header for the tests.

    g = gcd(orig, new); o = orig / g; n = new / g; base = min(o, n) * rolloff; width = ceil(W * o / base)
    t = clamp(((k - width) / o - i / n) * base, -W, W);  H[i][k] = 0 where |t| == W, else sinc(pi t) cos(pi t / 2W)^2 base / o
    out_frames(T) = ceil(new * T / orig);  y[j * n + i] = sum_k H[i][k] x[j * o + k - width], x zero outside [0, T)"""
import ctypes
import math

import numpy as np

from tests import host_build

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
    for i in range(min(n, frames)):  # the phases behind `frames` have no column
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


def running_bound(h32, first, x, orig, new, W=6, rolloff=0.99):
    """Per output, the running-error bound of the chain acc = fmaf(h[i][q], x[.], acc), q = 0 .. taps - 1, derived and not
    measured. The terms h[i][q] * x[j * o + first[i] + q - width] are products of two float32 values, exact in float64; s_q
    are their running sums in the chain's order. Every fmaf rounds once, by at most 2^-24 of its result, and its result
    differs from s_q by the error e_(q-1) so far: |e_q| <= |e_(q-1)| (1 + 2^-24) + 2^-24 |s_q|, so |e_taps| <= 2^-24 * sum_q
    |s_q| * (1 + 2^-24)^taps, and (1 + 2^-10) covers that factor for taps up to 2^13. A result below 2^-126 rounds by at most
    2^-150 instead, which taps * 2^-149 covers. |s_q| <= sum |h| |x| for each of the taps sums, so this is below bound()
    wherever that is above the underflow term. -> float64 [R, out_frames]"""
    o, n, _, width = geometry(orig, new, W, rolloff)
    x2 = np.atleast_2d(np.asarray(x, np.float64))
    h = np.asarray(h32, np.float64)
    first = np.asarray(first, np.int64)
    R, T = x2.shape
    taps = h.shape[1]
    frames = out_frames(orig, new, T)
    assert taps <= 1 << 13
    m = np.arange(frames)
    j, i = m // n, m % n
    start = j * o + first[i]  # into the row padded by `width` zeros in front
    xp = np.concatenate([np.zeros((R, width)), x2, np.zeros((R, max(0, int(start.max()) + taps - width - T) + 1))], axis=1)
    out = np.zeros((R, frames))
    step = max(1, (1 << 22) // (taps * R))
    for a in range(0, frames, step):
        idx = start[a:a + step, None] + np.arange(taps)[None, :]
        s = np.cumsum(xp[:, idx] * h[i[a:a + step]][None, :, :], axis=2)
        out[:, a:a + step] = np.abs(s).sum(axis=2)
    return 2.0 ** -24 * (1.0 + 2.0 ** -10) * out + taps * 2.0 ** -149


# ---- impulses: the index arithmetic, exactly --------------------------------------------------------------------------
def impulse_rows(info, orig, new, W=6, rolloff=0.99, amplitude=1.0):
    """Rows of +0.0 with `amplitude` every 2 * width + o + 1 frames, one more than an output's 2 * width + o inputs, so that
    no output sees two impulses; one row per start offset, about 7 of them spread over a spacing (or over the row, where the
    row is shorter), the row long enough for three tiles of the plan's tile_out. -> (x float32 [rows, T], offsets)"""
    o, n, _, width = geometry(orig, new, W, rolloff)
    spacing = 2 * width + o + 1
    T = -(-(3 * info["tile_out"] + 8) * o // n) + 2 * width + 1
    offsets = sorted({int(v) for v in np.linspace(0, min(spacing, T) - 1, 7)})
    x = np.zeros((len(offsets), T), np.float32)
    for r, off in enumerate(offsets):
        x[r, off::spacing] = amplitude
    return x, offsets


def impulse_expected(h32, first, offsets, T, orig, new, W=6, rolloff=0.99, amplitude=1.0):
    """What impulse_rows must come out as, bit for bit, in the restatement's geometry and not by the kernel's walk: with an
    impulse at p, y[j * n + i] = H32[i][p - j * o + width], H32 [n][2 * width + o] holding the plan's h[i] at first[i] and
    +0.0 elsewhere. fmaf(h, a, +0.0) is float32(h * a), exact for a = 1 and a = -0.5, and every other step adds a zero
    product to the accumulator, which leaves it as it is (and +0.0 where it still was +0.0). H32 is not built (44 100 -> 22
    051: 4 GB): output (j, i) sees the inputs [j * o - width, j * o - width + K), K = 2 * width + o, which hold at most one
    impulse since they are K + 1 apart. -> float32 [rows, out_frames]"""
    o, n, _, width = geometry(orig, new, W, rolloff)
    K = 2 * width + o
    spacing = K + 1
    h = np.asarray(h32, np.float32)
    first = np.asarray(first, np.int64)
    taps = h.shape[1]
    frames = out_frames(orig, new, T)
    m = np.arange(frames)
    j, i = m // n, m % n
    lo = j * o - width  # the input under tap k = 0
    y = np.zeros((len(offsets), frames), np.float32)
    for r, off in enumerate(offsets):
        t = np.maximum(-((off - lo) // spacing), 0)  # the first impulse at or behind lo
        p = off + t * spacing
        k = p - lo
        q = k - first[i]
        hit = (k < K) & (p < T) & (q >= 0) & (q < taps)
        v = h[i[hit], q[hit]].astype(np.float64) * amplitude + 0.0
        y[r, hit] = v.astype(np.float32)
    return y


# ---- the host build ---------------------------------------------------------------------------------------------------
def build_resample_sim():
    L = host_build.shared("resample_sim.cpp", "libresample_sim.so", host_build.SIM)
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


def special_rows(rng, T):
    """[5, T] float32 outside the audio range: 0 float32 denormals, one value in ten a normal below 2^-120; 1 values up to FLT_MAX /
    4 of alternating sign in blocks (the filters' sum |h| stays below 2.5, so no sum overflows); 2 a signal with -0.0
    scattered in it; 3 the same signal with one +inf and one NaN; 4 the signal itself."""
    x = np.zeros((5, T), np.float32)
    tiny = rng.integers(1, 1 << 23, T).astype(np.uint32) | (rng.integers(0, 2, T).astype(np.uint32) << 31)  # exponent field 0
    x[0] = tiny.view(np.float32)
    normal = rng.random(T) < 0.1
    x[0, normal] = (rng.uniform(-1, 1, T) * 2.0 ** rng.integers(-124, -120, T)).astype(np.float32)[normal]
    x[1] = (rng.uniform(0.01, 1, T) * np.where((np.arange(T) // 37) % 2 == 0, 1.0, -1.0)).astype(np.float32) * np.float32(3.4028234e38 / 4)
    x[4] = rng.uniform(-1, 1, T).astype(np.float32)
    x[2] = np.where(rng.random(T) < 0.3, np.float32(-0.0), x[4])
    x[3] = x[4]
    x[3, T // 3] = np.inf
    x[3, 2 * T // 3] = np.nan
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


# ---- the parameter cases, shared by the CPU and the GPU suite ---------------------------------------------------------
# (orig, new, lowpass_filter_width, rolloff)
CASES = [(3, 2, 6, 0.99), (8000, 48000, 6, 0.99), (16000, 44100, 6, 0.99), (44100, 48000, 6, 0.99), (11025, 48000, 6, 0.99),
         (44100, 22051, 6, 0.99),                                            # 22 051 phases
         (44100, 16000, 16, 0.9475), (44100, 16000, 64, 0.9475), (44100, 16000, 1, 0.5),
         (48000, 8000, 64, 0.9475),                                          # tile_out 256
         (44100, 8000, 64, 0.9),                                             # tile_out 512
         (192000, 16000, 64, 0.99),                                          # 1 551 taps, tile_out 128
         (192000, 4000, 6, 0.99),                                            # tile_out 64
         (2, 1, 6, 1.0), (1, 2, 6, 1.0),                                     # rolloff 1.0
         (1, 3, 1, 1.0),                                                     # two taps
         (5, 7, 2, 0.3)]                                                     # a low rolloff
TILE_OUT = {(48000, 8000, 64, 0.9475): 256, (44100, 8000, 64, 0.9): 512, (192000, 16000, 64, 0.99): 128, (192000, 4000, 6, 0.99): 64}
OFFSETS = [(0, 0), (1, 3), (2, 1), (3, 2)]  # (out_off, in_off): every misalignment of either side once


def sweep_frames(info, orig, new):
    """boundary_frames, and the length whose output ends 5/8 of a tile behind a tile boundary: with tile_out = 1 024 that last
    tile has three columns for some work items (compute_tile's case 3), which no other length here reaches."""
    tile = info["tile_out"]
    want = tile + 5 * tile // 8
    extra = min(t for t in range(1, 4 * tile * orig // new + 8) if out_frames(orig, new, t) >= want)
    return sorted(set(boundary_frames(info, orig, new)) | {extra})


def tile_counts(tile_out, frames, mis):
    """The column counts of a row's tiles as the header cuts them, restated: tile t is the columns [t * tile_out - mis, (t + 1)
    * tile_out - mis) inside [0, frames), mis the elements of the row's column 0 behind a 16-byte boundary."""
    counts = []
    for t in range((frames + 3 + tile_out - 1) // tile_out):
        a, b = max(t * tile_out - mis, 0), min((t + 1) * tile_out - mis, frames)
        if b > a:
            counts.append(b - a)
    return counts


def chain_paths(tile_out, rows, frames, out_off):
    """{ceil(count / 256)} over the tiles of the rows of layout(): which of compute_tile's four cases a pass runs."""
    _, _, _, out_stride, out_lead, _ = layout(rows, 1, frames, 0, out_off)
    return {-(-c // 256) for r in range(rows) for c in tile_counts(tile_out, frames, (out_lead + r * out_stride) % 4)}
