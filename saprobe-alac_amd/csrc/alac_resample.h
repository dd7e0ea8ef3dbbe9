/*
 * alac_resample.h — float32 rows at one sample rate -> the same rows at another: the plan (filter table), the index
 * arithmetic and the three phases of a tile, as plain host + device code. k_resample.hip builds the gfx950 kernel from this
 * text; tests/host_sim/resample_sim.cpp builds the same text with g++ for the CPU suite.
 *
 * The filter is torchaudio's sinc_interp_hann. With g = gcd(orig, new), o = orig / g, n = new / g, W =
 * lowpass_filter_width and
 *
 *   base  = min(o, n) * rolloff
 *   width = ceil(W * o / base)
 *   t     = clamp(((k - width) / o - i / n) * base, -W, W)                                  phase i < n, tap k < 2 * width + o
 *   H[i][k] = |t| == W ? 0 : sinc(pi t) * cos(pi t / (2 W))^2 * base / o                    in double, sinc(0) = 1
 *   out_frames(T) = ceil(new * T / orig)
 *   y[m] = sum_k H[i][k] * x[j * o + k - width],   m = j * n + i,   x[.] = 0 outside [0, T)
 *
 * |t| grows with the distance of k from width + o * i / n, so the taps of a phase that are not zero are ONE run of at most
 * 2 * width + 1. A plan keeps that window only: first[i], the k of the first kept tap of phase i, and h[i][q] =
 * float(H[i][first[i] + q]) for q < taps, taps the widest run of all phases. make_plan evaluates the window and two taps
 * beyond each end of it, never the n * (2 * width + o) taps of the full table, and refuses a plan in which a tap that is
 * not zero would lie outside a window. The arithmetic of an output is fixed, so that every build gives the same bits:
 *
 *   acc = +0.0f;  for q = 0 .. taps - 1:  acc = fmaf(h[i][q], x[j * o + first[i] + q - width], acc)
 *
 * with +0.0f for an x outside [0, T) (the fmaf is still executed), one accumulator per output, and no other float arithmetic.
 *
 * s(m) = j * o + first[i] does not decrease with m (make_plan checks it), so the inputs of a run of outputs [m0, m0 +
 * count) are the run [s(m0) - width, s(m0 + count - 1) - width + taps). A TILE is tile_out consecutive columns of one output
 * row, cut so that every tile but a row's first starts on a 16-byte boundary of the output's ABSOLUTE address: with mis =
 * the elements of the row's column 0 behind such a boundary, tile t is the columns [t * tile_out - mis, (t + 1) * tile_out -
 * mis) inside [0, out_frames). Phase 1 stages the tile's inputs (LDS on the device) in 16-byte chunks of the absolute
 * address space as alacwf::stage_tile does: whole chunks inside [0, T) with one 16-byte load, the others element by element
 * with zeros for the indices outside [0, T), the image keeping the source's offset within its first chunk. Phase 2: work
 * item w runs the chains of the columns w, w + 256, ... of the tile together (independent accumulators), neighbouring work
 * items on neighbouring phases, so the table is stored [taps][n] on the device; the results go to a second buffer at the
 * row's offset within a 16-byte chunk. Phase 3 stores that buffer: 16 bytes at a time, element by element in the chunks
 * at a row's two ends. tile_out is a multiple of 64, at most 1 024, halved until the inputs of a tile fit kStageFloats.
 */
#ifndef ALAC_RESAMPLE_H
#define ALAC_RESAMPLE_H

#include "alac_waveform.h"

#include <cmath>
#include <vector>

namespace alacrs {

using alacwf::kThreads;

/* staging budget: 15 KB of inputs + 4 KB of outputs = 19 472 bytes of LDS, so that eight workgroups (the 32 waves a CU
 * holds) share a CU's 160 KB */
constexpr uint32_t kStageFloats = 3840;
constexpr uint32_t kMaxTile = 1024, kMinTile = 64;
static_assert(kMaxTile == 4u * kThreads, "compute_tile runs at most four columns per work item");
constexpr uint32_t kOutFloats = kMaxTile + 4;       /* the tile's outputs behind the row's offset within a chunk */
constexpr uint64_t kMaxTableBytes = (uint64_t)64 << 20; /* of n * (2 * width + 2) floats, the bound on the table known before it is built */

/* 16 bytes moved by one instruction */
typedef float F4 __attribute__((vector_size(16), may_alias));

struct Params {
    const float* in;      /* 4-byte aligned */
    uint64_t in_stride;   /* elements */
    uint64_t rows;
    uint64_t in_frames;   /* T */
    float* out;           /* 4-byte aligned */
    uint64_t out_stride;
    uint64_t out_frames;
    const float* ht;      /* [taps][n]: h transposed */
    const int32_t* first; /* [n] */
    uint32_t o, n, width, taps;
    uint32_t tile_out;
    uint64_t tiles_per_row; /* ceil((out_frames + 3) / tile_out): whatever the row's offset within a chunk */
};

/* ceil(n * T / o); false when the product leaves 64 bits */
ALAC_WF_FN bool out_frames_of(uint32_t o, uint32_t n, uint64_t T, uint64_t* out) {
    if (T > (~(uint64_t)0 - o) / n) return false;
    *out = (T * n + o - 1u) / o;
    return true;
}

/* what a tile works on */
struct Tile {
    const float* x; /* the input row's frame 0 */
    float* y;       /* the output row's column 0 */
    uint64_t m0;    /* first column */
    uint32_t count; /* columns; 0: nothing to do */
    uint32_t i0;    /* m0 = j0 * n + i0 */
    int32_t f0;     /* first[i0] */
    int64_t lo;     /* first input staged: s(m0) - width, may be negative */
    uint32_t span;  /* inputs staged: [lo, lo + span) */
    uint32_t sh;    /* elements of x + lo behind a 16-byte boundary */
    uint32_t lead;  /* elements of y + m0 behind a 16-byte boundary (not zero in a row's first tile only) */
};

ALAC_WF_FN Tile make_tile(const Params& p, uint64_t row, uint64_t tile) {
    Tile t{};
    t.x = p.in + row * p.in_stride;
    t.y = p.out + row * p.out_stride;
    const uint32_t mis = (uint32_t)((uintptr_t)t.y >> 2) & 3u;
    const uint64_t a = tile * p.tile_out;
    t.m0 = a > mis ? a - mis : 0u;
    uint64_t end = a + p.tile_out - mis;
    if (end > p.out_frames) end = p.out_frames;
    if (end <= t.m0) return t;
    t.count = (uint32_t)(end - t.m0);
    t.lead = (uint32_t)(((uintptr_t)t.y >> 2) + t.m0) & 3u;
    const uint64_t j0 = t.m0 / p.n; /* the one 64-bit division: everything else is carried from it */
    t.i0 = (uint32_t)(t.m0 - j0 * p.n);
    t.f0 = p.first[t.i0];
    t.lo = (int64_t)(j0 * p.o) + t.f0 - (int64_t)p.width;
    const uint32_t u = t.i0 + t.count - 1u; /* the last column, counted from phase 0 of j0 */
    const uint32_t dj = u / p.n;
    t.span = (uint32_t)((uint64_t)dj * p.o + (uint32_t)(p.first[u - dj * p.n] - t.f0)) + p.taps;
    t.sh = (uint32_t)((int64_t)((uintptr_t)t.x >> 2) + t.lo) & 3u;
    return t;
}

/* Phase 1: work item `tid` of kThreads copies its chunks of the tile's inputs into stage (16-byte aligned, kStageFloats):
 * stage[sh + e] = x[lo + e] for e < span, zero where lo + e is outside [0, T). Nothing outside [0, T) of the row is read. */
ALAC_WF_FN void stage_tile(const Params& p, const Tile& t, float* stage, uint32_t tid) {
    const uint32_t total = t.sh + t.span;
    const int64_t base = t.lo - (int64_t)t.sh; /* x + base is 16-byte aligned */
    const int64_t T = (int64_t)p.in_frames;
    for (uint32_t e0 = 4u * tid; e0 < total; e0 += 4u * kThreads) {
        const int64_t idx0 = base + e0;
        if (e0 >= t.sh && e0 + 4u <= total && idx0 >= 0 && idx0 + 4 <= T) {
            *(F4*)(stage + e0) = *(const F4*)(t.x + idx0);
        } else {
            for (uint32_t b = 0; b < 4u; b++) {
                const uint32_t e = e0 + b;
                const int64_t idx = idx0 + b;
                if (e >= t.sh && e < total) stage[e] = (idx >= 0 && idx < T) ? t.x[idx] : 0.0f;
            }
        }
    }
}

/* R columns per work item: w, w + kThreads, ... Their chains run together, tap by tap. A work item without a column in a
 * turn runs column 0's chain and drops the result. */
template <uint32_t R>
ALAC_WF_FN void run_chains(const Params& p, const Tile& t, const float* stage, float* outb, uint32_t tid) {
    const float* xs[R];
    const float* hp[R];
    float acc[R];
    for (uint32_t r = 0; r < R; r++) {
        const uint32_t c = tid + r * kThreads;
        const uint32_t u = t.i0 + (c < t.count ? c : 0u);
        const uint32_t dj = u / p.n;
        const uint32_t i = u - dj * p.n;
        xs[r] = stage + t.sh + (uint32_t)((uint64_t)dj * p.o + (uint32_t)(p.first[i] - t.f0));
        hp[r] = p.ht + i;
        acc[r] = 0.0f;
    }
    for (uint32_t q = 0; q < p.taps; q++)
        for (uint32_t r = 0; r < R; r++) {
            acc[r] = fmaf(*hp[r], xs[r][q], acc[r]);
            hp[r] += p.n;
        }
    for (uint32_t r = 0; r < R; r++) {
        const uint32_t c = tid + r * kThreads;
        if (c < t.count) outb[t.lead + c] = acc[r];
    }
}

/* Phase 2: work item `tid` of kThreads runs its columns' chains out of stage into outb (16-byte aligned, kOutFloats). */
ALAC_WF_FN void compute_tile(const Params& p, const Tile& t, const float* stage, float* outb, uint32_t tid) {
    switch ((t.count + kThreads - 1u) / kThreads) {
    case 1: run_chains<1>(p, t, stage, outb, tid); break;
    case 2: run_chains<2>(p, t, stage, outb, tid); break;
    case 3: run_chains<3>(p, t, stage, outb, tid); break;
    default: run_chains<4>(p, t, stage, outb, tid); break;
    }
}

/* Phase 3: work item `tid` of kThreads stores its 16-byte chunks of outb: chunk k is the columns m0 + 4 k - lead + [0, 4). */
ALAC_WF_FN void store_tile(const Params& p, const Tile& t, const float* outb, uint32_t tid) {
    (void)p;
    const uint32_t total = t.lead + t.count;
    float* dst = t.y + t.m0 - t.lead; /* 16-byte aligned; in front of the row when lead != 0, then it is not stored to */
    for (uint32_t e0 = 4u * tid; e0 < total; e0 += 4u * kThreads) {
        if (e0 >= t.lead && e0 + 4u <= total) {
            *(F4*)(dst + e0) = *(const F4*)(outb + e0);
        } else {
            for (uint32_t b = 0; b < 4u; b++)
                if (e0 + b >= t.lead && e0 + b < total) dst[e0 + b] = outb[e0 + b];
        }
    }
}

/* ---- the plan: host only ------------------------------------------------------------------------------------------- */
struct Plan {
    uint32_t o = 0, n = 0, width = 0, taps = 0, tile_out = 0;
    std::vector<float> h;       /* [n][taps], each entry the double value rounded once */
    std::vector<int32_t> first; /* [n] */
    std::vector<float> ht;      /* [taps][n], what the device reads */
};

/* H[i][k] */
inline double tap(uint32_t o, uint32_t n, uint32_t width, double W, double base, uint32_t i, int64_t k) {
    double t = ((double)(k - (int64_t)width) / (double)o - (double)i / (double)n) * base;
    if (t < -W) t = -W;
    if (t > W) t = W;
    if (std::fabs(t) == W) return 0.0;
    const double pi = 3.14159265358979323846;
    const double s = t == 0.0 ? 1.0 : std::sin(pi * t) / (pi * t);
    const double c = std::cos(pi * t / (2.0 * W));
    return s * c * c * base / (double)o;
}

/* inputs a tile of tc columns can need, with the offset within the first chunk: the widest s(m + tc - 1) - s(m), + taps + 3 */
inline uint64_t stage_need(const Plan& pl, uint32_t tc) {
    uint64_t widest = 0;
    for (uint32_t i0 = 0; i0 < pl.n; i0++) {
        const uint64_t u = (uint64_t)i0 + tc - 1u;
        const uint64_t d = (u / pl.n) * pl.o + (uint64_t)pl.first[u % pl.n] - (uint64_t)pl.first[i0];
        if (d > widest) widest = d;
    }
    return widest + pl.taps + 3u;
}

/* false: no plan for these arguments (a rate of 0, equal rates, W = 0, rolloff outside (0, 1], a table above kMaxTableBytes,
 * or 64 outputs whose inputs do not fit the staging buffer) */
inline bool make_plan(uint32_t orig, uint32_t new_, uint32_t W, double rolloff, Plan* out) {
    if (!orig || !new_ || orig == new_ || !W || !(rolloff > 0.0 && rolloff <= 1.0)) return false;
    uint32_t a = orig, b = new_;
    while (b) {
        const uint32_t r = a % b;
        a = b;
        b = r;
    }
    Plan pl;
    pl.o = orig / a;
    pl.n = new_ / a;
    const uint32_t o = pl.o, n = pl.n;
    const double base = (double)(o < n ? o : n) * rolloff;
    const double wd = std::ceil((double)W * (double)o / base);
    if (!(wd >= 1.0) || 2.0 * wd + 2.0 + 3.0 > (double)kStageFloats) return false; /* one output does not fit, let alone 64 */
    pl.width = (uint32_t)wd;
    const uint32_t width = pl.width;
    if ((uint64_t)n * (2u * width + 2u) * sizeof(float) > kMaxTableBytes) return false;
    const uint64_t K = 2ull * width + o; /* taps of the full table */
    if (K > 0x7fffffffu) return false;
    const double dW = (double)W, half = (double)o * dW / base;
    /* pass 1: each phase's run of taps that are not zero */
    pl.first.resize(n);
    std::vector<uint32_t> run(n);
    for (uint32_t i = 0; i < n; i++) {
        const double centre = (double)width + (double)o * (double)i / (double)n;
        int64_t klo = (int64_t)std::floor(centre - half) - 2, khi = (int64_t)std::ceil(centre + half) + 2;
        if (klo < 0) klo = 0;
        if (khi > (int64_t)K - 1) khi = (int64_t)K - 1;
        int64_t f = -1, l = -1;
        for (int64_t k = klo; k <= khi; k++)
            if (tap(o, n, width, dW, base, i, k) != 0.0) {
                if (f < 0) f = k;
                l = k;
            }
        /* |t| only grows beyond a zero tap: a zero at each end of the scan (or the table's end) closes the run */
        if (f < 0 || (f == klo && klo != 0) || (l == khi && khi != (int64_t)K - 1)) return false;
        pl.first[i] = (int32_t)f;
        run[i] = (uint32_t)(l - f + 1);
        if (run[i] > pl.taps) pl.taps = run[i];
    }
    /* windows of one length, inside the table, starting where s(m) = j * o + first[i] does not decrease */
    for (uint32_t i = 0; i < n; i++) {
        if ((uint64_t)pl.first[i] + pl.taps > K) pl.first[i] = (int32_t)(K - pl.taps);
        if (i && pl.first[i] < pl.first[i - 1]) return false;
    }
    if ((uint64_t)pl.first[n - 1] > (uint64_t)pl.first[0] + o) return false;
    /* pass 2: the window */
    pl.h.resize((size_t)n * pl.taps);
    pl.ht.resize((size_t)n * pl.taps);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t q = 0; q < pl.taps; q++) {
            const float v = (float)tap(o, n, width, dW, base, i, (int64_t)pl.first[i] + q);
            pl.h[(size_t)i * pl.taps + q] = v;
            pl.ht[(size_t)q * n + i] = v;
        }
    uint32_t tc = kMaxTile;
    while (tc > kMinTile && stage_need(pl, tc) > kStageFloats) tc /= 2u;
    if (stage_need(pl, tc) > kStageFloats) return false;
    pl.tile_out = tc;
    *out = std::move(pl);
    return true;
}

/* the arguments of one pass; false for what the entry rejects */
inline bool make_params(const Plan& pl, const float* in, uint64_t in_stride, uint64_t rows, uint64_t in_frames, float* out,
                        uint64_t out_stride, const float* ht, const int32_t* first, Params* p) {
    if (!in || !out || ((uintptr_t)in & 3u) || ((uintptr_t)out & 3u)) return false;
    uint64_t of;
    if (!out_frames_of(pl.o, pl.n, in_frames, &of) || of > ((uint64_t)1 << 62)) return false;
    if (in_stride < in_frames || out_stride < of) return false;
    const uint64_t lim = (SIZE_MAX / 8u) / rows;
    if (in_stride > lim || out_stride > lim) return false;
    const uint64_t tpr = (of + 3u + pl.tile_out - 1u) / pl.tile_out;
    if (tpr > (~(uint64_t)0) / rows) return false;
    *p = Params{in, in_stride, rows, in_frames, out, out_stride, of, ht, first, pl.o, pl.n, pl.width, pl.taps, pl.tile_out, tpr};
    return true;
}

}  // namespace alacrs

#if defined(__HIPCC__)
/* k_resample.hip */
namespace alack {
/* All kernels of one pass on `stream`. */
hipError_t resample_launch(hipStream_t stream, const alacrs::Params& p);
}  // namespace alack
#endif
#endif /* ALAC_RESAMPLE_H */
