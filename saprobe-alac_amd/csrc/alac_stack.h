/*
 * alac_stack.h — the step behind the normalisation: float32 features [rows][frames][bins] with per-row lengths -> deltas,
 * context splicing and subsampling in one pass, with lengths of their own, as plain host + device code. k_stack.hip builds the
 * gfx950 kernel from this text; tests/host_sim/stack_sim.cpp builds the same text with g++ (contraction off) for the CPU suite.
 *
 * Input and output are addressed as alac_featview.h says: three element strides each, one inner stride 1, n_r valid frames in
 * row r.
 *
 * Parameters, fixed at create: order 0..2, window 1..8 (read only when order > 0), left and right 0..16, stride 1..64,
 * pad_value any float.
 *
 * Delta weights, Kaldi's DeltaFeatures: w_0 = [1]; w_k = w_(k-1) convolved with the ramp j = -window .. window, divided by
 * sum j^2; half-width M_k = k * window. Each table is built once as exact integer numerators over (sum j^2)^k and rounded to
 * float32 once.
 *   d_k[t][b] = the chain acc = fmaf(w_k[i], x[clamp(t + i, 0, n_r - 1)][b], acc) for i = -M_k .. M_k in that order from +0.0f;
 *               taps whose weight is zero are skipped; d_0 = x, copied and never multiplied.
 * Order 1 is torchaudio's compute_deltas(mode="replicate") with win_length = 2 * window + 1. Order 2 is Kaldi's: one clamp, on x,
 * and not compute_deltas applied twice.
 *
 * Output: G = ceil(frames / stride) frames of D = (left + right + 1) * (order + 1) * bins columns, m_r = ceil(n_r / stride) of them
 * valid in row r:
 *   y[r][g][(c * (order + 1) + k) * bins + b] = d_k[clamp(g * stride + c - left, 0, n_r - 1)][b]   for g < m_r, c = 0 .. left + right
 *   y[r][g][.] = pad_value                                                                         for g >= m_r
 *   out_lengths[r] = m_r (int32; the pointer may be NULL)
 * The input at frames >= n_r is never read. The output has three strides of its own and either layout, whatever the input's; it
 * may not overlap the input.
 *
 * A TILE is tile_out consecutive output frames of one row, one workgroup of 256. It needs the input frames [g0 * stride - left -
 * M_order, (g0 + tile_out - 1) * stride + right + M_order] clamped to [0, n_r - 1]: at most tile_in of them. Where one image of
 * all bins would not fit, the workgroup walks the bins in slabs of tile_bins. Per slab: stage_slab brings the frames into image 0
 * (LDS on the device) with alacfv::lines_in along the contiguous axis, at an odd pitch in the bins layout; delta_slab computes
 * d_1 and d_2 once each into images 1 and 2 of the same geometry; store_slab writes the output along its contiguous axis out of
 * the images: whole lines of D floats in the frames layout, runs of frames per column in the bins layout, 16 bytes at a time in
 * the absolute 16-byte chunks, elements at the ends. tile_out, tile_bins and the LDS size are functions of the parameters alone
 * (plan_of). All index arithmetic that leaves a tile is in 64 bits; there is no atomic; no operation is contracted.
 */
#ifndef ALAC_STACK_H
#define ALAC_STACK_H

#include "alac_featview.h"

#include <cmath>

namespace alacst {

using alacfv::F4, alacfv::kThreads, alacfv::length_of, alacfv::lines_in;

constexpr uint32_t kMaxBins = 4096, kMaxCols = 4096;
constexpr uint32_t kMaxOrder = 2, kMaxWindow = 8, kMaxContext = 16, kMaxStride = 64;
constexpr uint32_t kMaxTileOut = 64;  /* 256 contiguous bytes of a column in the bins layout */
constexpr uint32_t kLdsFloats = 6400; /* 25 600 bytes, half the normalisation pass's: six workgroups share a CU's 160 KB, which
                                         measured faster than three with tiles twice as long */
constexpr uint32_t kMaxWeights = (2u * kMaxWindow + 1u) + (4u * kMaxWindow + 1u); /* w_1 then w_2 */

struct Config {
    uint32_t bins, order, window, left, right, stride;
    float pad_value;
};

struct Plan {
    uint32_t cols;      /* D */
    uint32_t tile_bins; /* bins of a slab */
    uint32_t tile_out;  /* output frames of a tile */
    uint32_t tile_in;   /* input frames a tile stages at most */
    uint32_t pitch;     /* tile_in | 1: a bin's line in the bins layout */
    uint32_t lds_floats;
};

struct Params {
    const float* in;
    uint64_t in_rs, in_fs, in_bs; /* elements */
    float* out;
    uint64_t out_rs, out_fs, out_bs;
    const int32_t* lengths; /* [rows], may be null */
    int32_t* out_lengths;   /* [rows], may be null */
    uint64_t rows, frames;
    uint64_t out_frames; /* G */
    uint64_t tiles;      /* of a row: ceil(G / tile_out) */
    const float* w;      /* w_1 (2 window + 1 floats), then w_2 (4 window + 1) */
    uint32_t bins, order, window, left, right, stride;
    uint32_t cols, tile_bins, tile_out, tile_in, pitch;
    float pad_value;
};

/* what a tile works on */
struct Tile {
    uint64_t row, n; /* the row's valid input frames */
    uint64_t g0;     /* the tile's first output frame */
    uint32_t ng, gv; /* its output frames, and how many of them are valid */
    uint64_t lo;     /* the first input frame staged: image frame 0 */
    uint32_t nfr;    /* input frames staged: [lo, lo + nfr) */
    uint64_t mlo;    /* the first frame whose deltas are computed */
    uint32_t nmid;   /* how many: [mlo, mlo + nmid) */
    int32_t off;     /* g0 * stride - left - lo: output frame g0 + gl at context position c reads image frame
                        clamp(off + gl * stride + c, mlo - lo, mlo - lo + nmid - 1), which is the clamp to [0, n - 1] for every
                        valid gl: below mlo only a negative frame lies, above mlo + nmid - 1 only one behind n - 1 */
    uint32_t lf, lb; /* element (f, b) of a slab is image[(f - lo) * lf + (b - b0) * lb] */
    uint32_t image;  /* floats of one image */
    float* y;        /* the output row's frame g0, column 0 */
};

ALAC_WF_FN Tile make_tile(const Params& p, uint64_t row, uint64_t tile) {
    Tile t{};
    t.row = row;
    t.n = length_of(p.lengths, p.frames, row);
    t.g0 = tile * p.tile_out;
    const uint64_t m = (t.n + p.stride - 1u) / p.stride;
    t.ng = p.out_frames - t.g0 < p.tile_out ? (uint32_t)(p.out_frames - t.g0) : p.tile_out;
    t.gv = m > t.g0 ? (m - t.g0 < t.ng ? (uint32_t)(m - t.g0) : t.ng) : 0u;
    if (t.gv) { /* g0 * stride <= n - 1 */
        const uint32_t M = p.order * p.window;
        const uint64_t a = t.g0 * p.stride, last = t.n - 1u;
        t.mlo = a > p.left ? a - p.left : 0u;
        uint64_t mhi = (t.g0 + t.gv - 1u) * p.stride + p.right;
        if (mhi > last) mhi = last;
        t.lo = t.mlo > M ? t.mlo - M : 0u;
        const uint64_t hi = mhi + M > last ? last : mhi + M;
        t.nfr = (uint32_t)(hi - t.lo + 1u);
        t.nmid = (uint32_t)(mhi - t.mlo + 1u);
        t.off = (int32_t)((int64_t)a - (int64_t)p.left - (int64_t)t.lo);
    }
    if (p.in_bs == 1u) { /* frames layout: the image is the frames one behind the other */
        t.lf = p.tile_bins;
        t.lb = 1u;
    } else { /* bins layout: the bins one behind the other, at an odd pitch */
        t.lf = 1u;
        t.lb = p.pitch;
    }
    t.image = p.tile_bins * p.pitch;
    t.y = p.out + row * p.out_rs + t.g0 * p.out_fs;
    return t;
}

ALAC_WF_FN uint32_t slab_bins(const Params& p, uint32_t b0) { return p.bins - b0 < p.tile_bins ? p.bins - b0 : p.tile_bins; }

/* the row's count of output frames, once per row */
ALAC_WF_FN void put_length(const Params& p, const Tile& t, uint32_t tid) {
    if (p.out_lengths && t.g0 == 0u && tid == 0u) p.out_lengths[t.row] = (int32_t)((t.n + p.stride - 1u) / p.stride);
}

/* Phase 1: the bins [b0, b0 + nb) of the tile's nfr input frames into image 0. Frames that follow each other without a gap are
 * one line. */
ALAC_WF_FN void stage_slab(const Params& p, const Tile& t, uint32_t b0, float* image, uint32_t tid) {
    const uint32_t nb = slab_bins(p, b0);
    const float* x = p.in + t.row * p.in_rs + t.lo * p.in_fs + (uint64_t)b0 * p.in_bs;
    if (p.in_bs == 1u) {
        if (p.in_fs == p.bins && nb == p.bins) lines_in(x, 0u, 1u, t.nfr * nb, image, 0u, 1u, tid);
        else lines_in(x, p.in_fs, t.nfr, nb, image, t.lf, 1u, tid);
    } else {
        lines_in(x, p.in_bs, nb, t.nfr, image, t.lb, 1u, tid);
    }
}

/* Phase 2: d_1 .. d_order of the frames [mlo, mlo + nmid) into the images 1 .. order, each element one chain over image 0 */
ALAC_WF_FN void delta_slab(const Params& p, const Tile& t, uint32_t b0, float* image, uint32_t tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t nb = slab_bins(p, b0);
    const uint32_t total = t.nmid * nb;
    const int64_t last = (int64_t)t.n - 1;
    for (uint32_t k = 1; k <= p.order; k++) {
        const int32_t M = (int32_t)(k * p.window);
        const float* w = p.w + (k == 1u ? 0u : 2u * p.window + 1u) + M;
        float* d = image + k * t.image;
        for (uint32_t e = tid; e < total; e += kThreads) {
            const uint32_t fm = e / nb, bl = e - fm * nb;
            const int64_t f = (int64_t)(t.mlo + fm);
            float acc = 0.0f;
            for (int32_t i = -M; i <= M; i++) {
                const float wi = w[i];
                if (wi == 0.0f) continue;
                int64_t fi = f + i;
                fi = fi < 0 ? 0 : fi > last ? last : fi;
                acc = fmaf(wi, image[(uint32_t)(fi - (int64_t)t.lo) * t.lf + bl * t.lb], acc);
            }
            d[(uint32_t)(f - (int64_t)t.lo) * t.lf + bl * t.lb] = acc;
        }
    }
}

/* output frame g0 + gl, context position c, order k, bin b0 + bl of the slab */
ALAC_WF_FN float element_of(const Params& p, const Tile& t, const float* image, uint32_t gl, uint32_t c, uint32_t k, uint32_t bl) {
    if (gl >= t.gv) return p.pad_value;
    const int32_t first = (int32_t)(t.mlo - t.lo), last = first + (int32_t)t.nmid - 1;
    int32_t f = t.off + (int32_t)(gl * p.stride + c);
    f = f < first ? first : f > last ? last : f;
    return image[k * t.image + (uint32_t)f * t.lf + bl * t.lb];
}

/* Phase 3, frames layout of the output: the tile's ng lines of D columns (one line where they follow each other without a gap;
 * per frame and (c, k) a segment of the slab's bins where the slab is not all bins) */
ALAC_WF_FN void store_frames(const Params& p, const Tile& t, uint32_t b0, const float* image, uint32_t tid) {
    const uint32_t nb = slab_bins(p, b0);
    const uint32_t K = p.order + 1u, C = p.left + p.right + 1u;
    const bool whole = nb == p.bins;
    const bool merged = whole && p.out_fs == p.cols;
    const uint32_t spf = whole ? 1u : C * K; /* segments of a frame */
    const uint32_t nl = merged ? 1u : t.ng * spf;
    const uint32_t len = merged ? t.ng * p.cols : whole ? p.cols : nb;
    const uint32_t cpl = (len + 3u) / 4u + 1u; /* chunks that cover a line at any offset within its first */
    const uint32_t total = nl * cpl;
    for (uint32_t ch = tid; ch < total; ch += kThreads) {
        const uint32_t l = ch / cpl, q = ch - l * cpl;
        const uint32_t g_line = l / spf, s = l - g_line * spf;
        const uint32_t col0 = whole ? 0u : s * p.bins + b0;
        float* d = t.y + (uint64_t)g_line * p.out_fs + col0;
        const int32_t e0 = (int32_t)(4u * q) - (int32_t)(((uintptr_t)d >> 2) & 3u);
        const uint32_t first = e0 < 0 ? 0u : (uint32_t)e0;
        const uint32_t end = (uint32_t)(e0 + 4) < len ? (uint32_t)(e0 + 4) : len;
        if (first >= end) continue;
        /* where the first element lies: frame, context position, order, bin of the slab */
        uint32_t gl = g_line + (merged ? first / p.cols : 0u);
        const uint32_t j = col0 + (merged ? first - (first / p.cols) * p.cols : first);
        uint32_t c = j / (K * p.bins);
        uint32_t k = (j - c * K * p.bins) / p.bins;
        uint32_t bl = j - (c * K + k) * p.bins - b0;
        F4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t i = 0; i < 4u; i++) {
            if (first + i < end) v[i] = element_of(p, t, image, gl, c, k, bl);
            if (++bl == nb) { /* only a whole line goes on behind its bins */
                bl = 0u;
                if (++k == K) {
                    k = 0u;
                    if (++c == C) {
                        c = 0u;
                        gl++;
                    }
                }
            }
        }
        if (end - first == 4u) *(F4*)(d + first) = v;
        else
            for (uint32_t i = 0; i < 4u; i++)
                if (first + i < end) d[first + i] = v[i];
    }
}

/* Phase 3, bins layout of the output: per column of the slab a run of the tile's ng frames */
ALAC_WF_FN void store_bins(const Params& p, const Tile& t, uint32_t b0, const float* image, uint32_t tid) {
    const uint32_t nb = slab_bins(p, b0);
    const uint32_t K = p.order + 1u, C = p.left + p.right + 1u;
    const uint32_t len = t.ng;
    const uint32_t cpl = (len + 3u) / 4u + 1u;
    const uint32_t total = C * K * nb * cpl;
    for (uint32_t ch = tid; ch < total; ch += kThreads) {
        const uint32_t l = ch / cpl, q = ch - l * cpl;
        const uint32_t ck = l / nb, bl = l - ck * nb;
        const uint32_t c = ck / K, k = ck - c * K;
        float* d = t.y + ((uint64_t)ck * p.bins + b0 + bl) * p.out_bs;
        const int32_t e0 = (int32_t)(4u * q) - (int32_t)(((uintptr_t)d >> 2) & 3u);
        if (e0 >= 0 && (uint32_t)e0 + 4u <= len) {
            F4 v;
            for (uint32_t i = 0; i < 4u; i++) v[i] = element_of(p, t, image, (uint32_t)e0 + i, c, k, bl);
            *(F4*)(d + e0) = v;
        } else {
            for (int32_t i = 0; i < 4; i++)
                if (e0 + i >= 0 && (uint32_t)(e0 + i) < len) d[e0 + i] = element_of(p, t, image, (uint32_t)(e0 + i), c, k, bl);
        }
    }
}

ALAC_WF_FN void store_slab(const Params& p, const Tile& t, uint32_t b0, const float* image, uint32_t tid) {
    if (p.out_bs == 1u) store_frames(p, t, b0, image, tid);
    else store_bins(p, t, b0, image, tid);
}

/* ---- host only ------------------------------------------------------------------------------------------------------ */
/* what create refuses */
inline bool config_ok(const Config& c) {
    if (c.bins < 1u || c.bins > kMaxBins || c.order > kMaxOrder) return false;
    if (c.order > 0u && (c.window < 1u || c.window > kMaxWindow)) return false;
    if (c.left > kMaxContext || c.right > kMaxContext || c.stride < 1u || c.stride > kMaxStride) return false;
    return (uint64_t)(c.left + c.right + 1u) * (c.order + 1u) * c.bins <= kMaxCols;
}

/* The tile of a configuration that config_ok accepts. tile_bins: all bins, halved until the images of one output frame fit;
 * tile_out: the most output frames, up to 64, whose input span's images fit. */
inline Plan plan_of(const Config& c) {
    const uint32_t K = c.order + 1u, C = c.left + c.right + 1u, M = c.order ? c.order * c.window : 0u;
    Plan pl{};
    pl.cols = C * K * c.bins;
    pl.tile_bins = c.bins;
    while (K * pl.tile_bins * ((C + 2u * M) | 1u) > kLdsFloats) pl.tile_bins = (pl.tile_bins + 1u) / 2u;
    pl.tile_out = 1u;
    while (pl.tile_out < kMaxTileOut && K * pl.tile_bins * ((pl.tile_out * c.stride + C + 2u * M) | 1u) <= kLdsFloats) pl.tile_out++;
    pl.tile_in = (pl.tile_out - 1u) * c.stride + C + 2u * M;
    pl.pitch = pl.tile_in | 1u;
    pl.lds_floats = (K * pl.tile_bins * pl.pitch + 3u) & ~3u;
    return pl;
}

/* w_1 and w_2 one behind the other -> the floats of both; counts[k - 1] the taps of w_k, 0 above the order. The numerators are
 * integers below 2^24 and so is the denominator, so the quotient in double lies, relative to its size, no nearer than 2^-49 to
 * a float32 midpoint it does not hit: rounding the double to float32 rounds the exact quotient once. */
inline uint32_t make_weights(uint32_t order, uint32_t window, float* w, uint32_t* counts) {
    int64_t num[3][4 * kMaxWindow + 1] = {{1}};
    int64_t den = 1, norm = 0;
    for (int64_t j = 1; j <= (int64_t)window; j++) norm += 2 * j * j;
    uint32_t at = 0;
    counts[0] = counts[1] = 0u;
    for (uint32_t k = 1; k <= order; k++) {
        const int32_t Mp = (int32_t)((k - 1u) * window), M = (int32_t)(k * window);
        for (int32_t i = 0; i <= 2 * M; i++) num[k][i] = 0;
        for (int32_t i = -Mp; i <= Mp; i++)
            for (int32_t j = -(int32_t)window; j <= (int32_t)window; j++) num[k][i + j + M] += j * num[k - 1u][i + Mp];
        den *= norm;
        for (int32_t i = 0; i <= 2 * M; i++) w[at + (uint32_t)i] = (float)((double)num[k][i] / (double)den);
        counts[k - 1u] = 2u * (uint32_t)M + 1u;
        at += counts[k - 1u];
    }
    return at;
}

inline uint64_t out_frames_of(const Config& c, uint64_t frames) { return frames / c.stride + (frames % c.stride ? 1u : 0u); }

/* the arguments of one pass (rows, frames >= 1); false for what the entry rejects */
inline bool make_params(const Config& c, const Plan& pl, const float* in, uint64_t in_rs, uint64_t in_fs, uint64_t in_bs, uint64_t rows,
                        uint64_t frames, const int32_t* lengths, float* out, uint64_t out_rs, uint64_t out_fs, uint64_t out_bs,
                        int32_t* out_lengths, const float* w, Params* p) {
    if (!in || !out || ((uintptr_t)lengths & 3u) || ((uintptr_t)out_lengths & 3u)) return false;
    if (frames > 0x7fffffffu) return false; /* out_lengths is int32 */
    const uint64_t G = out_frames_of(c, frames);
    Params q{};
    if (!alacfv::strides_of(in, in_rs, in_fs, in_bs, rows, frames, c.bins, &q.in_fs, &q.in_bs) ||
        !alacfv::strides_of(out, out_rs, out_fs, out_bs, rows, G, pl.cols, &q.out_fs, &q.out_bs))
        return false;
    q.in = in;
    q.in_rs = in_rs;
    q.out = out;
    q.out_rs = out_rs;
    /* the two tensors apart */
    const uintptr_t a0 = (uintptr_t)in, a1 = a0 + 4u * alacfv::extent_of(q.in_rs, q.in_fs, q.in_bs, rows, frames, c.bins);
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + 4u * alacfv::extent_of(q.out_rs, q.out_fs, q.out_bs, rows, G, pl.cols);
    if (a0 < b1 && b0 < a1) return false;
    q.lengths = lengths;
    q.out_lengths = out_lengths;
    q.rows = rows;
    q.frames = frames;
    q.out_frames = G;
    q.tiles = (G + pl.tile_out - 1u) / pl.tile_out;
    if (q.tiles > ((uint64_t)1 << 60) / rows) return false;
    q.w = w;
    q.bins = c.bins;
    q.order = c.order;
    q.window = c.order ? c.window : 0u;
    q.left = c.left;
    q.right = c.right;
    q.stride = c.stride;
    q.cols = pl.cols;
    q.tile_bins = pl.tile_bins;
    q.tile_out = pl.tile_out;
    q.tile_in = pl.tile_in;
    q.pitch = pl.pitch;
    q.pad_value = c.pad_value;
    *p = q;
    return true;
}

}  // namespace alacst

#if defined(__HIPCC__)
/* k_stack.hip */
namespace alack {
/* The kernel of one pass on `stream`. */
hipError_t stack_launch(hipStream_t stream, const alacst::Params& p, uint32_t lds_bytes);
}  // namespace alack
#endif
#endif /* ALAC_STACK_H */
