/*
 * alac_featnorm.h — the step behind the feature kernels: float32 features [rows][frames][bins] with per-row lengths ->
 * normalised features with the padding masked, as plain host + device code. k_featnorm.hip builds the gfx950 kernels from this
 * text; tests/host_sim/featnorm_sim.cpp builds the same text with g++ (contraction off) for the CPU suite.
 *
 * Input and output are addressed as alac_featview.h says: three element strides each, one inner stride 1, n_r valid frames in
 * row r. The output may be the input itself (same base, same strides). Per row, in this order:
 *
 *   statistic over the valid frames f < n_r
 *     none      s = x
 *     mean      m_b = S_b / (float)n_r,  s = x - m_b
 *     mean_var  d = x - m_b,  v_b = Q_b / (float)n_r,  rstd_b = 1.0f / sqrtf(v_b < var_floor ? var_floor : v_b),  s = d * rstd_b
 *     max       M = the largest x of all bins and valid frames that is no NaN (+0.0 above -0.0; -inf where there is none),
 *               c = M - range,  s = x < c ? c : x   (fmaxf(x, c) for every x that is no NaN; a NaN stays one)
 *   affine      y = s;  y = y - shift_b where there is a shift;  y = y * scale_b where there is a scale
 *   padding     y = pad_value for f >= n_r; the input there is never used
 *
 * The sums are fixed: S_b and Q_b (of d * d, the product rounded, then added) run over CHUNKS of tile_frames consecutive
 * frames, chunk c = the frames [c * tile_frames, (c + 1) * tile_frames) below n_r: each chunk a chain acc = acc + term in frame
 * order from +0.0f, then total = total + chunk_c for c = 0 .. ceil(n_r / tile_frames) - 1 from +0.0f. The order depends on n_r
 * and tile_frames (a function of bins alone) only: not on rows, the grid or the layout, so both layouts of the same data give
 * the same bits. No operation is contracted (`#pragma clang fp contract(off)`; g++ runs with -ffp-contract=off), there is no
 * float atomic, and the maximum is taken over an integer key of the float, so its order does not matter. stats[r][2][bins]:
 * mean and rstd for mean_var, mean and 1.0 for mean, M in [r][0][0] for max, +0.0 elsewhere and in every row with n_r = 0.
 *
 * A TILE is one chunk of one row, one workgroup of 256. stage_tile brings its valid frames into an image (LDS on the device)
 * with loads along the contiguous axis (alacfv::lines_in). Lanes then take bins and walk the frames out of the image: sum_tile /
 * max_tile for the partial results of a (row, chunk), finish_* for a row's statistics out of the partials, apply_tile for the
 * output, which goes back into the image and from there, along the output's contiguous axis, to memory (store_tile).
 */
#ifndef ALAC_FEATNORM_H
#define ALAC_FEATNORM_H

#include "alac_featview.h"

#include <cmath>
#include <cstring>

namespace alacfn {

using alacfv::kThreads, alacfv::length_of, alacfv::lines_in, alacfv::lines_out;

constexpr uint32_t kNone = 0, kMean = 1, kMeanVar = 2, kMax = 3; /* ALACGPU_NORM_STAT_* */
constexpr uint32_t kSum = 0, kSquares = 1, kLargest = 2;         /* what a partials launch reduces */
constexpr uint32_t kMaxBins = 4096;
constexpr uint32_t kMaxTileFrames = 64;  /* 256 contiguous bytes of a bin in the bins layout */
constexpr uint32_t kLdsFloats = 12800;   /* 51 200 bytes: three workgroups share a CU's 160 KB at the widest tile */
constexpr uint32_t kRed = kThreads;      /* the keys of a maximum, behind the image */

/* frames of a tile: the largest power of two <= 64 whose image (a line pitch of tile_frames | 1 in the bins layout) and keys fit */
ALAC_WF_FN uint32_t tile_frames_of(uint32_t bins) {
    uint32_t tf = kMaxTileFrames;
    while (tf > 1u && bins * (tf | 1u) + kRed > kLdsFloats) tf /= 2u;
    return tf;
}
ALAC_WF_FN uint32_t image_floats_of(uint32_t bins, uint32_t tf) { return (bins * (tf | 1u) + 3u) & ~3u; }
ALAC_WF_FN uint32_t lds_floats_of(uint32_t bins, uint32_t tf) { return image_floats_of(bins, tf) + kRed; }

struct Params {
    const float* in;
    uint64_t in_rs, in_fs, in_bs; /* elements */
    float* out;
    uint64_t out_rs, out_fs, out_bs;
    const int32_t* lengths; /* [rows], may be null */
    uint64_t rows, frames;
    uint64_t chunks; /* ceil(frames / tile_frames) */
    uint32_t bins, tile_frames;
    uint32_t stat, phase; /* phase: kSum / kSquares / kLargest in the partials and finishing kernels */
    float var_floor, range, pad_value;
    const float* shift; /* [bins], may be null */
    const float* scale; /* [bins], may be null */
    float* partial;     /* [rows][chunks][bins], for max [rows][chunks] */
    float* stats;       /* [rows][2][bins] */
};

/* a float as an integer that orders as the float does, +0.0 above -0.0 */
ALAC_WF_FN int32_t key_of(float v) {
    int32_t i;
    memcpy(&i, &v, 4);
    return i ^ ((i >> 31) & 0x7fffffff);
}
ALAC_WF_FN float float_of(int32_t k) {
    const int32_t i = k ^ ((k >> 31) & 0x7fffffff);
    float v;
    memcpy(&v, &i, 4);
    return v;
}
ALAC_WF_FN int32_t lowest_key() { return (int32_t)0x807fffff; /* key_of(-inf) */ }

/* what a tile works on */
struct Tile {
    uint64_t row, chunk;
    uint64_t n;     /* the row's valid frames */
    uint32_t nf;    /* frames of the tile: [chunk * tile_frames, + nf) */
    uint32_t nv;    /* of which valid */
    const float* x; /* the input row's frame chunk * tile_frames, bin 0 */
    float* y;       /* the output's */
    uint32_t lf, lb; /* element (f, b) of the tile is image[f * lf + b * lb] */
};

ALAC_WF_FN Tile make_tile(const Params& p, uint64_t row, uint64_t chunk) {
    Tile t{};
    t.row = row;
    t.chunk = chunk;
    t.n = length_of(p.lengths, p.frames, row);
    const uint64_t f0 = chunk * p.tile_frames;
    t.nf = p.frames - f0 < p.tile_frames ? (uint32_t)(p.frames - f0) : p.tile_frames;
    t.nv = t.n > f0 ? (t.n - f0 < t.nf ? (uint32_t)(t.n - f0) : t.nf) : 0u;
    t.x = p.in + row * p.in_rs + f0 * p.in_fs;
    t.y = p.out + row * p.out_rs + f0 * p.out_fs;
    if (p.in_bs == 1u) { /* frames layout: the image is the frames one behind the other */
        t.lf = p.bins;
        t.lb = 1u;
    } else { /* bins layout: the bins one behind the other, at an odd pitch */
        t.lf = 1u;
        t.lb = p.tile_frames | 1u;
    }
    return t;
}

/* Phase 1: the tile's nv valid frames into the image. Frames that follow each other without a gap are one line. */
ALAC_WF_FN void stage_tile(const Params& p, const Tile& t, float* image, uint32_t tid) {
    if (p.in_bs == 1u) {
        if (p.in_fs == p.bins) lines_in(t.x, 0u, 1u, t.nv * p.bins, image, 0u, 1u, tid);
        else lines_in(t.x, p.in_fs, t.nv, p.bins, image, t.lf, 1u, tid);
    } else {
        lines_in(t.x, p.in_bs, p.bins, t.nv, image, t.lb, 1u, tid);
    }
}

/* Phase 2 of a sum: work item `tid` runs the chains of the bins tid, tid + 256, ... over the tile's valid frames */
ALAC_WF_FN void sum_tile(const Params& p, const Tile& t, const float* image, uint32_t tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float* part = p.partial + (t.row * p.chunks + t.chunk) * p.bins;
    const float* mean = p.stats + t.row * 2u * p.bins;
    for (uint32_t b = tid; b < p.bins; b += kThreads) {
        const float* e = image + b * t.lb;
        float acc = 0.0f;
        if (p.phase == kSum) {
            for (uint32_t f = 0; f < t.nv; f++) acc = acc + e[f * t.lf];
        } else {
            const float m = mean[b];
            for (uint32_t f = 0; f < t.nv; f++) {
                const float d = e[f * t.lf] - m;
                const float q = d * d;
                acc = acc + q;
            }
        }
        part[b] = acc;
    }
}

/* which elements of a tile a work item takes where the frames are independent: bins b0, b0 + bw, ..., frames g, g + groups, ...;
 * groups = 0: none */
struct Share {
    uint32_t b0, bw, g, groups;
};
ALAC_WF_FN Share share_of(uint32_t bins, uint32_t tid) {
    Share s;
    s.bw = bins < kThreads ? bins : kThreads;
    s.groups = kThreads / s.bw;
    s.g = tid / s.bw;
    s.b0 = tid - s.g * s.bw;
    if (s.g >= s.groups) s.groups = 0u;
    return s;
}

/* Phase 2 of a maximum: every work item the key of its share's largest value into red[tid] */
ALAC_WF_FN void max_tile(const Params& p, const Tile& t, const float* image, int32_t* red, uint32_t tid) {
    const Share s = share_of(p.bins, tid);
    int32_t k = lowest_key();
    if (s.groups)
        for (uint32_t b = s.b0; b < p.bins; b += s.bw)
            for (uint32_t f = s.g; f < t.nv; f += s.groups) {
                const float v = image[f * t.lf + b * t.lb];
                const int32_t kv = key_of(v);
                if (v == v && kv > k) k = kv;
            }
    red[tid] = k;
}

/* 256 keys -> 16 (step 0, work items below 16) -> 1 (step 1, work item 0), a barrier in front of each */
ALAC_WF_FN void reduce_keys(int32_t* red, uint32_t step, uint32_t tid) {
    const uint32_t stride = step ? 16u : 1u;
    if (tid >= (step ? 1u : 16u)) return;
    int32_t k = red[tid * 16u * stride];
    for (uint32_t j = 1; j < 16u; j++) {
        const int32_t v = red[(tid * 16u + j) * stride];
        if (v > k) k = v;
    }
    red[tid * 16u * stride] = k;
}

ALAC_WF_FN void put_tile_max(const Params& p, const Tile& t, const int32_t* red, uint32_t tid) {
    if (tid == 0u) p.partial[t.row * p.chunks + t.chunk] = float_of(red[0]);
}

/* the chunks of a row that hold a valid frame */
ALAC_WF_FN uint64_t chunks_of(const Params& p, uint64_t n) { return (n + p.tile_frames - 1u) / p.tile_frames; }

/* A row's mean (phase kSum) or rstd (kSquares) of bin b out of the chunks' partial sums, in chunk order */
ALAC_WF_FN void finish_bin(const Params& p, uint64_t row, uint32_t b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint64_t n = length_of(p.lengths, p.frames, row);
    const uint64_t K = chunks_of(p, n);
    const float* part = p.partial + row * p.chunks * p.bins + b;
    float acc = 0.0f;
    for (uint64_t c = 0; c < K; c++) acc = acc + part[c * p.bins];
    float* st = p.stats + row * 2u * p.bins;
    if (p.phase == kSum) {
        st[b] = n ? acc / (float)n : 0.0f;
        st[p.bins + b] = (n && p.stat == kMean) ? 1.0f : 0.0f;
    } else if (n) {
        float v = acc / (float)n;
        if (v < p.var_floor) v = p.var_floor;
        st[p.bins + b] = 1.0f / sqrtf(v);
    }
}

/* A row's maximum: every work item the largest of the chunks tid, tid + 256, ... into red[tid]; then reduce_keys twice; then
 * put_row_max */
ALAC_WF_FN void row_max(const Params& p, uint64_t row, int32_t* red, uint32_t tid) {
    const uint64_t K = chunks_of(p, length_of(p.lengths, p.frames, row));
    const float* part = p.partial + row * p.chunks;
    int32_t k = lowest_key();
    for (uint64_t c = tid; c < K; c += kThreads) {
        const int32_t kv = key_of(part[c]);
        if (kv > k) k = kv;
    }
    red[tid] = k;
}
ALAC_WF_FN void put_row_max(const Params& p, uint64_t row, const int32_t* red, uint32_t tid) {
    const uint64_t n = length_of(p.lengths, p.frames, row);
    float* st = p.stats + row * 2u * p.bins;
    for (uint32_t i = tid; i < 2u * p.bins; i += kThreads) st[i] = (i == 0u && n) ? float_of(red[0]) : 0.0f;
}

/* Phase 2 of the output: the tile's elements, the padding included, in place in the image */
ALAC_WF_FN void apply_tile(const Params& p, const Tile& t, float* image, uint32_t tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const Share s = share_of(p.bins, tid);
    if (!s.groups) return;
    const float* st = p.stats + t.row * 2u * p.bins;
    const float floor_ = (p.stat == kMax && t.nv) ? st[0] - p.range : 0.0f;
    for (uint32_t b = s.b0; b < p.bins; b += s.bw) {
        float* e = image + b * t.lb;
        const float m = (t.nv && (p.stat == kMean || p.stat == kMeanVar)) ? st[b] : 0.0f;
        const float r = (t.nv && p.stat == kMeanVar) ? st[p.bins + b] : 1.0f;
        const float sh = p.shift ? p.shift[b] : 0.0f;
        const float sc = p.scale ? p.scale[b] : 1.0f;
        for (uint32_t f = s.g; f < t.nf; f += s.groups) {
            float y = p.pad_value;
            if (f < t.nv) {
                y = e[f * t.lf];
                if (p.stat == kMean) y = y - m;
                else if (p.stat == kMeanVar) y = (y - m) * r;
                else if (p.stat == kMax) y = y < floor_ ? floor_ : y;
                if (p.shift) y = y - sh;
                if (p.scale) y = y * sc;
            }
            e[f * t.lf] = y;
        }
    }
}

/* Phase 3: the image's nf frames to the output, along its contiguous axis */
ALAC_WF_FN void store_tile(const Params& p, const Tile& t, const float* image, uint32_t tid) {
    if (p.out_bs == 1u) {
        if (p.out_fs == p.bins && t.lb == 1u) lines_out(t.y, 0u, 1u, t.nf * p.bins, image, 0u, 1u, tid);
        else lines_out(t.y, p.out_fs, t.nf, p.bins, image, t.lf, t.lb, tid);
    } else {
        lines_out(t.y, p.out_bs, p.bins, t.nf, image, t.lb, t.lf, tid);
    }
}

/* ---- host only ------------------------------------------------------------------------------------------------------ */
struct Config {
    uint32_t bins, stat;
    float var_floor, range, pad_value;
};

/* what create refuses */
inline bool config_ok(const Config& c) {
    if (c.bins < 1u || c.bins > kMaxBins || c.stat > kMax) return false;
    if (!(c.var_floor > 0.0f)) return false;
    if (c.stat == kMax && !(c.range >= 0.0f)) return false;
    return true;
}

/* floats of scratch a pass needs behind the caller's buffers: the partials, and the stats where the caller keeps none */
inline bool scratch_floats_of(const Config& c, uint64_t rows, uint64_t frames, bool own_stats, uint64_t* floats) {
    const uint32_t tf = tile_frames_of(c.bins);
    const uint64_t chunks = (frames + tf - 1u) / tf;
    const uint64_t lim = (uint64_t)1 << 60;
    if (chunks > lim / rows) return false;
    uint64_t part = 0;
    if (c.stat == kMax) part = rows * chunks;
    else if (c.stat != kNone) {
        if (rows * chunks > lim / c.bins) return false;
        part = rows * chunks * c.bins;
    }
    uint64_t st = 0;
    if (own_stats && c.stat != kNone) {
        if (rows > lim / (2u * c.bins)) return false;
        st = rows * 2u * c.bins;
    }
    *floats = ((part + 3u) & ~(uint64_t)3) + st;
    return true;
}

/* the arguments of one pass (rows, frames >= 1) but for the scratch block (set_scratch); false for what the entry rejects */
inline bool make_params(const Config& c, const float* in, uint64_t in_rs, uint64_t in_fs, uint64_t in_bs, uint64_t rows,
                        uint64_t frames, const int32_t* lengths, float* out, uint64_t out_rs, uint64_t out_fs, uint64_t out_bs,
                        float* stats, const float* shift, const float* scale, Params* p) {
    if (!in || !out || ((uintptr_t)lengths & 3u) || ((uintptr_t)stats & 3u)) return false;
    Params q{};
    if (!alacfv::strides_of(in, in_rs, in_fs, in_bs, rows, frames, c.bins, &q.in_fs, &q.in_bs) ||
        !alacfv::strides_of(out, out_rs, out_fs, out_bs, rows, frames, c.bins, &q.out_fs, &q.out_bs))
        return false;
    uint64_t floats;
    if (!scratch_floats_of(c, rows, frames, stats == nullptr, &floats)) return false;
    q.in = in;
    q.in_rs = in_rs;
    q.out = out;
    q.out_rs = out_rs;
    q.lengths = lengths;
    q.rows = rows;
    q.frames = frames;
    q.bins = c.bins;
    q.tile_frames = tile_frames_of(c.bins);
    q.chunks = (frames + q.tile_frames - 1u) / q.tile_frames;
    q.stat = c.stat;
    q.phase = kSum;
    q.var_floor = c.var_floor;
    q.range = c.range;
    q.pad_value = c.pad_value;
    q.shift = shift;
    q.scale = scale;
    q.partial = nullptr;
    q.stats = stats;
    *p = q;
    return true;
}

/* scratch: scratch_floats_of floats (never NULL): the partials, then the stats where the caller keeps none */
inline void set_scratch(Params* p, float* scratch) {
    p->partial = scratch;
    const uint64_t part = p->stat == kMax ? p->rows * p->chunks : p->stat != kNone ? p->rows * p->chunks * p->bins : 0u;
    if (!p->stats) p->stats = scratch + ((part + 3u) & ~(uint64_t)3);
}

/* the launches of one pass in order: (kernel, phase) with kernel 0 = partials over (row, chunk), 1 = finishing over rows x
 * blocks of 256 bins (one block per row for a maximum), 2 = apply over (row, chunk) */
template <typename F>
inline void for_each_launch(uint32_t stat, F&& launch) {
    if (stat == kMean || stat == kMeanVar) {
        launch(0u, kSum);
        launch(1u, kSum);
    }
    if (stat == kMeanVar) {
        launch(0u, kSquares);
        launch(1u, kSquares);
    }
    if (stat == kMax) {
        launch(0u, kLargest);
        launch(1u, kLargest);
    }
    launch(2u, kSum);
}

}  // namespace alacfn

#if defined(__HIPCC__)
/* k_featnorm.hip */
namespace alack {
/* All kernels of one pass on `stream`. */
hipError_t featnorm_launch(hipStream_t stream, const alacfn::Params& p, uint32_t lds_bytes);
}  // namespace alack
#endif
#endif /* ALAC_FEATNORM_H */
