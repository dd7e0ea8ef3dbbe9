/*
 * alac_specaug.h — the training step between the normalisation and the stacking: SpecAugment over float32 features [rows][frames]
 * [bins] with per-row lengths: a time warp, frequency masks and time masks drawn inside each row's own n_r frames, as plain host
 * + device code. k_specaug.hip builds the gfx950 kernel from this text; tests/host_sim/specaug_sim.cpp builds the same text with
 * g++ (contraction off) for the CPU suite.
 *
 * Input and output are addressed as alac_featview.h says: three element strides each, one inner stride 1, n_r valid frames in
 * row r. The output has the input's shape, strides of its own and either layout.
 *
 * Parameters, fixed at create: bins 1..4096, freq_masks (nf) 0..8, freq_width (Fw) 0..bins, time_masks (nt) 0..16, time_width (Tw)
 * 0..65535, time_ratio_q16 (q) 0..65536, warp (W) 0..256, mask_value and pad_value any float. Per call: seed, row_base, ids.
 *
 * Random words: Philox4x32-10 (Random123's constants), key (seed low, seed high). Row r's identity is id = ids ? ids[r] :
 * row_base + r; its word j is output word j % 4 of the block at counter (id low, id high, j / 4, 0). A draw from [0, m) is
 * mulhi32(word, m). A row consumes P = 2 + 2 nf + 2 nt words whatever n_r is:
 *   words 0, 1             the warp: where W > 0 and n_r > 2 W, c = W + draw(n_r - 2 W) and w = c - W + 1 + draw(2 W); else c = w = 0
 *   words 2 + 2 i, 3 + 2 i  frequency mask i: fw = draw(Fw + 1), f0 = draw(bins - fw + 1): bins [f0, f0 + fw)
 *   the 2 nt behind them   time mask i: cap = min(Tw, (n_r * q) >> 16), tw = draw(cap + 1), t0 = draw(n_r - tw + 1): frames [t0, t0 + tw)
 * The resolved draws of a row are P int32: c, w, then (start, width) per mask in word order.
 *
 * Warp: output frames [0, w) are the source frames [0, c) resampled linearly, output frames [w, n_r) the source frames [c, n_r),
 * each segment on its own. Output frame t of a segment of a source frames and b output frames: num = (2 t + 1) a - b; num <= 0:
 * i0 = 0, lq = 0; else i0 = num / (2 b), lq = ((num % (2 b)) << 23) / (2 b) in uint64; i1 = min(i0 + 1, a - 1). Where lq == 0 or
 * i1 == i0 the element x[i0] is copied and never multiplied; else y = fmaf((float)lq * 0x1p-23f, x[i1] - x[i0], x[i0]). With
 * c = w = 0 every element is a copy. Then the masks, in output coordinates: an element under any mask is mask_value. Every frame
 * f >= n_r is pad_value, and its input is never read.
 *
 * A TILE is tile_out consecutive output frames of one row, one workgroup of 256: resolve_draws (the first P / 2 work items, one
 * Philox block per two of them) puts the row's draws into LDS; frame_plan (the first tile_out work items) each frame's (i0, i1,
 * lq) or its kind (masked, padding), with the 64-bit divisions once per frame, and bin_plan the masked bins as bits; build_image
 * the tile of y in an LDS image by reading along the input's contiguous axis straight from global memory (two source lines per
 * output frame in the frames layout, neighbouring source frames per bin in the bins layout), masks and padding applied as it is
 * written; lines_out stores it along the output's contiguous axis. tile_out and the LDS size are functions of bins alone. All
 * index arithmetic that leaves a tile is in 64 bits; there is no atomic; no operation is contracted.
 */
#ifndef ALAC_SPECAUG_H
#define ALAC_SPECAUG_H

#include "alac_featview.h"

#include <cmath>

namespace alacsa {

using alacfv::F4, alacfv::kThreads, alacfv::length_of, alacfv::lines_out;

constexpr uint32_t kMaxBins = 4096, kMaxFreqMasks = 8, kMaxTimeMasks = 16, kMaxTimeWidth = 65535, kMaxRatioQ16 = 65536, kMaxWarp = 256;
constexpr uint32_t kMaxTileOut = 64;    /* 256 contiguous bytes of a bin's line in the bins layout */
constexpr uint32_t kImageFloats = 6016; /* with the plans behind it at most 25 600 bytes: six workgroups share a CU's 160 KB */
constexpr uint32_t kMaxDraws = 2u + 2u * kMaxFreqMasks + 2u * kMaxTimeMasks;
constexpr uint32_t kDrawSlots = (kMaxDraws + 3u) & ~3u;
constexpr uint32_t kMasked = 0xFFFFFFFFu, kPadding = 0xFFFFFFFEu; /* a frame's kind where its lq would stand (lq < 2^23) */

struct Config {
    uint32_t bins, freq_masks, freq_width, time_masks, time_width, time_ratio_q16, warp;
    float mask_value, pad_value;
};

struct Plan {
    uint32_t draws;    /* P */
    uint32_t tile_out; /* output frames of a tile */
    uint32_t pitch;    /* tile_out | 1: a bin's line of the image in the bins layout */
    uint32_t image;    /* 4-byte words of the image, a multiple of 4 */
    uint32_t lds_words;
};

struct Params {
    const float* in;
    uint64_t in_rs, in_fs, in_bs; /* elements */
    float* out;
    uint64_t out_rs, out_fs, out_bs;
    const int32_t* lengths; /* [rows], may be null */
    const int64_t* ids;     /* [rows], may be null */
    int32_t* draws_out;     /* [rows][P], may be null */
    uint64_t rows, frames;
    uint64_t tiles; /* of a row: ceil(frames / tile_out) */
    uint64_t seed, row_base;
    uint32_t bins, freq_masks, freq_width, time_masks, time_width, time_ratio_q16, warp;
    uint32_t draws, tile_out, pitch, image;
    float mask_value, pad_value;
};

/* what a tile works on */
struct Tile {
    uint64_t row, n; /* the row's valid frames */
    uint64_t id;     /* the row's identity */
    uint64_t t0;     /* the tile's first frame */
    uint32_t ng;     /* its frames */
    uint32_t lf, lb; /* element (t0 + fl, b) of the tile is image[fl * lf + b * lb] */
    const float* x;  /* the input row's frame 0, bin 0 */
    float* y;        /* the output row's frame t0, bin 0 */
};

/* the LDS block behind the image: three words per frame, the row's draws, the masked bins as bits */
struct Lds {
    float* image;
    uint32_t *i0, *i1, *lq;
    int32_t* draws;
    uint32_t* binmask;
};

ALAC_WF_FN Lds carve(const Params& p, float* lds) {
    Lds l;
    l.image = lds;
    l.i0 = (uint32_t*)(lds + p.image);
    l.i1 = l.i0 + p.tile_out;
    l.lq = l.i1 + p.tile_out;
    l.draws = (int32_t*)(l.lq + p.tile_out);
    l.binmask = (uint32_t*)(l.draws + kDrawSlots);
    return l;
}

ALAC_WF_FN Tile make_tile(const Params& p, uint64_t row, uint64_t tile) {
    Tile t{};
    t.row = row;
    t.n = length_of(p.lengths, p.frames, row);
    t.id = p.ids ? (uint64_t)p.ids[row] : p.row_base + row;
    t.t0 = tile * p.tile_out;
    t.ng = p.frames - t.t0 < p.tile_out ? (uint32_t)(p.frames - t.t0) : p.tile_out;
    if (p.in_bs == 1u) { /* frames layout: the image is the frames one behind the other */
        t.lf = p.bins;
        t.lb = 1u;
    } else { /* bins layout: the bins one behind the other, at an odd pitch */
        t.lf = 1u;
        t.lb = p.pitch;
    }
    t.x = p.in + row * p.in_rs;
    t.y = p.out + row * p.out_rs + t.t0 * p.out_fs;
    return t;
}

ALAC_WF_FN uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

/* Philox4x32-10: counter c[4] and key (k0, k1) -> the block in c */
ALAC_WF_FN void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (uint32_t round = 0; round < 10u; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (uint32_t)p1;
        c[2] = n2;
        c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

/* Phase 1, work item k < P / 2: the pair of words 2 k, 2 k + 1 of the row (they lie in one block) resolved into draws[2 k],
 * draws[2 k + 1]: pair 0 the warp's (c, w), the others a mask's (start, width) */
ALAC_WF_FN void resolve_draws(const Params& p, const Tile& t, int32_t* draws, uint32_t k) {
    if (2u * k >= p.draws) return;
    uint32_t c[4] = {(uint32_t)t.id, (uint32_t)(t.id >> 32), k / 2u, 0u};
    philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
    const uint32_t wa = c[2u * (k & 1u)], wb = c[2u * (k & 1u) + 1u];
    const uint32_t n = (uint32_t)t.n; /* at most 2^31 - 1 */
    uint32_t first = 0u, second = 0u;
    if (k == 0u) {
        if (p.warp > 0u && n > 2u * p.warp) {
            first = p.warp + mulhi32(wa, n - 2u * p.warp);                /* c */
            second = first - p.warp + 1u + mulhi32(wb, 2u * p.warp);     /* w */
        }
    } else if (k <= p.freq_masks) {
        second = mulhi32(wa, p.freq_width + 1u);     /* fw */
        first = mulhi32(wb, p.bins - second + 1u);   /* f0 */
    } else {
        const uint64_t share = ((uint64_t)n * p.time_ratio_q16) >> 16;
        const uint32_t cap = share < p.time_width ? (uint32_t)share : p.time_width;
        second = mulhi32(wa, cap + 1u);       /* tw */
        first = mulhi32(wb, n - second + 1u); /* t0 */
    }
    draws[2u * k] = (int32_t)first;
    draws[2u * k + 1u] = (int32_t)second;
}

/* Phase 2, work item fl < ng: frame t0 + fl's source frames and weight, or its kind. Tile 0's first P work items store the
 * row's draws. */
ALAC_WF_FN void frame_plan(const Params& p, const Tile& t, const Lds& l, uint32_t fl) {
    if (t.t0 == 0u && p.draws_out && fl < p.draws) p.draws_out[t.row * p.draws + fl] = l.draws[fl];
    if (fl >= t.ng) return;
    const uint64_t f = t.t0 + fl;
    if (f >= t.n) {
        l.lq[fl] = kPadding;
        return;
    }
    const int32_t* tm = l.draws + 2u + 2u * p.freq_masks;
    for (uint32_t i = 0; i < p.time_masks; i++) {
        const uint64_t s = (uint64_t)(uint32_t)tm[2u * i];
        if (f >= s && f < s + (uint32_t)tm[2u * i + 1u]) {
            l.lq[fl] = kMasked;
            return;
        }
    }
    const uint64_t c = (uint32_t)l.draws[0], w = (uint32_t)l.draws[1];
    if (w == 0u) { /* no warp in this row: the frame itself */
        l.i0[fl] = l.i1[fl] = (uint32_t)f;
        l.lq[fl] = 0u;
        return;
    }
    const bool head = f < w;
    const uint64_t a = head ? c : t.n - c, b = head ? w : t.n - w, ts = head ? f : f - w, base = head ? 0u : c;
    const uint64_t twice = (2u * ts + 1u) * a;
    uint64_t i0 = 0u, lq = 0u;
    if (twice > b) {
        const uint64_t num = twice - b;
        i0 = num / (2u * b);
        lq = ((num % (2u * b)) << 23) / (2u * b);
    }
    const uint64_t i1 = i0 + 1u < a ? i0 + 1u : a - 1u;
    l.i0[fl] = (uint32_t)(base + i0);
    l.i1[fl] = (uint32_t)(base + i1);
    l.lq[fl] = i1 == i0 ? 0u : (uint32_t)lq;
}

/* Phase 2 too: the bins under a frequency mask as bits, 32 bins per word */
ALAC_WF_FN void bin_plan(const Params& p, const Lds& l, uint32_t tid) {
    const uint32_t words = (p.bins + 31u) / 32u;
    for (uint32_t wd = tid; wd < words; wd += kThreads) {
        uint32_t bits = 0u;
        for (uint32_t i = 0; i < p.freq_masks; i++) {
            const uint32_t f0 = (uint32_t)l.draws[2u + 2u * i], f1 = f0 + (uint32_t)l.draws[3u + 2u * i];
            const uint32_t lo = f0 > 32u * wd ? f0 - 32u * wd : 0u, hi = f1 > 32u * wd ? (f1 - 32u * wd < 32u ? f1 - 32u * wd : 32u) : 0u;
            if (lo < hi) bits |= (hi == 32u ? 0xFFFFFFFFu : (1u << hi) - 1u) & ~((1u << lo) - 1u);
        }
        l.binmask[wd] = bits;
    }
}

ALAC_WF_FN bool bin_masked(const Lds& l, uint32_t b) { return (l.binmask[b >> 5] >> (b & 31u)) & 1u; }

/* one element of y out of its two sources; the weight 0 copies */
ALAC_WF_FN float blend(float x0, float x1, uint32_t lq) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return fmaf((float)lq * 0x1p-23f, x1 - x0, x0);
}

/* Phase 3, frames layout of the input: per frame of the tile the line of source frame i0 and, where its weight is not zero, the
 * line of i1, 16 bytes at a time in the absolute 16-byte chunks of the first, elements at the ends; masked and padding frames
 * read nothing */
ALAC_WF_FN void build_frames(const Params& p, const Tile& t, const Lds& l, uint32_t tid) {
    const uint32_t len = p.bins;
    const uint32_t cpl = (len + 3u) / 4u + 1u; /* chunks that cover a line at any offset within its first */
    const uint32_t total = t.ng * cpl;
    for (uint32_t ch = tid; ch < total; ch += kThreads) {
        const uint32_t fl = ch / cpl, q = ch - fl * cpl;
        const uint32_t lq = l.lq[fl];
        float* d = l.image + fl * t.lf;
        const bool flat = lq >= kPadding;
        const float* s0 = flat ? t.x : t.x + (uint64_t)l.i0[fl] * p.in_fs;
        const float* s1 = flat ? t.x : t.x + (uint64_t)l.i1[fl] * p.in_fs;
        const int32_t e0 = (int32_t)(4u * q) - (int32_t)(((uintptr_t)s0 >> 2) & 3u); /* slot j of the chunk is bin e0 + j */
        if (e0 >= (int32_t)len) continue;
        const bool whole = e0 >= 0 && (uint32_t)e0 + 4u <= len;
        F4 a = {0.0f, 0.0f, 0.0f, 0.0f}, c = a;
        if (flat) {
            const float v = lq == kPadding ? p.pad_value : p.mask_value;
            a = F4{v, v, v, v};
        } else {
            if (whole) a = *(const F4*)(s0 + e0);
            else
                for (int32_t j = 0; j < 4; j++)
                    if (e0 + j >= 0 && (uint32_t)(e0 + j) < len) a[j] = s0[e0 + j];
            if (lq != 0u) {
                if (whole && ((uintptr_t)(s1 + e0) & 15u) == 0u) c = *(const F4*)(s1 + e0);
                else
                    for (int32_t j = 0; j < 4; j++)
                        if (e0 + j >= 0 && (uint32_t)(e0 + j) < len) c[j] = s1[e0 + j];
                for (int32_t j = 0; j < 4; j++) a[j] = blend(a[j], c[j], lq);
            }
        }
        for (int32_t j = 0; j < 4; j++)
            if (e0 + j >= 0 && (uint32_t)(e0 + j) < len)
                d[e0 + j] = !flat && bin_masked(l, (uint32_t)(e0 + j)) ? p.mask_value : a[j];
    }
}

/* Phase 3, bins layout of the input: per bin the tile's frames one behind the other, each out of the bin's source frames i0 and
 * i1: neighbouring work items read neighbouring frames of one bin's line. A row without a warp reads its lines as lines_in does. */
ALAC_WF_FN void build_bins(const Params& p, const Tile& t, const Lds& l, uint32_t tid) {
    if (l.draws[1] == 0) { /* no warp in this row: the tile's own valid frames of a bin are one line, 16 bytes at a time */
        const uint32_t nv = t.n > t.t0 ? (t.n - t.t0 < t.ng ? (uint32_t)(t.n - t.t0) : t.ng) : 0u;
        const uint32_t cpl = (t.ng + 3u) / 4u + 1u;
        const uint32_t total = p.bins * cpl;
        for (uint32_t ch = tid; ch < total; ch += kThreads) {
            const uint32_t b = ch / cpl, q = ch - b * cpl;
            const float* s = t.x + (uint64_t)b * p.in_bs + t.t0;
            const int32_t e0 = (int32_t)(4u * q) - (int32_t)(((uintptr_t)s >> 2) & 3u); /* slot j of the chunk is frame t0 + e0 + j */
            if (e0 >= (int32_t)t.ng) continue;
            F4 a = {0.0f, 0.0f, 0.0f, 0.0f};
            if (e0 >= 0 && (uint32_t)e0 + 4u <= nv) a = *(const F4*)(s + e0);
            else
                for (int32_t j = 0; j < 4; j++)
                    if (e0 + j >= 0 && (uint32_t)(e0 + j) < nv) a[j] = s[e0 + j];
            const bool under = bin_masked(l, b);
            for (int32_t j = 0; j < 4; j++)
                if (e0 + j >= 0 && (uint32_t)(e0 + j) < t.ng) {
                    const uint32_t lq = l.lq[e0 + j];
                    l.image[(uint32_t)(e0 + j) * t.lf + b * t.lb] = lq == kPadding ? p.pad_value : lq == kMasked || under ? p.mask_value : a[j];
                }
        }
        return;
    }
    const uint32_t total = p.bins * t.ng;
    for (uint32_t e = tid; e < total; e += kThreads) {
        const uint32_t b = e / t.ng, fl = e - b * t.ng;
        const uint32_t lq = l.lq[fl];
        float v;
        if (lq >= kPadding) v = lq == kPadding ? p.pad_value : p.mask_value;
        else if (bin_masked(l, b)) v = p.mask_value;
        else {
            const float* s = t.x + (uint64_t)b * p.in_bs;
            const float x0 = s[l.i0[fl]];
            v = lq == 0u ? x0 : blend(x0, s[l.i1[fl]], lq);
        }
        l.image[fl * t.lf + b * t.lb] = v;
    }
}

ALAC_WF_FN void build_image(const Params& p, const Tile& t, const Lds& l, uint32_t tid) {
    if (p.in_bs == 1u) build_frames(p, t, l, tid);
    else build_bins(p, t, l, tid);
}

/* Phase 4: the image along the output's contiguous axis: the tile's lines of bins floats, or per bin a run of its frames */
ALAC_WF_FN void store_image(const Params& p, const Tile& t, const Lds& l, uint32_t tid) {
    if (p.out_bs == 1u) lines_out(t.y, p.out_fs, t.ng, p.bins, l.image, t.lf, t.lb, tid);
    else lines_out(t.y, p.out_bs, p.bins, t.ng, l.image, t.lb, t.lf, tid);
}

/* ---- host only ------------------------------------------------------------------------------------------------------ */
/* what create refuses */
inline bool config_ok(const Config& c) {
    return c.bins >= 1u && c.bins <= kMaxBins && c.freq_masks <= kMaxFreqMasks && c.freq_width <= c.bins && c.time_masks <= kMaxTimeMasks &&
           c.time_width <= kMaxTimeWidth && c.time_ratio_q16 <= kMaxRatioQ16 && c.warp <= kMaxWarp;
}

/* the most frames, up to 64, whose image fits: a function of bins alone */
inline uint32_t tile_out_of(uint32_t bins) {
    uint32_t T = kMaxTileOut;
    while (T > 1u && bins * (T | 1u) > kImageFloats) T--;
    return T;
}

/* The tile of a configuration that config_ok accepts */
inline Plan plan_of(const Config& c) {
    Plan pl{};
    pl.draws = 2u + 2u * c.freq_masks + 2u * c.time_masks;
    pl.tile_out = tile_out_of(c.bins);
    pl.pitch = pl.tile_out | 1u;
    pl.image = (c.bins * pl.pitch + 3u) & ~3u;
    pl.lds_words = (pl.image + 3u * pl.tile_out + kDrawSlots + (c.bins + 31u) / 32u + 3u) & ~3u;
    return pl;
}

/* the arguments of one pass (rows, frames >= 1); false for what the entry rejects */
inline bool make_params(const Config& c, const Plan& pl, const float* in, uint64_t in_rs, uint64_t in_fs, uint64_t in_bs, uint64_t rows,
                        uint64_t frames, const int32_t* lengths, uint64_t seed, uint64_t row_base, const int64_t* ids, float* out,
                        uint64_t out_rs, uint64_t out_fs, uint64_t out_bs, int32_t* draws_out, Params* p) {
    if (!in || !out || ((uintptr_t)lengths & 3u) || ((uintptr_t)ids & 7u) || ((uintptr_t)draws_out & 3u)) return false;
    if (frames > 0x7fffffffu) return false; /* the draws are int32 */
    Params q{};
    if (!alacfv::strides_of(in, in_rs, in_fs, in_bs, rows, frames, c.bins, &q.in_fs, &q.in_bs) ||
        !alacfv::strides_of(out, out_rs, out_fs, out_bs, rows, frames, c.bins, &q.out_fs, &q.out_bs))
        return false;
    q.in = in;
    q.in_rs = in_rs;
    q.out = out;
    q.out_rs = out_rs;
    /* the two tensors apart, or one and the same without a warp: a tile then reads its own frames only, before it writes them */
    const bool same = in == out && in_rs == out_rs && q.in_fs == q.out_fs && q.in_bs == q.out_bs;
    if (!(same && c.warp == 0u)) {
        const uintptr_t a0 = (uintptr_t)in, a1 = a0 + 4u * alacfv::extent_of(q.in_rs, q.in_fs, q.in_bs, rows, frames, c.bins);
        const uintptr_t b0 = (uintptr_t)out, b1 = b0 + 4u * alacfv::extent_of(q.out_rs, q.out_fs, q.out_bs, rows, frames, c.bins);
        if (a0 < b1 && b0 < a1) return false;
    }
    q.lengths = lengths;
    q.ids = ids;
    q.draws_out = draws_out;
    q.rows = rows;
    q.frames = frames;
    q.tiles = (frames + pl.tile_out - 1u) / pl.tile_out;
    if (q.tiles > ((uint64_t)1 << 60) / rows) return false;
    q.seed = seed;
    q.row_base = row_base;
    q.bins = c.bins;
    q.freq_masks = c.freq_masks;
    q.freq_width = c.freq_width;
    q.time_masks = c.time_masks;
    q.time_width = c.time_width;
    q.time_ratio_q16 = c.time_ratio_q16;
    q.warp = c.warp;
    q.draws = pl.draws;
    q.tile_out = pl.tile_out;
    q.pitch = pl.pitch;
    q.image = pl.image;
    q.mask_value = c.mask_value;
    q.pad_value = c.pad_value;
    *p = q;
    return true;
}

}  // namespace alacsa

#if defined(__HIPCC__)
/* k_specaug.hip */
namespace alack {
/* The kernel of one pass on `stream`. */
hipError_t specaug_launch(hipStream_t stream, const alacsa::Params& p, uint32_t lds_bytes);
}  // namespace alack
#endif
#endif /* ALAC_SPECAUG_H */
