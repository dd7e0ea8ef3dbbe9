/*
 * alac_waveaug.h — the training step between the clips and the features: a gain, noise from a bank at an SNR and dither over float32
 * waveforms [rows][T] with per-row lengths, as plain host + device code. k_waveaug.hip builds the gfx950 kernels from this text;
 * tests/host_sim/waveaug_sim.cpp builds the same text with g++ (contraction off) for the CPU suite.
 *
 * Input x[r][t] at in + r * in_rs + t, n_r = clamp(lengths[r], 0, T) valid samples (T without lengths); the output y has the same
 * shape, a row stride of its own, and may be the input itself. The bank z[k][u] at z + k * z_rs + u, N clips of m_k =
 * clamp(noise_lengths[k], 0, Tn) samples (Tn without noise_lengths); N = 0 or no bank: no noise.
 *
 * Parameters, fixed at create: snr_lo_q8 <= snr_hi_q8 and gain_lo_q8 <= gain_hi_q8 in 1 / 256 dB, each within +-64 * 256 and no
 * more than 64 * 256 apart; noise_prob_q16 0..65536; dither finite and >= 0; clamp 0 / 1; pad_value. The plan holds two tables,
 * computed in double and rounded once: snr_amp[i] = 10^(-(snr_lo_q8 + i) / 5120), gain_amp[i] = 10^((gain_lo_q8 + i) / 5120). The
 * device never calls pow.
 *
 * Random words: Philox4x32-10 as alac_specaug.h's, key (seed low, seed high), id = ids ? ids[r] : row_base + r. The fourth counter
 * word is a stream number (SpecAugment is stream 0). The row's word j is output word j % 4 of the block at (id low, id high, j / 4,
 * 2); the dither of sample t is the block at (id low, id high, t, 3). A row consumes 5 words whatever n_r and N are:
 *   word 0  applied = N > 0 && mulhi32(w, 65536) < noise_prob_q16
 *   word 1  k = draw(N)
 *   word 2  o = draw(m_k); m_k == 0: applied = 0; N == 0 or m_k == 0: k = o = 0
 *   word 3  snr_i = draw(snr_hi_q8 - snr_lo_q8 + 1)
 *   word 4  gain_i = draw(gain_hi_q8 - gain_lo_q8 + 1)
 * The noise under sample t is z_t = z[k][(o + t) mod m_k]. The resolved draws are 5 int32: applied, k, o, snr_lo_q8 + snr_i,
 * gain_lo_q8 + gain_i.
 *
 * Energies Ex = sum x_t^2 and En = sum z_t^2 over t < n_r, in one order that is a function of n_r alone: CHUNKS of `tile` (4096)
 * samples on the row's own index t; in a chunk, lane l of 256 chains acc = fmaf(v, v, acc) from +0.0f over the chunk's samples
 * of index = l mod 256, in increasing order; acc[l] += acc[l + s] for s = 128, 64 .. 1; the chunks' sums are added in chunk order
 * from +0.0f. a = gain_amp[gain_i]; b = (sqrtf(Ex / En) * snr_amp[snr_i]) * a where applied, Ex > 0, En > 0 and both finite, else 0.
 * Stats per row: Ex, En (0 without noise), a, b.
 *
 * Output for t < n_r: v = a * x_t; where b != 0: v = fmaf(b, z_t, v); where dither != 0: v = fmaf(dither, g_t, v); clamp: v =
 * v < -1 ? -1 : v > 1 ? 1 : v (a NaN stays one). Every t >= n_r is pad_value; nothing at t >= n_r or behind m_k is read, and a row
 * with b == 0 never reads the bank. g_t: the block's eight 16-bit halves h0..h7 (low half of word 0 first), s = (h0 + h1 + h2 + h3)
 * - (h4 + h5 + h6 + h7), g = (float)s * kDitherScale: zero mean, unit variance, |g| < 4.9.
 *
 * Three kernels. PARTIALS, one workgroup of 256 per (row, chunk in front of n_r): the chunk of x into LDS 16 bytes at a time in the
 * chunks of the absolute address space, its sum; where applied the wrapped noise segment into the same LDS, its sum. FINISH, one
 * workgroup per row: the partials in chunk order, a and b, the stats and the draws. APPLY, one workgroup per (row, chunk): the
 * noise segment into LDS where b != 0, then the output's line 16 bytes at a time. The position (o + t0) mod m_k is divided once
 * per chunk; a clip shorter than the chunk costs one division per work item. All indices that leave a chunk are 64-bit; there is
 * no atomic; nothing is contracted.
 */
#ifndef ALAC_WAVEAUG_H
#define ALAC_WAVEAUG_H

#include "alac_specaug.h"

#include <vector>

namespace alacwa {

using alacfv::F4, alacfv::kThreads, alacfv::length_of, alacfv::lines_in;
using alacsa::mulhi32, alacsa::philox4x32_10;

constexpr uint32_t kTile = 4096;                 /* samples of a chunk: 16 per work item */
constexpr uint32_t kDraws = 5, kStats = 4;       /* int32 and floats per row */
constexpr uint32_t kRowStream = 2, kDitherStream = 3;
constexpr int32_t kMaxQ8 = 64 * 256;             /* +-64 dB, and the widest span of a range */
constexpr uint32_t kMaxProbQ16 = 65536;
constexpr float kDitherScale = 0x1.3988e2p-16f;  /* the float nearest 1 / sqrt((2^32 - 1) * 2 / 3) */
constexpr uint32_t kSideFloats = 2u * kThreads + 12u; /* the two sums' lanes, the row's words, the finish kernel's two sums */
constexpr uint32_t kLdsFloats = kTile + kSideFloats;  /* behind the image of a chunk */

struct Config {
    int32_t snr_lo_q8, snr_hi_q8, gain_lo_q8, gain_hi_q8;
    uint32_t noise_prob_q16;
    float dither;
    uint32_t clamp;
    float pad_value;
};

struct Params {
    const float* in;
    uint64_t in_rs; /* elements */
    float* out;
    uint64_t out_rs;
    const int32_t* lengths;       /* [rows], may be null */
    const int64_t* ids;           /* [rows], may be null */
    const float* noise;           /* null: no noise, and noise_rows is 0 */
    uint64_t noise_rs;
    const int32_t* noise_lengths; /* [noise_rows], may be null */
    const float *snr_amp, *gain_amp;
    float* partials;    /* [rows][chunks][2]; read and written where reduce */
    float* stats;       /* [rows][4]: the caller's or the handle's; where reduce */
    int32_t* draws_out; /* [rows][5], may be null */
    uint64_t rows, T, chunks;
    uint64_t seed, row_base;
    uint32_t noise_rows, noise_T;
    uint32_t snr_count, gain_count; /* entries of the two tables */
    int32_t snr_lo_q8, gain_lo_q8;
    uint32_t noise_prob_q16, clamp, tile;
    uint32_t reduce; /* the partials and the finish kernel run: there is a bank, or the caller wants the stats */
    float dither, pad_value;
};

/* the LDS block of a workgroup */
struct Lds {
    float* image;    /* [tile]; the finish kernel has none */
    float* lanes;    /* [2][256]: the lanes' sums of x^2 and z^2; finish: a block of the two partials */
    uint32_t* words; /* [8]: the row's two Philox blocks */
    float* sums;     /* [2]: finish: Ex and En as they grow */
};

ALAC_WF_FN Lds carve(float* lds, uint32_t image_floats) {
    Lds l;
    l.image = lds;
    l.lanes = lds + image_floats;
    l.words = (uint32_t*)(l.lanes + 2u * kThreads);
    l.sums = (float*)(l.words + 8u);
    return l;
}

/* what a workgroup of the partials or the apply kernel works on */
struct Chunk {
    uint64_t row, id, t0; /* the chunk's first sample */
    uint32_t ng, nv;      /* its samples, and the valid ones among them */
    const float* x;       /* the input row's sample t0 */
    float* y;             /* the output row's sample t0 */
};

ALAC_WF_FN uint64_t id_of(const Params& p, uint64_t row) { return p.ids ? (uint64_t)p.ids[row] : p.row_base + row; }

ALAC_WF_FN Chunk make_chunk(const Params& p, uint64_t row, uint64_t chunk) {
    Chunk c{};
    c.row = row;
    c.id = id_of(p, row);
    c.t0 = chunk * p.tile;
    const uint64_t n = length_of(p.lengths, p.T, row);
    c.ng = p.T - c.t0 < p.tile ? (uint32_t)(p.T - c.t0) : p.tile;
    c.nv = n > c.t0 ? (n - c.t0 < c.ng ? (uint32_t)(n - c.t0) : c.ng) : 0u;
    c.x = p.in + row * p.in_rs + c.t0;
    c.y = p.out + row * p.out_rs + c.t0;
    return c;
}

/* the resolved draws of a row */
struct Draws {
    uint32_t applied, k, o, m, snr_i, gain_i;
};

/* block `blk` (0, 1) of the row's words into words[4 blk ..] */
ALAC_WF_FN void row_block(const Params& p, uint64_t id, uint32_t blk, uint32_t* words) {
    uint32_t c[4] = {(uint32_t)id, (uint32_t)(id >> 32), blk, kRowStream};
    philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
    for (uint32_t j = 0; j < 4u; j++) words[4u * blk + j] = c[j];
}

/* work items 0 and 64 (two waves) compute one block each */
ALAC_WF_FN void row_words(const Params& p, uint64_t id, uint32_t* words, uint32_t tid) {
    if (tid == 0u) row_block(p, id, 0u, words);
    if (tid == 64u) row_block(p, id, 1u, words);
}

ALAC_WF_FN Draws resolve(const Params& p, const uint32_t* w) {
    Draws d{};
    const uint32_t N = p.noise_rows;
    d.applied = N > 0u && mulhi32(w[0], 65536u) < p.noise_prob_q16;
    d.k = mulhi32(w[1], N);
    if (N > 0u) {
        d.m = p.noise_T;
        if (p.noise_lengths) {
            const int32_t v = p.noise_lengths[d.k];
            d.m = v <= 0 ? 0u : (uint32_t)v < p.noise_T ? (uint32_t)v : p.noise_T;
        }
    }
    d.o = mulhi32(w[2], d.m);
    if (d.m == 0u) d.applied = d.k = 0u;
    d.snr_i = mulhi32(w[3], p.snr_count);
    d.gain_i = mulhi32(w[4], p.gain_count);
    return d;
}

ALAC_WF_FN void put_draws(const Params& p, uint64_t row, const Draws& d) {
    int32_t* o = p.draws_out + row * kDraws;
    o[0] = (int32_t)d.applied;
    o[1] = (int32_t)d.k;
    o[2] = (int32_t)d.o;
    o[3] = p.snr_lo_q8 + (int32_t)d.snr_i;
    o[4] = p.gain_lo_q8 + (int32_t)d.gain_i;
}

/* the chunk's wrapped noise segment z[k][(o + t0 + e) mod m], e < nv, into image[e] */
ALAC_WF_FN void stage_noise(const Params& p, const Chunk& c, const Draws& d, float* image, uint32_t tid) {
    const float* z = p.noise + (uint64_t)d.k * p.noise_rs;
    const uint32_t p0 = (d.o + (uint32_t)c.t0) % d.m; /* the one division of the chunk; o and t0 are below 2^31 */
    if (d.m >= c.nv) { /* at most two runs: up to the clip's end, then from its start */
        const uint32_t la = d.m - p0 < c.nv ? d.m - p0 : c.nv;
        lines_in(z + p0, 0u, 1u, la, image, 0u, 1u, tid);
        if (la < c.nv) lines_in(z, 0u, 1u, c.nv - la, image + la, 0u, 1u, tid);
        return;
    }
    /* a clip shorter than the chunk: each work item walks it in steps of 256 mod m */
    const uint32_t step = kThreads % d.m;
    uint32_t pos = (p0 + tid) % d.m;
    for (uint32_t e = tid; e < c.nv; e += kThreads) {
        image[e] = z[pos];
        pos += step;
        if (pos >= d.m) pos -= d.m;
    }
}

/* lane `tid`'s chain over image[tid], image[tid + 256] .. below nv */
ALAC_WF_FN float lane_sum(const float* image, uint32_t nv, uint32_t tid) {
    float acc = 0.0f;
    for (uint32_t e = tid; e < nv; e += kThreads) acc = fmaf(image[e], image[e], acc);
    return acc;
}

/* one step of the tree over both sums' lanes */
ALAC_WF_FN void fold(float* lanes, uint32_t s, uint32_t tid) {
    if (tid >= s) return;
    lanes[tid] += lanes[tid + s];
    lanes[kThreads + tid] += lanes[kThreads + tid + s];
}

ALAC_WF_FN void put_partials(const Params& p, const Chunk& c, const float* lanes, uint32_t tid) {
    if (tid != 0u) return;
    float* o = p.partials + (c.row * p.chunks + c.t0 / p.tile) * 2u;
    o[0] = lanes[0];
    o[1] = lanes[kThreads];
}

/* FINISH. The block [c0, c0 + cnt) of the row's partials into LDS; then work item 0 adds its Ex ones to sums[0] and work item 64
 * (another wave) its En ones to sums[1], in chunk order. The same two work items start the sums at +0.0f. */
ALAC_WF_FN void finish_start(float* sums, uint32_t tid) {
    if (tid == 0u) sums[0] = 0.0f;
    if (tid == 64u) sums[1] = 0.0f;
}

/* the chunks of a row that hold a valid sample */
ALAC_WF_FN uint64_t chunks_of(const Params& p, uint64_t row) { return (length_of(p.lengths, p.T, row) + p.tile - 1u) / p.tile; }

ALAC_WF_FN void finish_load(const Params& p, uint64_t row, uint64_t c0, uint32_t cnt, float* lanes, uint32_t tid) {
    if (tid >= cnt) return;
    const float* s = p.partials + (row * p.chunks + c0 + tid) * 2u;
    lanes[tid] = s[0];
    lanes[kThreads + tid] = s[1];
}

ALAC_WF_FN void finish_add(const float* lanes, uint32_t cnt, float* sums, uint32_t tid) {
    if (tid != 0u && tid != 64u) return;
    const float* s = lanes + (tid ? kThreads : 0u);
    float acc = sums[tid ? 1 : 0];
    for (uint32_t i = 0; i < cnt; i++) acc += s[i];
    sums[tid ? 1 : 0] = acc;
}

ALAC_WF_FN bool finite_positive(float v) { return v > 0.0f && v < __builtin_inff(); }

/* a and b of a row out of its draws and energies */
ALAC_WF_FN float gain_of(const Params& p, const Draws& d) { return p.gain_amp[d.gain_i]; }

ALAC_WF_FN float noise_amp_of(const Params& p, const Draws& d, float ex, float en, float a) {
    if (!d.applied || !finite_positive(ex) || !finite_positive(en)) return 0.0f;
    return (sqrtf(ex / en) * p.snr_amp[d.snr_i]) * a;
}

ALAC_WF_FN void finish_row(const Params& p, uint64_t row, const Lds& l, uint32_t tid) {
    if (tid != 0u) return;
    const float* sums = l.sums;
    const Draws d = resolve(p, l.words);
    const float a = gain_of(p, d);
    float* st = p.stats + row * kStats;
    st[0] = sums[0];
    st[1] = d.applied ? sums[1] : 0.0f;
    st[2] = a;
    st[3] = noise_amp_of(p, d, sums[0], sums[1], a);
    if (p.draws_out) put_draws(p, row, d);
}

/* the dither variate of sample t of the row */
ALAC_WF_FN float dither_of(const Params& p, uint64_t id, uint32_t t) {
    uint32_t c[4] = {(uint32_t)id, (uint32_t)(id >> 32), t, kDitherStream};
    philox4x32_10(c, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
    const int32_t s = (int32_t)((c[0] & 0xFFFFu) + (c[0] >> 16) + (c[1] & 0xFFFFu) + (c[1] >> 16)) -
                      (int32_t)((c[2] & 0xFFFFu) + (c[2] >> 16) + (c[3] & 0xFFFFu) + (c[3] >> 16));
    return (float)s * kDitherScale;
}

/* APPLY: the chunk's line of y, 16 bytes at a time in the chunks of the absolute address space that lie inside it, element by
 * element at its two ends; x likewise where it is aligned as y is, else element by element. image holds the noise where b != 0. */
template <bool Dither>
ALAC_WF_FN void apply_chunk(const Params& p, const Chunk& c, float a, float b, const float* image, uint32_t tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t cpl = (c.ng + 3u) / 4u + 1u;
    const int32_t lead = (int32_t)(((uintptr_t)c.y >> 2) & 3u);
    for (uint32_t q = tid; q < cpl; q += kThreads) {
        const int32_t e0 = (int32_t)(4u * q) - lead; /* slot j of the chunk is sample t0 + e0 + j */
        if (e0 >= (int32_t)c.ng) continue;
        const bool whole = e0 >= 0 && (uint32_t)e0 + 4u <= c.ng;
        F4 v = {p.pad_value, p.pad_value, p.pad_value, p.pad_value};
        if (e0 >= 0 && (uint32_t)e0 + 4u <= c.nv && ((uintptr_t)(c.x + e0) & 15u) == 0u) v = *(const F4*)(c.x + e0);
        else
            for (int32_t j = 0; j < 4; j++)
                if (e0 + j >= 0 && (uint32_t)(e0 + j) < c.nv) v[j] = c.x[e0 + j];
        for (int32_t j = 0; j < 4; j++) {
            if (e0 + j < 0 || (uint32_t)(e0 + j) >= c.nv) continue;
            float w = a * v[j];
            if (b != 0.0f) w = fmaf(b, image[e0 + j], w);
            if constexpr (Dither) w = fmaf(p.dither, dither_of(p, c.id, (uint32_t)(c.t0 + (uint32_t)(e0 + j))), w);
            if (p.clamp) w = w < -1.0f ? -1.0f : w > 1.0f ? 1.0f : w;
            v[j] = w;
        }
        if (whole) *(F4*)(c.y + e0) = v;
        else
            for (int32_t j = 0; j < 4; j++)
                if (e0 + j >= 0 && (uint32_t)(e0 + j) < c.ng) c.y[e0 + j] = v[j];
    }
}

/* ---- host only ------------------------------------------------------------------------------------------------------ */
/* what create refuses */
inline bool config_ok(const Config& c) {
    const auto range_ok = [](int32_t lo, int32_t hi) { return lo >= -kMaxQ8 && hi <= kMaxQ8 && lo <= hi && hi - lo <= kMaxQ8; };
    return range_ok(c.snr_lo_q8, c.snr_hi_q8) && range_ok(c.gain_lo_q8, c.gain_hi_q8) && c.noise_prob_q16 <= kMaxProbQ16 &&
           c.dither >= 0.0f && c.dither < __builtin_inff() && c.clamp <= 1u;
}

/* the two tables of a configuration that config_ok accepts: computed in double, rounded once */
inline std::vector<float> snr_table(const Config& c) {
    std::vector<float> t((size_t)(c.snr_hi_q8 - c.snr_lo_q8) + 1u);
    for (size_t i = 0; i < t.size(); i++) t[i] = (float)pow(10.0, -(double)(c.snr_lo_q8 + (int32_t)i) / 5120.0);
    return t;
}

inline std::vector<float> gain_table(const Config& c) {
    std::vector<float> t((size_t)(c.gain_hi_q8 - c.gain_lo_q8) + 1u);
    for (size_t i = 0; i < t.size(); i++) t[i] = (float)pow(10.0, (double)(c.gain_lo_q8 + (int32_t)i) / 5120.0);
    return t;
}

/* whether the byte ranges of two tensors of rows x cols floats meet */
inline bool overlap(const float* a, uint64_t a_rs, uint64_t a_rows, uint64_t a_cols, const float* b, uint64_t b_rs, uint64_t b_rows,
                    uint64_t b_cols) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + 4u * ((a_rows - 1u) * a_rs + a_cols);
    const uintptr_t b0 = (uintptr_t)b, b1 = b0 + 4u * ((b_rows - 1u) * b_rs + b_cols);
    return a0 < b1 && b0 < a1;
}

/* the floats of the handle's block for one pass: the partials and, where the caller keeps none, the stats; 0 where only the
 * apply kernel runs; false where the sizes overflow */
inline bool scratch_floats_of(uint64_t rows, uint64_t T, bool reduce, bool own_stats, uint64_t* floats) {
    const uint64_t chunks = (T + kTile - 1u) / kTile;
    if (chunks > ((uint64_t)1 << 58) / rows) return false;
    *floats = reduce ? rows * chunks * 2u + (own_stats ? rows * kStats : 0u) : 0u;
    return true;
}

/* the arguments of one pass (rows, T >= 1); false for what the entry rejects. The partials, and the stats where the caller
 * passes none, are set by set_scratch. */
inline bool make_params(const Config& c, const float* snr_amp, const float* gain_amp, const float* in, uint64_t in_rs, uint64_t rows,
                        uint64_t T, const int32_t* lengths, const float* noise, uint64_t noise_rs, uint64_t noise_rows, uint64_t noise_T,
                        const int32_t* noise_lengths, uint64_t seed, uint64_t row_base, const int64_t* ids, float* out, uint64_t out_rs,
                        int32_t* draws_out, float* stats, Params* p) {
    if (!in || !out || (((uintptr_t)in | (uintptr_t)out | (uintptr_t)lengths | (uintptr_t)noise | (uintptr_t)noise_lengths |
                         (uintptr_t)draws_out | (uintptr_t)stats) & 3u) || ((uintptr_t)ids & 7u))
        return false;
    if (T > 0x7fffffffu || noise_T > 0x7fffffffu || noise_rows > 0x7fffffffu) return false; /* the draws are int32 */
    const uint64_t lim = (uint64_t)1 << 61;
    if (in_rs > lim / rows || out_rs > lim / rows || (rows > 1u && (in_rs < T || out_rs < T))) return false;
    if (!(in == out && (rows == 1u || in_rs == out_rs)) && overlap(in, in_rs, rows, T, out, out_rs, rows, T)) return false;
    Params q{};
    if (noise && noise_rows > 0u && noise_T > 0u) {
        if (noise_rs > lim / noise_rows || (noise_rows > 1u && noise_rs < noise_T)) return false;
        if (overlap(noise, noise_rs, noise_rows, noise_T, out, out_rs, rows, T)) return false;
        q.noise = noise;
        q.noise_rs = noise_rs;
        q.noise_lengths = noise_lengths;
        q.noise_rows = (uint32_t)noise_rows;
        q.noise_T = (uint32_t)noise_T;
    }
    q.in = in;
    q.in_rs = in_rs;
    q.out = out;
    q.out_rs = out_rs;
    q.lengths = lengths;
    q.ids = ids;
    q.snr_amp = snr_amp;
    q.gain_amp = gain_amp;
    q.stats = stats;
    q.draws_out = draws_out;
    q.rows = rows;
    q.T = T;
    q.tile = kTile;
    q.chunks = (T + kTile - 1u) / kTile;
    if (q.chunks > ((uint64_t)1 << 58) / rows) return false;
    q.seed = seed;
    q.row_base = row_base;
    q.snr_count = (uint32_t)(c.snr_hi_q8 - c.snr_lo_q8) + 1u;
    q.gain_count = (uint32_t)(c.gain_hi_q8 - c.gain_lo_q8) + 1u;
    q.snr_lo_q8 = c.snr_lo_q8;
    q.gain_lo_q8 = c.gain_lo_q8;
    q.noise_prob_q16 = c.noise_prob_q16;
    q.clamp = c.clamp;
    q.reduce = q.noise || stats ? 1u : 0u;
    q.dither = c.dither;
    q.pad_value = c.pad_value;
    *p = q;
    return true;
}

/* the handle's block behind the arguments: the partials, then the stats where the caller passed none */
inline void set_scratch(Params* p, float* block) {
    if (!p->reduce) return;
    p->partials = block;
    if (!p->stats) p->stats = block + p->rows * p->chunks * 2u;
}

}  // namespace alacwa

#if defined(__HIPCC__)
/* k_waveaug.hip */
namespace alack {
/* The kernels of one pass on `stream`. */
hipError_t waveaug_launch(hipStream_t stream, const alacwa::Params& p);
}  // namespace alack
#endif
#endif /* ALAC_WAVEAUG_H */
