/*
 * alac_mel.h — float32 rows -> their power or (log-)mel spectrograms: the plan (basis and filterbank tables), the index
 * arithmetic and the phases of a tile, as plain host + device code. k_mel.hip builds the gfx950 kernel from this text;
 * tests/host_sim/mel_sim.cpp builds the same text with g++ (contraction off) for the CPU suite.
 *
 * The definition. N = n_fft in [2, 2048], W = win_length in [1, N], h = hop_length >= 1, K = N / 2 + 1 bins.
 *
 *   window   periodic Hann, hann[j] = 0.5 - 0.5 cos(2 pi j / W) for j < W, at offset (N - W) / 2 within N, zero elsewhere
 *            (torch.stft's centring of a short window): w[n]. W = 1 is the one sample 1.0, as torch.hann_window(1) is, not
 *            the formula's 0.
 *   basis    C[k][n] = w[n] cos(2 pi ((k n) mod N) / N),  S[k][n] = w[n] sin(2 pi ((k n) mod N) / N): the integer reduction
 *            first, (2 pi r) / N, cos, sin and the product in double, each entry rounded to float32 once, +0.0f where w[n] is
 *            0. The window lives in the table: there is no separate multiply.
 *   frames   center: F = 1 + (T - (N & 1)) / h for T > N / 2 (torch.stft's 1 + (T + 2 (N / 2) - N) / h: it pads N / 2 on
 *            each side), frame f reads xr[f h - N / 2 + n], xr[i] = x[-i] for i < 0, x[2 (T - 1) - i] for i >= T. The last
 *            frame reads up to T + N / 2 - 1, which reflects to T - 1 - N / 2 >= 0: every index of a frame that exists lies
 *            in [0, T) after one reflection. Otherwise F = 1 + (T - N) / h for T >= N and frame f reads x[f h + n].
 *            out_frames(T) is 0 where no frame exists.
 *   power    re = im = +0.0f;  for n = 0 .. N - 1:  re = fmaf(C[k][n], xr[n], re);  im = fmaf(S[k][n], xr[n], im)
 *            p[k] = fmaf(im, im, re * re)                                 the product rounded on its own
 *   mel      fb = torchaudio.functional.melscale_fbanks(K, f_min, f_max, n_mels, sample_rate, norm, mel_scale) restated in
 *            double: all_freqs[k] = k * ((sample_rate / 2) / (K - 1)), the last one sample_rate / 2 itself; n_mels + 2 points
 *            equally spaced on the mel scale from f_min to f_max (the two end points are f_min and f_max themselves, not
 *            their round trip through the scale); weight = max(0, min(down, up)), down = (f - pt[m]) / (pt[m + 1] - pt[m]),
 *            up = (pt[m + 2] - f) / (pt[m + 2] - pt[m + 1]); slaney norm multiplies by 2 / (pt[m + 2] - pt[m]); htk is 2595
 *            log10(1 + f / 700), slaney 3 f / 200 below 1 kHz and 15 + ln(f / 1000) / (ln(6.4) / 27) from there. Each weight
 *            is rounded to float32 once. A filter's weights that are not zero are ONE run: the plan keeps first[m] and taps
 *            (the widest run, at least 1), windows clamped into [0, K), fbw[m][q] = float(fb[first[m] + q][m]).
 *            acc = +0.0f;  for q = 0 .. taps - 1:  acc = fmaf(fbw[m][q], p[first[m] + q], acc)
 *            A filter without a weight that is not zero is legal; its output is +0.0.
 *   log      v <= floor ? float(s log(floor)) : s * log(v), s = 1 with ln or log10, 10 with log10 for "db"; floor is the
 *            float32 nearest the configured one. The one step that is not pinned bit for bit: the device's log and libm's
 *            differ in the last places.
 *   output   [rows][bins][F] float32, bins = n_mels (or K without a mel stage), element (r, b, f) at out + r * row_stride +
 *            b * bin_stride + f. Exactly those elements are written.
 *
 * A TILE is tile_frames consecutive frames of one row, one workgroup of 256. Phase 1 (stage_tile) brings the (tile_frames -
 * 1) h + N inputs of the tile into LDS, 16 bytes at a time where a 16-byte chunk of the ABSOLUTE address space lies inside
 * the row and needs no reflection, element by element elsewhere, with reflection and the zeros resolved here; the image keeps
 * the source's offset within its first chunk (alacrs::stage_tile). Where h > N the frames are staged one behind the other, N
 * each. Frames of the tile behind the row's last are staged like the others and computed, and never stored. Phase 2
 * (dft_tile): a work item owns FB frames x 2 neighbouring bins, 4 FB accumulators, and walks n upwards; the frames come from
 * LDS (a wave reads at most two addresses at a time), the basis from a table [n][bin pair]{C[2b], S[2b], C[2b + 1], S[2b + 1]}
 * in global memory, so neighbouring work items read neighbouring 16 bytes, four n ahead of their use. The powers go to an LDS
 * tile [tile_frames][KP], KP = K | 1 (an odd pitch: walking frames at one bin touches every bank once). Phase 3: the mel
 * chains out of that tile, work items along the frames, and the log, into an LDS output tile [n_mels][tile_frames] that takes
 * the staging buffer's place; without a mel stage the log is applied to the power tile where it lies. Phase 4 (store_tile):
 * per bin, the 16-byte chunks of the absolute address space inside the tile's frames with one store each, the elements of a
 * chunk that the tile covers in part one by one.
 */
#ifndef ALAC_MEL_H
#define ALAC_MEL_H

#include "alac_waveform.h"

#include <cmath>
#include <vector>

namespace alacmel {

using alacwf::kThreads;

constexpr uint32_t kMaxFft = 2048, kMaxMels = 4096;
constexpr uint32_t kMaxTile = 64, kMinTile = 4; /* frames: 256 bytes of a bin's row down to one 16-byte store */
constexpr uint32_t kLdsFloats = 16384;          /* 64 KB: what a workgroup may ask for without an attribute */

enum : uint32_t { kLogNone = 0, kLogLn = 1, kLogLog10 = 2, kLogDb = 3 };
enum : uint32_t { kScaleNone = 0, kScaleHtk = 1, kScaleSlaney = 2 };

/* 16 bytes moved by one instruction */
typedef float F4 __attribute__((vector_size(16), may_alias));

struct Params {
    const float* in;         /* 4-byte aligned */
    uint64_t in_stride;      /* elements */
    uint64_t rows;
    uint64_t in_frames;      /* T */
    float* out;              /* 4-byte aligned */
    uint64_t out_row_stride; /* elements */
    uint64_t out_bin_stride;
    uint64_t out_frames;     /* F */
    const F4* bt;            /* [N][BP]: {C[2b][n], S[2b][n], C[2b + 1][n], S[2b + 1][n]} */
    const float* fbw;        /* [n_mels][taps] */
    const int32_t* first;    /* [n_mels] */
    uint32_t N, hop, K, KP, BP;
    uint32_t n_mels, taps, bins;
    uint32_t center, log;
    float floor, log_floor;
    uint32_t tile_frames;
    uint32_t fs;             /* a frame's distance from the one before it in the staged image: min(hop, N) */
    uint32_t a_floats;       /* the staging / output tile's floats; the power tile lies behind them */
    uint64_t tiles_per_row;  /* ceil(F / tile_frames) */
};

/* F; 0 where no frame exists */
ALAC_WF_FN uint64_t out_frames_of(uint32_t N, uint32_t hop, uint32_t center, uint64_t T) {
    if (center) return T > N / 2u ? 1u + (T - (N & 1u)) / hop : 0u;
    return T >= N ? 1u + (T - N) / hop : 0u;
}

/* what a tile works on */
struct Tile {
    const float* x; /* the input row's sample 0 */
    float* y;       /* the output row's element (bin 0, frame 0) */
    uint64_t c0;    /* first frame */
    uint32_t count; /* frames to store; 0: nothing to do */
    int64_t lo;     /* the index frame c0 reads at n = 0; negative in a centred row's first tile */
    uint32_t span;  /* inputs staged */
    uint32_t sh;    /* elements of x + lo behind a 16-byte boundary (0 where hop > N) */
};

ALAC_WF_FN Tile make_tile(const Params& p, uint64_t row, uint64_t tile) {
    Tile t{};
    t.x = p.in + row * p.in_stride;
    t.y = p.out + row * p.out_row_stride;
    t.c0 = tile * p.tile_frames;
    if (t.c0 >= p.out_frames) return t;
    const uint64_t left = p.out_frames - t.c0;
    t.count = left < p.tile_frames ? (uint32_t)left : p.tile_frames;
    t.lo = (int64_t)(t.c0 * p.hop) - (p.center ? (int64_t)(p.N / 2u) : 0);
    if (p.hop <= p.N) {
        t.span = (p.tile_frames - 1u) * p.hop + p.N;
        t.sh = (uint32_t)((int64_t)((uintptr_t)t.x >> 2) + t.lo) & 3u;
    } else {
        t.span = p.tile_frames * p.N;
    }
    return t;
}

/* xr[i] of the row x: the reflection of a centred row. No frame that exists reaches outside [0, T) after it; the frames a tile
 * stages behind the row's last do, and get +0.0 there (they are computed and never stored). */
ALAC_WF_FN float sample_at(const Params& p, const float* x, int64_t i) {
    const int64_t T = (int64_t)p.in_frames;
    if (p.center) {
        if (i < 0) i = -i;
        else if (i >= T) i = 2 * (T - 1) - i;
    }
    return (i >= 0 && i < T) ? x[i] : 0.0f;
}

/* Phase 1: work item `tid` of kThreads fills its part of stage (16-byte aligned, a_floats): stage[sh + e] = xr[lo + e] for e <
 * span where hop <= N, stage[f N + n] = xr[lo + f hop + n] otherwise. Nothing outside [0, T) of the row is read. */
ALAC_WF_FN void stage_tile(const Params& p, const Tile& t, float* stage, uint32_t tid) {
    if (p.hop > p.N) {
        for (uint32_t e = tid; e < t.span; e += kThreads) {
            const uint32_t f = e / p.N;
            stage[e] = sample_at(p, t.x, t.lo + (int64_t)((uint64_t)f * p.hop) + (e - f * p.N));
        }
        return;
    }
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
                if (e >= t.sh && e < total) stage[e] = sample_at(p, t.x, idx0 + b);
            }
        }
    }
}

/* one n of FB frames x 2 bins: acc[j] = {re, im of bin 2b, re, im of bin 2b + 1} of frame j */
template <uint32_t FB>
ALAC_WF_FN void dft_step(float (&acc)[FB][4], const F4 c, const float* xs, uint32_t fs) {
    for (uint32_t j = 0; j < FB; j++) {
        const float x = xs[j * fs];
        acc[j][0] = fmaf(c[0], x, acc[j][0]);
        acc[j][1] = fmaf(c[1], x, acc[j][1]);
        acc[j][2] = fmaf(c[2], x, acc[j][2]);
        acc[j][3] = fmaf(c[3], x, acc[j][3]);
    }
}

/* Phase 2: work item `tid` of kThreads runs the chains of its blocks of FB frames x 2 bins (block i = group of frames i / BP,
 * bin pair i % BP; i = tid, tid + 256, ...) out of stage and puts their powers into ptile [tile_frames][KP]. The basis of the
 * next four n is asked for before the four at hand are used. */
template <uint32_t FB>
ALAC_WF_FN void dft_blocks(const Params& p, const Tile& t, const float* stage, float* ptile, uint32_t tid) {
    const uint32_t items = (p.tile_frames / FB) * p.BP;
    const uint32_t N = p.N, BP = p.BP, fs = p.fs;
    for (uint32_t i = tid; i < items; i += kThreads) {
        const uint32_t g = i / BP, bp = i - g * BP;
        const float* xs = stage + t.sh + g * FB * fs;
        const F4* bt = p.bt + bp;
        float acc[FB][4];
        for (uint32_t j = 0; j < FB; j++) acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0f;
        uint32_t n = 0;
        if (N >= 4u) {
            F4 a0 = bt[0], a1 = bt[BP], a2 = bt[2u * BP], a3 = bt[3u * BP];
            for (; n + 8u <= N; n += 4u) {
                const F4* nx = bt + (size_t)(n + 4u) * BP;
                const F4 b0 = nx[0], b1 = nx[BP], b2 = nx[2u * BP], b3 = nx[3u * BP];
                dft_step<FB>(acc, a0, xs + n, fs);
                dft_step<FB>(acc, a1, xs + n + 1u, fs);
                dft_step<FB>(acc, a2, xs + n + 2u, fs);
                dft_step<FB>(acc, a3, xs + n + 3u, fs);
                a0 = b0, a1 = b1, a2 = b2, a3 = b3;
            }
            dft_step<FB>(acc, a0, xs + n, fs);
            dft_step<FB>(acc, a1, xs + n + 1u, fs);
            dft_step<FB>(acc, a2, xs + n + 2u, fs);
            dft_step<FB>(acc, a3, xs + n + 3u, fs);
            n += 4u;
        }
        for (; n < N; n++) dft_step<FB>(acc, bt[(size_t)n * BP], xs + n, fs);
        const uint32_t k0 = 2u * bp;
        for (uint32_t j = 0; j < FB; j++) {
            float* row = ptile + (g * FB + j) * p.KP + k0;
            row[0] = fmaf(acc[j][1], acc[j][1], acc[j][0] * acc[j][0]);
            if (k0 + 1u < p.K) row[1] = fmaf(acc[j][3], acc[j][3], acc[j][2] * acc[j][2]);
        }
    }
}

ALAC_WF_FN void dft_tile(const Params& p, const Tile& t, const float* stage, float* ptile, uint32_t tid) {
    if (p.tile_frames % 8u == 0u) dft_blocks<8>(p, t, stage, ptile, tid);
    else dft_blocks<4>(p, t, stage, ptile, tid);
}

ALAC_WF_FN float apply_log(const Params& p, float v) {
    if (p.log == kLogNone) return v;
    if (v <= p.floor) return p.log_floor;
    return p.log == kLogLn ? logf(v) : p.log == kLogLog10 ? log10f(v) : 10.0f * log10f(v);
}

/* Phase 3 with a mel stage: work item `tid` runs the chains of the outputs i = tid, tid + 256, ... (filter i / tile_frames,
 * frame i % tile_frames) out of ptile, eight weights asked for at a time, and puts log(acc) into outt [n_mels][tile_frames]. */
ALAC_WF_FN void mel_tile(const Params& p, const float* ptile, float* outt, uint32_t tid) {
    const uint32_t TF = p.tile_frames, items = p.n_mels * TF, taps = p.taps;
    for (uint32_t i = tid; i < items; i += kThreads) {
        const uint32_t m = i / TF, f = i - m * TF;
        const float* w = p.fbw + (size_t)m * taps;
        const float* pp = ptile + f * p.KP + p.first[m];
        float acc = 0.0f;
        uint32_t q = 0;
        for (; q + 8u <= taps; q += 8u) {
            float v[8];
            for (uint32_t u = 0; u < 8u; u++) v[u] = w[q + u];
            for (uint32_t u = 0; u < 8u; u++) acc = fmaf(v[u], pp[q + u], acc);
        }
        for (; q < taps; q++) acc = fmaf(w[q], pp[q], acc);
        outt[i] = apply_log(p, acc);
    }
}

/* Phase 3 without one: the log over the power tile where it lies */
ALAC_WF_FN void log_tile(const Params& p, float* ptile, uint32_t tid) {
    if (p.log == kLogNone) return;
    const uint32_t items = p.tile_frames * p.K;
    for (uint32_t i = tid; i < items; i += kThreads) {
        const uint32_t f = i / p.K;
        float* v = ptile + f * p.KP + (i - f * p.K);
        *v = apply_log(p, *v);
    }
}

/* Phase 4: element (bin b, frame c0 + f) is src[b * sb + f * sf]. Work item `tid` stores its 16-byte chunks: chunk c of bin b
 * is the elements 4 c - lead + [0, 4) of the bin's frames [c0, c0 + count), lead their first one's elements behind a 16-byte
 * boundary. */
ALAC_WF_FN void store_tile(const Params& p, const Tile& t, const float* src, uint32_t sb, uint32_t sf, uint32_t tid) {
    const uint32_t cpb = p.tile_frames / 4u + 1u; /* chunks a bin's count <= tile_frames frames can touch */
    const uint32_t items = p.bins * cpb;
    for (uint32_t i = tid; i < items; i += kThreads) {
        const uint32_t b = i / cpb, e0 = 4u * (i - b * cpb);
        float* row = t.y + (uint64_t)b * p.out_bin_stride + t.c0;
        const uint32_t lead = (uint32_t)((uintptr_t)row >> 2) & 3u;
        const uint32_t total = lead + t.count;
        if (e0 >= total) continue;
        const float* s = src + b * sb;
        if (e0 >= lead && e0 + 4u <= total) {
            const uint32_t f = e0 - lead;
            F4 v;
            v[0] = s[f * sf];
            v[1] = s[(f + 1u) * sf];
            v[2] = s[(f + 2u) * sf];
            v[3] = s[(f + 3u) * sf];
            *(F4*)(row + f) = v;
        } else {
            for (uint32_t u = 0; u < 4u; u++)
                if (e0 + u >= lead && e0 + u < total) row[e0 + u - lead] = s[(e0 + u - lead) * sf];
        }
    }
}

/* ---- the plan: host only ------------------------------------------------------------------------------------------- */
struct Config {
    uint32_t sample_rate = 0, n_fft = 0, win_length = 0, hop_length = 0;
    double f_min = 0.0, f_max = 0.0;
    uint32_t n_mels = 0;
    uint32_t center = 1;
    uint32_t norm = 0;      /* 0 none, 1 slaney */
    uint32_t mel_scale = 0; /* kScale*: none = the power spectrogram itself */
    uint32_t log = 0;       /* kLog* */
    double floor = 1e-10;
};

struct Plan {
    Config cfg;
    uint32_t N = 0, W = 0, hop = 0, K = 0, KP = 0, BP = 0, n_mels = 0, taps = 0, bins = 0;
    uint32_t tile_frames = 0, fs = 0, a_floats = 0, lds_floats = 0;
    float floor = 0.0f, log_floor = 0.0f;
    std::vector<float> basis;   /* [2][K][N]: C, then S */
    std::vector<float> bt;      /* [N][BP][4], what the device reads */
    std::vector<float> fbw;     /* [n_mels][taps] */
    std::vector<int32_t> first; /* [n_mels] */
};

inline double hz_to_mel(double f, uint32_t scale) {
    if (scale == kScaleHtk) return 2595.0 * std::log10(1.0 + f / 700.0);
    if (f >= 1000.0) return 15.0 + std::log(f / 1000.0) / (std::log(6.4) / 27.0);
    return f / (200.0 / 3.0);
}

inline double mel_to_hz(double m, uint32_t scale) {
    if (scale == kScaleHtk) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    if (m >= 15.0) return 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0));
    return (200.0 / 3.0) * m;
}

/* the periodic Hann window of W samples within N, in double: 0.5 - 0.5 cos(2 pi j / W) at offset (N - W) / 2 ([1.0] for W = 1),
 * 0 elsewhere */
inline std::vector<double> hann_window(uint32_t N, uint32_t W) {
    const double pi = 3.14159265358979323846;
    std::vector<double> w(N, 0.0);
    const uint32_t off = (N - W) / 2u;
    for (uint32_t j = 0; j < W; j++) w[off + j] = W == 1u ? 1.0 : 0.5 - 0.5 * std::cos(2.0 * pi * (double)j / (double)W);
    return w;
}

/* The dense filterbank fb [M][K] the way the device reads it: first[m] = filter m's first bin with a weight, taps = the longest
 * run of weights (at least 1), fbw [M][taps] = the weights from first[m] on, first[m] moved down where that would pass K. false:
 * a filter whose weights are not one run. The Kaldi plan's filterbank (alac_fbank.h) goes through here as well. */
inline bool compact_filters(const std::vector<float>& fb, uint32_t M, uint32_t K, std::vector<int32_t>* first, uint32_t* taps,
                            std::vector<float>* fbw) {
    first->assign(M, 0);
    *taps = 1u;
    for (uint32_t m = 0; m < M; m++) {
        const float* w = &fb[(size_t)m * K];
        int64_t f = -1, l = -1;
        for (uint32_t k = 0; k < K; k++)
            if (w[k] != 0.0f) {
                if (f < 0) f = k;
                l = k;
            }
        if (f < 0) continue;
        for (int64_t k = f; k <= l; k++)
            if (w[k] == 0.0f) return false; /* not one run */
        (*first)[m] = (int32_t)f;
        if ((uint32_t)(l - f + 1) > *taps) *taps = (uint32_t)(l - f + 1);
    }
    fbw->assign((size_t)M * *taps, 0.0f);
    for (uint32_t m = 0; m < M; m++) {
        if ((uint32_t)(*first)[m] + *taps > K) (*first)[m] = (int32_t)(K - *taps);
        for (uint32_t q = 0; q < *taps; q++) (*fbw)[(size_t)m * *taps + q] = fb[(size_t)m * K + (uint32_t)(*first)[m] + q];
    }
    return true;
}

/* floats of LDS a tile of tf frames needs: the staged inputs with their offset within a chunk, or the output tile in their
 * place, and the power tile */
inline uint64_t lds_need(const Plan& pl, uint32_t tf, uint32_t* a_floats) {
    uint64_t a = pl.hop <= pl.N ? (uint64_t)(tf - 1u) * pl.hop + pl.N + 3u : (uint64_t)tf * pl.N;
    const uint64_t o = (uint64_t)pl.n_mels * tf;
    if (o > a) a = o;
    a = (a + 3u) & ~(uint64_t)3u;
    if (a_floats) *a_floats = (uint32_t)a;
    return a + (uint64_t)tf * pl.KP;
}

/* false: no plan for these arguments (N outside [2, 2048], W outside [1, N], hop 0, a sample rate of 0, an enum outside its
 * values, floor not a positive float32, with a mel stage n_mels outside [1, 4096] or not 0 <= f_min < f_max, without one n_mels
 * or norm not 0, or four frames that do not fit the LDS budget). with_basis false leaves basis and bt empty: the plan of a pass
 * that brings its own transform (alac_melfft.h). */
inline bool make_plan(const Config& c, Plan* out, bool with_basis = true) {
    if (c.n_fft < 2u || c.n_fft > kMaxFft || c.win_length < 1u || c.win_length > c.n_fft || c.hop_length < 1u || !c.sample_rate)
        return false;
    if (c.center > 1u || c.norm > 1u || c.mel_scale > kScaleSlaney || c.log > kLogDb) return false;
    const float floor32 = (float)c.floor;
    if (!(c.floor > 0.0) || !(floor32 > 0.0f) || !std::isfinite(floor32)) return false;
    if (c.mel_scale != kScaleNone) {
        if (c.n_mels < 1u || c.n_mels > kMaxMels) return false;
        if (!std::isfinite(c.f_min) || !std::isfinite(c.f_max) || !(c.f_min >= 0.0) || !(c.f_min < c.f_max)) return false;
    } else if (c.n_mels || c.norm) {
        return false;
    }
    Plan pl;
    pl.cfg = c;
    const uint32_t N = pl.N = c.n_fft, W = pl.W = c.win_length, K = pl.K = N / 2u + 1u;
    pl.hop = c.hop_length;
    pl.KP = K | 1u;
    pl.BP = (K + 1u) / 2u;
    pl.n_mels = c.mel_scale != kScaleNone ? c.n_mels : 0u;
    pl.bins = pl.n_mels ? pl.n_mels : K;
    pl.fs = pl.hop < N ? pl.hop : N;
    pl.floor = floor32;
    const double lf = c.log == kLogLn ? std::log((double)floor32) : std::log10((double)floor32);
    pl.log_floor = c.log == kLogNone ? 0.0f : (float)((c.log == kLogDb ? 10.0 : 1.0) * lf);

    const double pi = 3.14159265358979323846;
    const std::vector<double> w = hann_window(N, W);
    if (with_basis) {
        pl.basis.assign((size_t)2 * K * N, 0.0f);
        pl.bt.assign((size_t)N * pl.BP * 4u, 0.0f);
        for (uint32_t k = 0; k < K; k++)
            for (uint32_t n = 0; n < N; n++) {
                const uint32_t r = (uint32_t)(((uint64_t)k * n) % N);
                const double ang = 2.0 * pi * (double)r / (double)N;
                const bool in = w[n] != 0.0; /* +0.0f, not the -0.0f a negative cosine would make of it, outside the window */
                const float cv = in ? (float)(w[n] * std::cos(ang)) : 0.0f, sv = in ? (float)(w[n] * std::sin(ang)) : 0.0f;
                pl.basis[((size_t)k) * N + n] = cv;
                pl.basis[((size_t)K + k) * N + n] = sv;
                float* e = &pl.bt[((size_t)n * pl.BP + k / 2u) * 4u + 2u * (k & 1u)];
                e[0] = cv;
                e[1] = sv;
            }
    }

    if (pl.n_mels) {
        const uint32_t M = pl.n_mels;
        std::vector<double> freqs(K), pts(M + 2u);
        const double half = (double)(c.sample_rate / 2u), fstep = half / (double)(K - 1u);
        for (uint32_t k = 0; k < K; k++) freqs[k] = (double)k * fstep;
        freqs[K - 1u] = half;
        const double m_min = hz_to_mel(c.f_min, c.mel_scale), m_max = hz_to_mel(c.f_max, c.mel_scale);
        const double mstep = (m_max - m_min) / (double)(M + 1u);
        for (uint32_t i = 0; i < M + 2u; i++) pts[i] = mel_to_hz(m_min + (double)i * mstep, c.mel_scale);
        pts[0] = c.f_min;
        pts[M + 1u] = c.f_max;
        for (uint32_t i = 0; i + 1u < M + 2u; i++)
            if (!(pts[i + 1u] > pts[i])) return false;
        std::vector<float> fb((size_t)M * K);
        for (uint32_t m = 0; m < M; m++) {
            const double d0 = pts[m + 1u] - pts[m], d1 = pts[m + 2u] - pts[m + 1u];
            const double enorm = c.norm ? 2.0 / (pts[m + 2u] - pts[m]) : 1.0;
            for (uint32_t k = 0; k < K; k++) {
                const double down = (freqs[k] - pts[m]) / d0, up = (pts[m + 2u] - freqs[k]) / d1;
                double v = down < up ? down : up;
                if (!(v > 0.0)) v = 0.0;
                if (c.norm) v *= enorm;
                fb[(size_t)m * K + k] = (float)v;
            }
        }
        if (!compact_filters(fb, M, K, &pl.first, &pl.taps, &pl.fbw)) return false;
    }

    uint32_t tf = kMaxTile;
    while (tf > kMinTile && lds_need(pl, tf, nullptr) > kLdsFloats) tf /= 2u;
    const uint64_t need = lds_need(pl, tf, &pl.a_floats);
    if (need > kLdsFloats) return false;
    pl.tile_frames = tf;
    pl.lds_floats = (uint32_t)need;
    *out = std::move(pl);
    return true;
}

/* the arguments of one pass with frames to write; false for what the entry rejects */
inline bool make_params(const Plan& pl, const float* in, uint64_t in_stride, uint64_t rows, uint64_t in_frames, float* out,
                        uint64_t out_row_stride, uint64_t out_bin_stride, const float* bt, const float* fbw, const int32_t* first,
                        Params* p) {
    if (!in || !out || ((uintptr_t)in & 3u) || ((uintptr_t)out & 3u) || !rows) return false;
    if (in_frames > ((uint64_t)1 << 61)) return false;
    const uint64_t F = out_frames_of(pl.N, pl.hop, pl.cfg.center, in_frames);
    if (!F) return false;
    if (in_stride < in_frames || out_bin_stride < F) return false;
    const uint64_t lim = SIZE_MAX / 8u;
    if (out_bin_stride > lim / pl.bins) return false;
    if (out_row_stride < (uint64_t)(pl.bins - 1u) * out_bin_stride + F) return false;
    if (in_stride > lim / rows || out_row_stride > lim / rows) return false;
    const uint64_t tpr = (F + pl.tile_frames - 1u) / pl.tile_frames;
    if (tpr > (~(uint64_t)0) / rows) return false;
    *p = Params{in, in_stride, rows, in_frames, out, out_row_stride, out_bin_stride, F, (const F4*)bt, fbw, first,
                pl.N, pl.hop, pl.K, pl.KP, pl.BP, pl.n_mels, pl.taps, pl.bins, pl.cfg.center, pl.cfg.log, pl.floor, pl.log_floor,
                pl.tile_frames, pl.fs, pl.a_floats, tpr};
    return true;
}

}  // namespace alacmel

#if defined(__HIPCC__)
/* k_mel.hip */
namespace alack {
/* All kernels of one pass on `stream`. */
hipError_t mel_launch(hipStream_t stream, const alacmel::Params& p, uint32_t lds_bytes);
}  // namespace alack
#endif
#endif /* ALAC_MEL_H */
