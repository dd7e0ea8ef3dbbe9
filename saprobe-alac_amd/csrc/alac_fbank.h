/*
 * alac_fbank.h — float32 rows -> Kaldi's filterbank (fbank) or MFCC features: the plan, the index arithmetic and the phases
 * of a tile that alac_mel.h does not have, as plain host + device code over that header. k_fbank.hip builds the gfx950 kernel
 * from this text; tests/host_sim/fbank_sim.cpp builds the same text with g++ (contraction off) for the CPU suite.
 *
 * The definition (what torchaudio.compliance.kaldi.fbank / .mfcc compute). W = frame length in [1, 2048] samples,
 * h = frame shift >= 1, N = the DFT size: the next power of two >= W with round_to_power_of_two, else W; K = N / 2 + 1.
 *
 *   frames   snip_edges: F = 1 + (T - W) / h for T >= W, frame f reads x[f h + n], n < W. Otherwise F = (T + h / 2) / h for
 *            T >= W, pad = W / 2 - h / 2 (integer halves; negative where h > W + 1), frame f reads xr[f h - pad + n], xr[i] =
 *            x[-1 - i] for i < 0 and x[2 T - 1 - i] for i >= T: Kaldi's reflection, which repeats the edge sample. -pad >=
 *            -(W / 2) and the last index is at most T + ceil(W / 2) - 1, so for T >= W one reflection brings every index of a
 *            frame that exists into [0, T). T < W has no frame in either mode.
 *   frame    the mean removed (remove_dc_offset), pre-emphasis y[n] = v[n] - c v[n - 1] with v[-1] = v[0], the window
 *            (symmetric: a = 2 pi / (W - 1); hanning 0.5 - 0.5 cos(a n), hamming 0.54 - 0.46 cos(a n), povey hanning^0.85,
 *            rectangular 1, blackman b - 0.5 cos(a n) + (0.5 - b) cos(2 a n); W = 1 is [1.0]), zeros up to N. These are one
 *            linear map of the W raw samples, so the plan folds them into the basis, in double, each entry rounded once:
 *              A[k][j] = win[j] cos(2 pi ((k j) mod N) / N)
 *              G[k][n] = A[k][n] - c A[k][n + 1] (no second term at n = W - 1);  G[k][0] -= c A[k][0]
 *              C[k][n] = scale (G[k][n] - (sum_j G[k][j]) / W)                    (no mean term without remove_dc_offset)
 *            and S the same with sin. An entry that is zero is +0.0f.
 *   power    alac_mel.h's: re, im fmaf chains over n = 0 .. W - 1 from +0.0f, p = fmaf(im, im, re * re). The loop runs to W,
 *            not N: the device table is [W][BP][4].
 *   mel      get_mel_banks in double: mel(f) = 1127 ln(1 + f / 700); high_freq <= 0 means Nyquist + high_freq; 0 <= low <
 *            nyquist, 0 < high <= nyquist, low < high; M + 2 points equally spaced in mel from low to high; FFT bin k < N / 2
 *            at m = mel(k sample_rate / N) weighs max(0, min((m - left) / (centre - left), (right - m) / (right - centre))),
 *            every other bin 0; each weight rounded once; first[m], taps and the chain as in alac_mel.h.
 *   log      use_log_fbank: ln(max(v, eps)), eps = 2^-23 (alacmel::apply_log with kLogLn).
 *   energy   s = +0.0f; s += xr[n];  mean = s * float(1.0 / W) (0 without remove_dc_offset);  e = +0.0f; d = xr[n] - mean; e =
 *            fmaf(d, d, e);  e *= float(scale^2);  then ln(max(e, eps)), raised to float(ln(energy_floor)) where energy_floor
 *            > 0. log_energy = 0 (for checks) keeps e itself. Column 0, or the last with htk_compat.
 *   MFCC     over the log-mel (always log): D[c][m] = sqrt(2 / M) cos(pi (m + 0.5) c / M), row 0 sqrt(1 / M), c < num_ceps <=
 *            M, in double, rounded once; acc = +0.0f; for m upwards acc = fmaf(D[c][m], logmel[m], acc); times lifter[c] =
 *            float(1 + 0.5 L sin(pi c / L)) (1 where L = 0). With use_energy column 0 is the energy instead; with htk_compat
 *            column 0 moves to the end, and where that column is C0 itself (htk_compat without use_energy) it leaves as
 *            sqrt(2) C0, as Kaldi's MfccComputer and torchaudio ("removing a scale we previously added") do: the plan's row 0
 *            is then sqrt(2 / M), in double, rounded once (lifter[0] is 1), and the kernel only permutes.
 *   output   float32. Layout frames: [rows][F][cols], element (r, f, c) at out + r * row_stride + f * frame_stride + c.
 *            Layout bins: [rows][cols][F], element (r, c, f) at out + r * row_stride + c * bin_stride + f, as the mel pass
 *            writes. Exactly those elements are written.
 *
 * A TILE is tile_frames consecutive frames of one row, one workgroup of 256. LDS: the staging image (later the mel tile
 * [n_mels (+ 1 with an energy column of fbank)][tile_frames]), the power tile [tile_frames][KP], tile_frames floats of energy,
 * and for MFCC the cepstral tile [num_ceps][tile_frames]. stage_tile here, then the energies out of the staged image (one work
 * item per frame), alacmel::dft_tile, alacmel::mel_tile, the energy's move into its column or the DCT and lifter, and the
 * store: alacmel::store_tile for the layout bins, store_frames here for frames.
 */
#ifndef ALAC_FBANK_H
#define ALAC_FBANK_H

#include "alac_mel.h"

namespace alacfb {

using alacmel::F4;
using alacmel::kLdsFloats;
using alacmel::kMaxFft;
using alacmel::kMaxMels;
using alacmel::kMaxTile;
using alacmel::kMinTile;
using alacmel::Tile;
using alacwf::kThreads;

enum : uint32_t { kWinHanning = 0, kWinHamming = 1, kWinPovey = 2, kWinRectangular = 3, kWinBlackman = 4 };
enum : uint32_t { kLayoutFrames = 0, kLayoutBins = 1 };

struct Params {
    alacmel::Params m;     /* N = W: the chains' length; bins = cols; center unused; out_bin_stride of the layout bins */
    const float* dct;      /* [num_ceps][n_mels] */
    const float* lifter;   /* [num_ceps] */
    uint64_t frame_stride; /* elements, layout frames */
    int64_t pad;           /* frame f starts at f h - pad; 0 with snip_edges */
    uint32_t snip, remove_dc, use_energy, log_energy, htk, num_ceps, cols, layout;
    uint32_t mel_off;      /* the mel tile's place within the first LDS region: tile_frames behind a leading energy column */
    uint32_t e_off, c_off; /* the energy floats' and the cepstral tile's place in LDS */
    uint32_t has_efloor;
    float inv_w, scale2, log_efloor;
};

/* F; 0 where no frame exists */
ALAC_WF_FN uint64_t out_frames_of(uint32_t W, uint32_t hop, uint32_t snip, uint64_t T) {
    if (T < W) return 0u;
    return snip ? 1u + (T - W) / hop : (T + hop / 2u) / hop;
}

ALAC_WF_FN Tile make_tile(const Params& p, uint64_t row, uint64_t tile) {
    const alacmel::Params& m = p.m;
    Tile t{};
    t.x = m.in + row * m.in_stride;
    t.y = m.out + row * m.out_row_stride;
    t.c0 = tile * m.tile_frames;
    if (t.c0 >= m.out_frames) return t;
    const uint64_t left = m.out_frames - t.c0;
    t.count = left < m.tile_frames ? (uint32_t)left : m.tile_frames;
    t.lo = (int64_t)(t.c0 * m.hop) - p.pad;
    if (m.hop <= m.N) {
        t.span = (m.tile_frames - 1u) * m.hop + m.N;
        t.sh = (uint32_t)((int64_t)((uintptr_t)t.x >> 2) + t.lo) & 3u;
    } else {
        t.span = m.tile_frames * m.N;
    }
    return t;
}

/* xr[i] of the row x: Kaldi's reflection without snip_edges. No frame that exists reaches outside [0, T) after it; the frames
 * a tile stages behind the row's last do, and get +0.0 there (they are computed and never stored). */
ALAC_WF_FN float sample_at(const Params& p, const float* x, int64_t i) {
    const int64_t T = (int64_t)p.m.in_frames;
    if (!p.snip) {
        if (i < 0) i = -1 - i;
        else if (i >= T) i = 2 * T - 1 - i;
    }
    return (i >= 0 && i < T) ? x[i] : 0.0f;
}

/* Phase 1: work item `tid` of kThreads fills its part of stage (16-byte aligned): stage[sh + e] = xr[lo + e] for e < span
 * where h <= W, stage[f W + n] = xr[lo + f h + n] otherwise. Nothing outside [0, T) of the row is read. */
ALAC_WF_FN void stage_tile(const Params& p, const Tile& t, float* stage, uint32_t tid) {
    const uint32_t W = p.m.N;
    if (p.m.hop > W) {
        for (uint32_t e = tid; e < t.span; e += kThreads) {
            const uint32_t f = e / W;
            stage[e] = sample_at(p, t.x, t.lo + (int64_t)((uint64_t)f * p.m.hop) + (e - f * W));
        }
        return;
    }
    const uint32_t total = t.sh + t.span;
    const int64_t base = t.lo - (int64_t)t.sh; /* x + base is 16-byte aligned */
    const int64_t T = (int64_t)p.m.in_frames;
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

/* The energies: work item `tid` takes the frames tid, tid + 256, ... of the tile out of the staged image, before the mel tile
 * overwrites it. Every step is written out: nothing here may be contracted. */
ALAC_WF_FN void energy_tile(const Params& p, const Tile& t, const float* stage, float* etile, uint32_t tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t W = p.m.N;
    for (uint32_t f = tid; f < p.m.tile_frames; f += kThreads) {
        const float* xs = stage + t.sh + f * p.m.fs;
        float mean = 0.0f;
        if (p.remove_dc) {
            float s = 0.0f;
            for (uint32_t n = 0; n < W; n++) s += xs[n];
            mean = s * p.inv_w;
        }
        float e = 0.0f;
        for (uint32_t n = 0; n < W; n++) {
            const float d = xs[n] - mean;
            e = fmaf(d, d, e);
        }
        e *= p.scale2;
        if (p.log_energy) {
            e = e <= p.m.floor ? p.m.log_floor : logf(e);
            if (p.has_efloor && e < p.log_efloor) e = p.log_efloor;
        }
        etile[f] = e;
    }
}

/* fbank with an energy column: the energies into their column of the output tile [cols][tile_frames] */
ALAC_WF_FN void place_energy(const Params& p, const float* etile, float* outt, uint32_t tid) {
    const uint32_t TF = p.m.tile_frames, col = p.htk ? p.m.n_mels : 0u;
    for (uint32_t f = tid; f < TF; f += kThreads) outt[col * TF + f] = etile[f];
}

/* MFCC: work item `tid` runs the chains of the outputs i = tid, tid + 256, ... (coefficient i / tile_frames, frame i %
 * tile_frames) over the log-mel tile [n_mels][tile_frames] and puts them where they leave: ctile [cols][tile_frames]. */
ALAC_WF_FN void dct_tile(const Params& p, const float* melt, const float* etile, float* ctile, uint32_t tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t TF = p.m.tile_frames, M = p.m.n_mels, items = p.num_ceps * TF;
    for (uint32_t i = tid; i < items; i += kThreads) {
        const uint32_t c = i / TF, f = i - c * TF;
        const uint32_t col = p.htk ? (c ? c - 1u : p.num_ceps - 1u) : c;
        float v;
        if (c == 0u && p.use_energy) {
            v = etile[f];
        } else {
            const float* d = p.dct + (size_t)c * M;
            const float* lm = melt + f;
            float acc = 0.0f;
            for (uint32_t m = 0; m < M; m++) acc = fmaf(d[m], lm[m * TF], acc);
            v = p.lifter[c] * acc;
        }
        ctile[col * TF + f] = v;
    }
}

/* The store of the layout frames: element (frame c0 + f, column c) is src[c * tile_frames + f]. Where the frame stride equals
 * cols the tile's count x cols elements are one line; otherwise every frame is a line of cols. Work item `tid` stores its
 * 16-byte chunks of the absolute address space inside a line with one store each, the elements of a chunk that the line covers
 * in part one by one. */
ALAC_WF_FN void store_frames(const Params& p, const Tile& t, const float* src, uint32_t tid) {
    const uint32_t TF = p.m.tile_frames, cols = p.cols;
    const bool dense = p.frame_stride == cols;
    const uint32_t lines = dense ? 1u : t.count, len = dense ? t.count * cols : cols;
    const uint32_t cpl = (len + 6u) / 4u; /* chunks that len elements behind a lead of up to 3 can touch */
    const uint32_t items = lines * cpl;
    for (uint32_t i = tid; i < items; i += kThreads) {
        const uint32_t line = i / cpl, e0 = 4u * (i - line * cpl);
        float* dst = t.y + (t.c0 + line) * p.frame_stride;
        const uint32_t lead = (uint32_t)((uintptr_t)dst >> 2) & 3u;
        const uint32_t total = lead + len;
        if (e0 >= total) continue;
        const uint32_t g0 = line * cols; /* the line's first element, counted from the tile's (frame 0, column 0) */
        if (e0 >= lead && e0 + 4u <= total) {
            F4 v;
            for (uint32_t u = 0; u < 4u; u++) {
                const uint32_t g = g0 + e0 + u - lead, f = g / cols;
                v[u] = src[(g - f * cols) * TF + f];
            }
            *(F4*)(dst + (e0 - lead)) = v;
        } else {
            for (uint32_t u = 0; u < 4u; u++)
                if (e0 + u >= lead && e0 + u < total) {
                    const uint32_t g = g0 + e0 + u - lead, f = g / cols;
                    dst[e0 + u - lead] = src[(g - f * cols) * TF + f];
                }
        }
    }
}

/* ---- the plan: host only ------------------------------------------------------------------------------------------- */
struct Config {
    uint32_t sample_rate = 0, frame_length = 0, frame_shift = 0;
    uint32_t round_to_power_of_two = 1;
    uint32_t num_mel_bins = 0;
    uint32_t num_ceps = 0; /* 0: fbank; otherwise MFCC */
    uint32_t snip_edges = 1, remove_dc_offset = 1, window_type = kWinPovey;
    uint32_t use_log_fbank = 1, use_energy = 0, raw_energy = 1, htk_compat = 0, use_power = 1, log_energy = 1;
    uint32_t layout = kLayoutFrames;
    double preemphasis = 0.97, blackman_coeff = 0.42, low_freq = 20.0, high_freq = 0.0, energy_floor = 1.0, scale = 1.0;
    double cepstral_lifter = 22.0, dither = 0.0, vtln_warp = 1.0;
};

struct Plan {
    Config cfg;
    uint32_t W = 0, hop = 0, N = 0, K = 0, KP = 0, BP = 0, n_mels = 0, taps = 0, num_ceps = 0, cols = 0;
    uint32_t tile_frames = 0, fs = 0, a_floats = 0, lds_floats = 0, mel_off = 0, e_off = 0, c_off = 0;
    int64_t pad = 0;
    float eps = 0.0f, log_eps = 0.0f, log_efloor = 0.0f, inv_w = 0.0f, scale2 = 0.0f;
    std::vector<float> basis;   /* [2][K][W]: C, then S, folded */
    std::vector<float> bt;      /* [W][BP][4], what the device reads */
    std::vector<float> fbw;     /* [n_mels][taps] */
    std::vector<int32_t> first; /* [n_mels] */
    std::vector<float> dct;     /* [num_ceps][n_mels] */
    std::vector<float> lifter;  /* [num_ceps] */
};

inline double mel_of(double f) { return 1127.0 * std::log(1.0 + f / 700.0); }

/* the symmetric window of W samples, in double */
inline std::vector<double> window_of(uint32_t type, uint32_t W, double blackman) {
    std::vector<double> w(W, 1.0);
    if (W == 1u || type == kWinRectangular) return w;
    const double a = 2.0 * 3.14159265358979323846 / (double)(W - 1u);
    for (uint32_t n = 0; n < W; n++) {
        const double c = std::cos(a * (double)n);
        if (type == kWinHanning) w[n] = 0.5 - 0.5 * c;
        else if (type == kWinHamming) w[n] = 0.54 - 0.46 * c;
        else if (type == kWinPovey) w[n] = std::pow(0.5 - 0.5 * c, 0.85);
        else w[n] = blackman - 0.5 * c + (0.5 - blackman) * std::cos(2.0 * a * (double)n);
    }
    return w;
}

inline float round_once(double v) {
    const float r = (float)v;
    return r == 0.0f ? 0.0f : r; /* +0.0f, never -0.0f */
}

/* floats of the first LDS region of a tile of tf frames: the staged inputs with their offset within a chunk, or the output tile
 * in their place, rounded up to 4. Both transforms' lds_need begin with it. */
inline uint64_t stage_floats(const Plan& pl, uint32_t tf) {
    uint64_t a = pl.hop <= pl.W ? (uint64_t)(tf - 1u) * pl.hop + pl.W + 3u : (uint64_t)tf * pl.W;
    const uint64_t o = (uint64_t)(pl.n_mels + (pl.num_ceps == 0u && pl.cfg.use_energy ? 1u : 0u)) * tf;
    if (o > a) a = o;
    return (a + 3u) & ~(uint64_t)3u;
}

/* floats of LDS a tile of tf frames needs; the places of its parts */
inline uint64_t lds_need(const Plan& pl, uint32_t tf, uint32_t* a_floats, uint32_t* e_off, uint32_t* c_off) {
    const uint64_t a = stage_floats(pl, tf);
    uint64_t at = a + (uint64_t)tf * pl.KP;
    if (a_floats) *a_floats = (uint32_t)a;
    if (e_off) *e_off = (uint32_t)at;
    if (pl.cfg.use_energy) at += tf;
    if (c_off) *c_off = (uint32_t)at;
    at += (uint64_t)pl.num_ceps * tf;
    return at;
}

/* The plan is built in steps, each a plain function over Config / Plan, so that the FFT transform's plan (alac_fbankfft.h) takes
 * the ones it shares (config_ok, set_dims, mel_banks, dct_lifter) and leaves the direct transform's own (make_basis, fit_tile). */

/* the DFT size of a configuration: 0 where frame_length is outside [1, 2048] */
inline uint32_t n_fft_of(const Config& c) {
    if (c.frame_length < 1u || c.frame_length > kMaxFft) return 0u;
    uint32_t N = c.frame_length;
    if (c.round_to_power_of_two)
        for (N = 1u; N < c.frame_length; N *= 2u) {}
    return N;
}

/* the filterbank's band in Hz: high_freq <= 0 counts from Nyquist. false: not 0 <= low < high <= Nyquist, high > 0 */
inline bool band_of(const Config& c, double* low, double* high) {
    const double nyquist = 0.5 * (double)c.sample_rate;
    *low = c.low_freq;
    *high = c.high_freq <= 0.0 ? c.high_freq + nyquist : c.high_freq;
    return *low >= 0.0 && *low < nyquist && *high > 0.0 && *high <= nyquist && *low < *high;
}

/* false: no plan for these arguments, whatever the transform (alacgpu.h lists them) */
inline bool config_ok(const Config& c) {
    if (c.frame_length < 1u || c.frame_length > kMaxFft || c.frame_shift < 1u || !c.sample_rate) return false;
    if (c.round_to_power_of_two > 1u || c.snip_edges > 1u || c.remove_dc_offset > 1u || c.window_type > kWinBlackman ||
        c.use_log_fbank > 1u || c.use_energy > 1u || c.raw_energy > 1u || c.htk_compat > 1u || c.use_power > 1u || c.log_energy > 1u ||
        c.layout > kLayoutBins)
        return false;
    if (c.dither != 0.0 || c.vtln_warp != 1.0 || !c.use_power || (c.use_energy && !c.raw_energy)) return false;
    if (c.num_mel_bins < 1u || c.num_mel_bins > kMaxMels || c.num_ceps > c.num_mel_bins) return false;
    for (double v : {c.preemphasis, c.blackman_coeff, c.low_freq, c.high_freq, c.energy_floor, c.scale, c.cepstral_lifter})
        if (!std::isfinite(v)) return false;
    if (c.scale == 0.0 || c.energy_floor < 0.0) return false;
    const float scale2 = (float)(c.scale * c.scale);
    if (!std::isfinite(scale2) || !(scale2 > 0.0f)) return false;
    double low, high;
    return band_of(c, &low, &high);
}

/* the dimensions and constants of a fresh plan for a configuration that config_ok accepts */
inline void set_dims(const Config& c, Plan& pl) {
    pl.cfg = c;
    const uint32_t W = pl.W = c.frame_length;
    pl.N = n_fft_of(c);
    pl.hop = c.frame_shift;
    const uint32_t K = pl.K = pl.N / 2u + 1u;
    pl.KP = K | 1u;
    pl.BP = (K + 1u) / 2u;
    pl.n_mels = c.num_mel_bins;
    pl.num_ceps = c.num_ceps;
    pl.cols = c.num_ceps ? c.num_ceps : pl.n_mels + c.use_energy;
    pl.fs = pl.hop < W ? pl.hop : W;
    pl.pad = c.snip_edges ? 0 : (int64_t)(W / 2u) - (int64_t)(pl.hop / 2u);
    pl.eps = 1.1920928955078125e-07f; /* 2^-23 */
    pl.log_eps = (float)std::log((double)pl.eps);
    pl.log_efloor = c.energy_floor > 0.0 ? (float)std::log(c.energy_floor) : 0.0f;
    pl.inv_w = (float)(1.0 / (double)W);
    pl.scale2 = (float)(c.scale * c.scale);
}

/* the folded basis and bt: the direct transform's own */
inline void make_basis(Plan& pl) {
    const Config& c = pl.cfg;
    const uint32_t W = pl.W, N = pl.N, K = pl.K;
    const double pi = 3.14159265358979323846;
    const std::vector<double> win = window_of(c.window_type, W, c.blackman_coeff);
    const double pre = c.preemphasis;
    pl.basis.assign((size_t)2 * K * W, 0.0f);
    pl.bt.assign((size_t)W * pl.BP * 4u, 0.0f);
    std::vector<double> a(W), g(W);
    for (uint32_t part = 0; part < 2u; part++)
        for (uint32_t k = 0; k < K; k++) {
            for (uint32_t j = 0; j < W; j++) {
                const uint32_t r = (uint32_t)(((uint64_t)k * j) % N);
                const double ang = 2.0 * pi * (double)r / (double)N;
                a[j] = win[j] * (part ? std::sin(ang) : std::cos(ang));
            }
            double sum = 0.0;
            for (uint32_t n = 0; n < W; n++) {
                g[n] = n + 1u < W ? a[n] - pre * a[n + 1u] : a[n];
                if (n == 0u) g[0] -= pre * a[0];
                sum += g[n];
            }
            const double mean = c.remove_dc_offset ? sum / (double)W : 0.0;
            for (uint32_t n = 0; n < W; n++) {
                const float v = round_once(c.scale * (g[n] - mean));
                pl.basis[((size_t)part * K + k) * W + n] = v;
                pl.bt[((size_t)n * pl.BP + k / 2u) * 4u + 2u * (k & 1u) + part] = v;
            }
        }
}

/* get_mel_banks: first, taps and fbw. false: a filter that is not one run of weights */
inline bool mel_banks(Plan& pl) {
    const uint32_t M = pl.n_mels, N = pl.N, K = pl.K;
    double low, high;
    band_of(pl.cfg, &low, &high);
    const double m_low = mel_of(low), m_high = mel_of(high), delta = (m_high - m_low) / (double)(M + 1u);
    const uint32_t nb = N / 2u; /* bins with a weight */
    const double width = (double)pl.cfg.sample_rate / (double)N;
    std::vector<float> fb((size_t)M * K, 0.0f);
    for (uint32_t m = 0; m < M; m++) {
        const double left = m_low + (double)m * delta, centre = m_low + (double)(m + 1u) * delta;
        const double right = m_low + (double)(m + 2u) * delta;
        for (uint32_t k = 0; k < nb; k++) {
            const double mk = mel_of(width * (double)k);
            const double up = (mk - left) / (centre - left), down = (right - mk) / (right - centre);
            double v = up < down ? up : down;
            if (!(v > 0.0)) v = 0.0;
            fb[(size_t)m * K + k] = (float)v;
        }
    }
    return alacmel::compact_filters(fb, M, K, &pl.first, &pl.taps, &pl.fbw);
}

/* the DCT and the lifter of MFCC; nothing for fbank */
inline void dct_lifter(Plan& pl) {
    const Config& c = pl.cfg;
    const uint32_t M = pl.n_mels;
    if (!c.num_ceps) return;
    const double pi = 3.14159265358979323846;
    pl.dct.assign((size_t)c.num_ceps * M, 0.0f);
    pl.lifter.assign(c.num_ceps, 1.0f);
    /* row 0: sqrt(1 / M); times sqrt(2) where C0 itself leaves in the last column (htk_compat without use_energy) */
    const float row0 = round_once(std::sqrt(((c.htk_compat && !c.use_energy) ? 2.0 : 1.0) / (double)M));
    for (uint32_t q = 0; q < c.num_ceps; q++) {
        for (uint32_t m = 0; m < M; m++)
            pl.dct[(size_t)q * M + m] = q ? round_once(std::sqrt(2.0 / (double)M) * std::cos(pi * ((double)m + 0.5) * (double)q / (double)M))
                                          : row0;
        if (c.cepstral_lifter != 0.0)
            pl.lifter[q] = (float)(1.0 + 0.5 * c.cepstral_lifter * std::sin(pi * (double)q / c.cepstral_lifter));
    }
}

/* where the mel tile begins in the first LDS region: behind a leading energy column of fbank */
inline uint32_t mel_off_of(const Config& c, uint32_t tf) { return (!c.num_ceps && c.use_energy && !c.htk_compat) ? tf : 0u; }

/* the direct transform's fit: tile_frames halved from 64 until the tile fits the LDS budget, and the places of its parts.
 * false: four frames do not fit */
inline bool fit_tile(Plan& pl) {
    uint32_t tf = kMaxTile;
    while (tf > kMinTile && lds_need(pl, tf, nullptr, nullptr, nullptr) > kLdsFloats) tf /= 2u;
    const uint64_t need = lds_need(pl, tf, &pl.a_floats, &pl.e_off, &pl.c_off);
    if (need > kLdsFloats) return false;
    pl.tile_frames = tf;
    pl.lds_floats = (uint32_t)need;
    pl.mel_off = mel_off_of(pl.cfg, tf);
    return true;
}

/* false: no plan for these arguments (alacgpu.h lists them) */
inline bool make_plan(const Config& c, Plan* out) {
    if (!config_ok(c)) return false;
    Plan pl;
    set_dims(c, pl);
    make_basis(pl);
    if (!mel_banks(pl)) return false;
    dct_lifter(pl);
    if (!fit_tile(pl)) return false;
    *out = std::move(pl);
    return true;
}

/* the arguments of one pass with frames to write; false for what the entry rejects. out_inner_stride is the frame stride of
 * the layout frames, the bin stride of the layout bins. */
inline bool make_params(const Plan& pl, const float* in, uint64_t in_stride, uint64_t rows, uint64_t in_frames, float* out,
                        uint64_t out_row_stride, uint64_t out_inner_stride, const float* bt, const float* fbw, const int32_t* first,
                        const float* dct, const float* lifter, Params* p) {
    if (!in || !out || ((uintptr_t)in & 3u) || ((uintptr_t)out & 3u) || !rows) return false;
    if (in_frames > ((uint64_t)1 << 61)) return false;
    const uint64_t F = out_frames_of(pl.W, pl.hop, pl.cfg.snip_edges, in_frames);
    if (!F) return false;
    if (in_stride < in_frames) return false;
    const uint64_t lim = SIZE_MAX / 8u;
    const bool bins = pl.cfg.layout == kLayoutBins;
    const uint64_t lines = bins ? pl.cols : F, len = bins ? F : pl.cols; /* lines of len elements, out_inner_stride apart */
    if (out_inner_stride < len || out_inner_stride > lim / lines) return false;
    if (out_row_stride < (lines - 1u) * out_inner_stride + len) return false;
    if (in_stride > lim / rows || out_row_stride > lim / rows) return false;
    const uint64_t tpr = (F + pl.tile_frames - 1u) / pl.tile_frames;
    if (tpr > (~(uint64_t)0) / rows) return false;
    Params q{};
    q.m = alacmel::Params{in, in_stride, rows, in_frames, out, out_row_stride, bins ? out_inner_stride : 0u, F, (const F4*)bt, fbw,
                          first, pl.W, pl.hop, pl.K, pl.KP, pl.BP, pl.n_mels, pl.taps, pl.cols, 0u,
                          (pl.num_ceps || pl.cfg.use_log_fbank) ? (uint32_t)alacmel::kLogLn : (uint32_t)alacmel::kLogNone, pl.eps,
                          pl.log_eps, pl.tile_frames, pl.fs, pl.a_floats, tpr};
    q.dct = dct;
    q.lifter = lifter;
    q.frame_stride = bins ? 0u : out_inner_stride;
    q.pad = pl.pad;
    q.snip = pl.cfg.snip_edges;
    q.remove_dc = pl.cfg.remove_dc_offset;
    q.use_energy = pl.cfg.use_energy;
    q.log_energy = pl.cfg.log_energy;
    q.htk = pl.cfg.htk_compat;
    q.num_ceps = pl.num_ceps;
    q.cols = pl.cols;
    q.layout = pl.cfg.layout;
    q.mel_off = pl.mel_off;
    q.e_off = pl.e_off;
    q.c_off = pl.c_off;
    q.has_efloor = pl.cfg.energy_floor > 0.0 ? 1u : 0u;
    q.inv_w = pl.inv_w;
    q.scale2 = pl.scale2;
    q.log_efloor = pl.log_efloor;
    *p = q;
    return true;
}

/* One tile, the way the kernel runs it: `phase` 0 .. 4, a barrier between two phases. The kernel and the host build call
 * exactly this, so they cannot drift apart. */
ALAC_WF_FN void tile_phase(const Params& p, const Tile& t, float* lds, uint32_t phase, uint32_t tid) {
    float* ptile = lds + p.m.a_floats;
    float* etile = lds + p.e_off;
    float* ctile = lds + p.c_off;
    if (phase == 0u) {
        stage_tile(p, t, lds, tid);
    } else if (phase == 1u) {
        if (p.use_energy) energy_tile(p, t, lds, etile, tid);
        alacmel::dft_tile(p.m, t, lds, ptile, tid);
    } else if (phase == 2u) {
        alacmel::mel_tile(p.m, ptile, lds + p.mel_off, tid); /* the mel tile takes the staged inputs' place */
        if (p.use_energy && !p.num_ceps) place_energy(p, etile, lds, tid);
    } else if (phase == 3u) {
        if (p.num_ceps) dct_tile(p, lds, etile, ctile, tid);
    } else {
        const float* fin = p.num_ceps ? ctile : lds;
        if (p.layout == kLayoutBins) alacmel::store_tile(p.m, t, fin, p.m.tile_frames, 1u, tid);
        else store_frames(p, t, fin, tid);
    }
}

}  // namespace alacfb

#if defined(__HIPCC__)
/* k_fbank.hip */
namespace alack {
/* All kernels of one pass on `stream`. */
hipError_t fbank_launch(hipStream_t stream, const alacfb::Params& p, uint32_t lds_bytes);
}  // namespace alack
#endif
#endif /* ALAC_FBANK_H */
