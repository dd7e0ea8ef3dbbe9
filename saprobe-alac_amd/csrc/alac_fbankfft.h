/*
 * alac_fbankfft.h — the Kaldi feature pass's second, opt-in transform: the frame's steps one after the other in float32 and a
 * mixed-radix FFT out of LDS, in place of the chains over the folded basis of alac_fbank.h. Plain host + device code over
 * alac_fbank.h and alac_melfft.h: k_fbankfft.hip builds the gfx950 kernel from this text, tests/host_sim/fbankfft_sim.cpp builds
 * the same text with g++ (contraction off) for the CPU suite. Framing, staging and reflection (alacfb::make_tile, stage_tile,
 * sample_at), the passes and the split step (alacmelfft::pass_batch, split_batch), the energy, the mel chains, the log, the DCT
 * and lifter, the column arrangement and both stores (alacfb::energy_tile, alacmel::mel_tile, alacfb::place_energy, dct_tile,
 * store_frames, alacmel::store_tile) are those headers', called as they are.
 *
 * The definition. W = frame length, h = frame shift, N = the DFT size as in alac_fbank.h: the next power of two
 * >= W with round_to_power_of_two, else W. N must satisfy alacmelfft::size_ok: even, in [2, 2048], M = N / 2 = 2^a 3^b 5^c; with
 * rounding that is every W in [2, 2048], without it W itself must qualify. Any other N is no plan, never the direct transform.
 *
 *   frame    x[n], n < W: what stage_tile / sample_at deliver for the frame, as in alac_fbank.h.
 *   mean     remove_dc_offset: P = 256 / tile_frames residue classes (4 .. 64). s_j = +0.0f; s_j += x[n] for n = j, j + P, j + 2 P,
 *            .. < W upwards (a class without a sample stays +0.0f). Then the tree: for d = P / 2, P / 4, .. 1: s_j += s_{j + d}
 *            for j < d. s = s_0; mean = s / (float)W, a correctly rounded division. Without remove_dc_offset mean is +0.0f and
 *            v = x.
 *   v        v[n] = x[n] - mean
 *   y        y[n] = fmaf(-c32, v[n - 1], v[n]) with v[-1] = v[0], c32 = float(preemphasis_coefficient); c32 = 0 leaves y = v.
 *   z        z[n] = ws[n] * y[n], ws[n] = float(scale * win[n]), win = alacfb::window_of in double, the product rounded once
 *            (+0.0f where it is 0); z[n] = +0.0f for W <= n < N.
 *   pack     Z[m] = z[2 m] + i z[2 m + 1] at pos[m], m < M
 *   passes   alac_melfft.h's, and its split step and power: p[k] = |X[k]|^2, k = 0 .. M, into the power tile [tile_frames][KP]
 *   energy, mel, log, MFCC, output: alac_fbank.h's, from the staged image and the power tile. The energy column is therefore
 *            the direct handle's, bit for bit; everything behind the power tile differs from the direct handle's only through p.
 * Every float operation above is written out in this order and none is contracted: the functions run under `#pragma clang fp
 * contract(off)` (the g++ build runs with -ffp-contract=off), so up to the logs the device and a CPU build of this header agree bit
 * for bit. Frames share nothing: a NaN or an infinity stays in the frames that read it. A constant frame has v = +0.0f exactly
 * wherever s and the quotient are exact, and so +0.0f in every mel column, as Kaldi has.
 *
 * The tables: ws[N], built here; the twiddle table and pos[M], which alacmelfft::make_passes(N) builds; fbw and first, which
 * alacfb::mel_banks builds, and dct and lifter, which alacfb::dct_lifter builds: the very functions alacfb::make_plan calls, so
 * these four are the direct plan's by construction. There is no folded basis: alacfb::make_basis is not called.
 *
 * A TILE is alac_fbank.h's: tile_frames frames of one row, one workgroup of 256. LDS, in floats:
 *   [staged inputs, later the output tile: a_floats] [power tile: tile_frames * KP, rounded up to 4] [energies: tile_frames, with
 *   use_energy] [cepstral tile: num_ceps * tile_frames] [sums: 256, with remove_dc_offset] [transform buffer: batch_frames *
 *   pitch complex]
 * tile_frames is 64 halved down to 4 with batch_frames = tile_frames until that fits 64 KB; then only batch_frames halves, down to
 * 1. The phases, a barrier behind each (for_each_phase names them, for the kernel and the host build alike): stage; the energies
 * and the classes' sums (work item tid: frame tid / P, class tid % P); the tree's levels, the last of which divides; then per
 * batch that holds a frame of the row: pack (mean, pre-emphasis, window, digit reversal), the passes, the split; then mel and log,
 * the DCT for MFCC, the store.
 */
#ifndef ALAC_FBANKFFT_H
#define ALAC_FBANKFFT_H

#include "alac_fbank.h"
#include "alac_melfft.h"

namespace alacfbfft {

using alacfb::Config;
using alacmel::kLdsFloats;
using alacmel::kMaxTile;
using alacmel::kMinTile;
using alacmel::Tile;
using alacmelfft::F2;
using alacwf::kThreads;

enum : uint32_t { kDirect = 0, kFft = 1 };
enum : uint32_t { kStage = 0, kSums = 1, kTree = 2, kPack = 3, kPass = 4, kSplit = 5, kMel = 6, kDct = 7, kStore = 8 };

struct Params {
    alacfb::Params fb;      /* m.bt unused; m.N = W */
    alacmelfft::Params fft; /* m: a copy of fb.m (the split step reads KP); w32 = ws[N]; the passes, pitch and batch */
    uint32_t N;             /* the DFT size */
    uint32_t parts, log_parts; /* P = 256 / tile_frames and its log2 */
    uint32_t s_off, b_off;  /* the sums' and the transform buffer's place in LDS, floats */
    uint32_t has_pre;       /* c32 != 0 */
    float neg_c32, wf;      /* -c32; (float)W */
};

/* The classes' sums: work item `tid` sums class tid % P of frame tid / P out of the staged image into sums[tid]. */
ALAC_WF_FN void sums_tile(const Params& p, const Tile& t, const float* stage, float* sums, uint32_t tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t W = p.fb.m.N, P = p.parts;
    const uint32_t f = tid >> p.log_parts, j = tid & (P - 1u);
    const float* xs = stage + t.sh + f * p.fb.m.fs;
    float s = 0.0f;
    for (uint32_t n = j; n < W; n += P) s += xs[n];
    sums[tid] = s;
}

/* One level of the tree: s_j += s_{j + d} for j < d; the last level (d = 1) leaves mean = s / (float)W in s_0. */
ALAC_WF_FN void tree_tile(const Params& p, float* sums, uint32_t d, uint32_t tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t j = tid & (p.parts - 1u);
    if (j >= d) return;
    float s = sums[tid] + sums[tid + d];
    if (d == 1u) s = s / p.wf;
    sums[tid] = s;
}

/* Mean, pre-emphasis, window and pack: work item `tid` puts Z[m] of the frames f0 .. f0 + batch - 1 of the tile at buf[f * pitch +
 * at(pos[m])]. */
ALAC_WF_FN void pack_batch(const Params& p, const Tile& t, const float* stage, const float* sums, F2* buf, uint32_t f0, uint32_t tid) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint32_t M = p.fft.M, items = p.fft.batch * M, W = p.fb.m.N;
    for (uint32_t i = tid; i < items; i += kThreads) {
        const uint32_t f = alacmelfft::qdiv(i, M, p.fft.inv_M), m = i - f * M, n = 2u * m;
        const float* xs = stage + t.sh + (f0 + f) * p.fb.m.fs;
        F2 z;
        z[0] = 0.0f;
        z[1] = 0.0f;
        if (n < W) {
            const bool dc = p.fb.remove_dc != 0u;
            const float mean = dc ? sums[(f0 + f) << p.log_parts] : 0.0f;
            const F2 w = *(const F2*)(p.fft.w32 + n);
            const float v0 = dc ? xs[n] - mean : xs[n];
            float vm = v0; /* v[-1] = v[0] */
            if (n) vm = dc ? xs[n - 1u] - mean : xs[n - 1u];
            const float y0 = p.has_pre ? fmaf(p.neg_c32, vm, v0) : v0;
            z[0] = w[0] * y0;
            if (n + 1u < W) {
                const float v1 = dc ? xs[n + 1u] - mean : xs[n + 1u];
                const float y1 = p.has_pre ? fmaf(p.neg_c32, v0, v1) : v1;
                z[1] = w[1] * y1;
            }
        }
        buf[f * p.fft.pitch + alacmelfft::at(p.fft.pos[m])] = z;
    }
}

/* One phase of a tile for work item `tid`; `arg` is the tree's d, the batch's first frame or the pass. */
ALAC_WF_FN void tile_phase(const Params& p, const Tile& t, float* lds, uint32_t phase, uint32_t arg, uint32_t tid) {
    float* ptile = lds + p.fb.m.a_floats;
    float* sums = lds + p.s_off;
    F2* buf = (F2*)(lds + p.b_off);
    if (phase == kStage) {
        alacfb::stage_tile(p.fb, t, lds, tid);
    } else if (phase == kSums) {
        if (p.fb.use_energy) alacfb::energy_tile(p.fb, t, lds, lds + p.fb.e_off, tid);
        if (p.fb.remove_dc) sums_tile(p, t, lds, sums, tid);
    } else if (phase == kTree) {
        tree_tile(p, sums, arg, tid);
    } else if (phase == kPack) {
        pack_batch(p, t, lds, sums, buf, arg, tid);
    } else if (phase == kPass) {
        alacmelfft::pass_batch(p.fft, arg, buf, tid);
    } else if (phase == kSplit) {
        alacmelfft::split_batch(p.fft, buf, ptile, arg, tid);
    } else if (phase == kMel) {
        alacfb::tile_phase(p.fb, t, lds, 2u, tid); /* mel, log, the energy's column of fbank */
    } else if (phase == kDct) {
        alacfb::tile_phase(p.fb, t, lds, 3u, tid);
    } else {
        alacfb::tile_phase(p.fb, t, lds, 4u, tid);
    }
}

/* The phases of a tile in order: each(phase, arg) runs one for every work item and ends in a barrier. The kernel and the host
 * build call exactly this, so they cannot drift apart. Only the batches that hold a frame of the row run: behind them the power
 * tile's rows keep what LDS held, and what the later phases make of those is never stored. */
template <typename Each>
ALAC_WF_FN void for_each_phase(const Params& p, const Tile& t, Each&& each) {
    each((uint32_t)kStage, 0u);
    if (p.fb.use_energy || p.fb.remove_dc) each((uint32_t)kSums, 0u);
    if (p.fb.remove_dc)
        for (uint32_t d = p.parts / 2u; d >= 1u; d /= 2u) each((uint32_t)kTree, d);
    for (uint32_t f0 = 0; f0 < t.count; f0 += p.fft.batch) { /* t.count is uniform */
        each((uint32_t)kPack, f0);
        for (uint32_t s = 0; s < p.fft.n_pass; s++) each((uint32_t)kPass, s);
        each((uint32_t)kSplit, f0);
    }
    each((uint32_t)kMel, 0u);
    if (p.fb.num_ceps) each((uint32_t)kDct, 0u);
    each((uint32_t)kStore, 0u);
}

/* ---- the plan: host only ------------------------------------------------------------------------------------------- */
struct Plan {
    alacfb::Plan base;    /* without a basis (basis, bt empty); tile_frames, the offsets and lds_floats are this transform's own */
    alacmelfft::Plan fft; /* what alacmelfft::make_passes(N) fills; its base is unused */
    uint32_t batch = 0, parts = 0, log_parts = 0, p_floats = 0, s_off = 0, b_off = 0;
    float c32 = 0.0f;
    std::vector<float> ws; /* [N] */
};

/* floats of LDS a tile of tf frames, transformed `batch` at a time, needs; the places of its parts */
inline uint64_t lds_need(const Plan& pl, uint32_t tf, uint32_t batch, uint32_t* a_floats, uint32_t* p_floats, uint32_t* e_off,
                         uint32_t* c_off, uint32_t* s_off, uint32_t* b_off) {
    const alacfb::Plan& b = pl.base;
    const uint64_t a = alacfb::stage_floats(b, tf);
    const uint64_t pt = ((uint64_t)tf * b.KP + 3u) & ~(uint64_t)3u; /* rounded up to 4, which the direct plan's is not */
    uint64_t at = a + pt;
    if (a_floats) *a_floats = (uint32_t)a;
    if (p_floats) *p_floats = (uint32_t)pt;
    if (e_off) *e_off = (uint32_t)at;
    if (b.cfg.use_energy) at += tf;
    if (c_off) *c_off = (uint32_t)at;
    at += (uint64_t)b.num_ceps * tf;
    if (s_off) *s_off = (uint32_t)at;
    if (b.cfg.remove_dc_offset) at += kThreads;
    if (b_off) *b_off = (uint32_t)at; /* a multiple of 4: every part before it is one */
    return at + (uint64_t)2u * batch * pl.fft.pitch;
}

using alacfb::n_fft_of; /* the DFT size of a configuration: k_fbank.hip asks for it under this name */

/* false: no plan: a configuration that alacfb::config_ok refuses, an N that size_ok refuses, a filter that is not one run, or
 * four frames with one in the transform buffer that do not fit the LDS budget. The checks, the dimensions, the filterbank, the
 * DCT and the lifter are alac_fbank.h's steps, the ones alacfb::make_plan runs; ws, c32, the passes and the fit are this
 * transform's own. It never passes through the direct transform's basis or fit: base.basis and base.bt stay empty. */
inline bool make_plan(const Config& c, Plan* out) {
    if (!alacfb::config_ok(c) || !alacmelfft::size_ok(n_fft_of(c))) return false;
    Plan plan;
    alacfb::Plan& pl = plan.base;
    alacfb::set_dims(c, pl);

    /* the window times the scale, rounded once */
    const std::vector<double> win = alacfb::window_of(c.window_type, pl.W, c.blackman_coeff);
    plan.ws.assign(pl.N, 0.0f);
    for (uint32_t n = 0; n < pl.W; n++) plan.ws[n] = alacfb::round_once(c.scale * win[n]);
    plan.c32 = (float)c.preemphasis;
    if (!alacmelfft::make_passes(pl.N, &plan.fft) || !alacfb::mel_banks(pl)) return false;
    alacfb::dct_lifter(pl);

    uint32_t tf = kMaxTile;
    while (tf > kMinTile && lds_need(plan, tf, tf, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) > kLdsFloats) tf /= 2u;
    uint32_t batch = tf;
    while (batch > 1u && lds_need(plan, tf, batch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) > kLdsFloats) batch /= 2u;
    const uint64_t need = lds_need(plan, tf, batch, &pl.a_floats, &plan.p_floats, &pl.e_off, &pl.c_off, &plan.s_off, &plan.b_off);
    if (need > kLdsFloats) return false;
    pl.tile_frames = tf;
    pl.lds_floats = (uint32_t)need;
    pl.mel_off = alacfb::mel_off_of(c, tf);
    plan.batch = batch;
    plan.parts = kThreads / tf;
    for (plan.log_parts = 0u; (1u << plan.log_parts) < plan.parts; plan.log_parts++) {}
    *out = std::move(plan);
    return true;
}

/* the arguments of one pass with frames to write; false for what the entry rejects (alacfb::make_params) */
inline bool make_params(const Plan& pl, const float* in, uint64_t in_stride, uint64_t rows, uint64_t in_frames, float* out,
                        uint64_t out_row_stride, uint64_t out_inner_stride, const float* ws, const float* tw, const uint32_t* pos,
                        const float* fbw, const int32_t* first, const float* dct, const float* lifter, Params* p) {
    Params q{};
    if (!alacfb::make_params(pl.base, in, in_stride, rows, in_frames, out, out_row_stride, out_inner_stride, nullptr, fbw, first, dct,
                             lifter, &q.fb))
        return false;
    q.fft.m = q.fb.m;
    alacmelfft::fill_params(pl.fft, pl.batch, pl.p_floats, ws, tw, pos, &q.fft);
    q.N = pl.base.N;
    q.parts = pl.parts;
    q.log_parts = pl.log_parts;
    q.s_off = pl.s_off;
    q.b_off = pl.b_off;
    q.has_pre = pl.c32 != 0.0f ? 1u : 0u;
    q.neg_c32 = -pl.c32;
    q.wf = (float)pl.base.W;
    *p = q;
    return true;
}

}  // namespace alacfbfft

#if defined(__HIPCC__)
/* k_fbankfft.hip */
namespace alack {
/* All kernels of one pass on `stream`. */
hipError_t fbankfft_launch(hipStream_t stream, const alacfbfft::Params& p, uint32_t lds_bytes);
}  // namespace alack
#endif
#endif /* ALAC_FBANKFFT_H */
