/*
 * alac_melfft.h — the spectrogram pass's second, opt-in transform: a mixed-radix FFT out of LDS in place of the basis walk of
 * alac_mel.h. Plain host + device code over alac_mel.h: k_melfft.hip builds the gfx950 kernel from this text,
 * tests/host_sim/melfft_sim.cpp builds the same text with g++ (contraction off) for the CPU suite. Framing, reflection, the
 * power tile, the mel chains, the log, the store and the output layout are alac_mel.h's, called as they are.
 *
 * The definition. N = n_fft even in [2, 2048], M = N / 2 = 2^a 3^b 5^c; any other N is no plan.
 *
 *   window   w32[n] = float(w[n]), w the direct pass's window in double (alacmel::hann_window, the one both plans call):
 *            periodic Hann of W at offset (N - W) / 2 ([1.0] for W = 1), +0.0f elsewhere.  v[n] = w32[n] * x~[n], one float32
 *            product; x~ is what stage_tile / sample_at deliver.
 *   pack     z[m] = v[2 m] + i v[2 m + 1], m < M: a real transform of N through a complex one of M, one frame at a time.
 *   passes   radices r_0 .. r_{P-1} (the 5s, then the 3s, then the 4s, then a 2), L_s = r_0 .. r_{s-1}. Decimation in time, in
 *            place: z[m] is put at pos(m), pos over [r_0 .. r_s](n) = (n mod r_s) L_s + pos over [r_0 .. r_{s-1}](n / r_s), so
 *            that pass s takes its r legs b[g L r + k + q L], q < r (g < M / (L r), k < L), multiplies leg q >= 1 by
 *            tw_s[k][q - 1] = exp(-2 pi i ((q k) mod (L r)) / (L r)) (not in pass 0, where L = 1 and every twiddle is 1), runs
 *            the r-point butterfly and writes the r results where the legs were. After the last pass b[k] = Z[k].
 *   cmul     (a * w).re = fmaf(a.re, w.re, -(a.im * w.im)),  .im = fmaf(a.re, w.im, a.im * w.re)
 *   radix 2  y0 = a + b, y1 = a - b
 *   radix 4  t0 = a + c, t1 = a - c, t2 = b + d, t3 = b - d;  y0 = t0 + t2, y2 = t0 - t2, y1 = (t1.re + t3.im, t1.im - t3.re),
 *            y3 = (t1.re - t3.im, t1.im + t3.re)
 *   radix 3  t = b + c, d = b - c, y0 = a + t, m = fmaf(-0.5, t, a) per component;  y1 = (fmaf(s3, d.im, m.re), fmaf(-s3, d.re,
 *            m.im)),  y2 = (fmaf(-s3, d.im, m.re), fmaf(s3, d.re, m.im)),  s3 = sin(2 pi / 3)
 *   radix 5  t1 = b + e, t2 = c + d, t3 = b - e, t4 = c - d;  y0 = a + (t1 + t2);  m1 = fmaf(c2, t2, fmaf(c1, t1, a)),  m2 =
 *            fmaf(c1, t2, fmaf(c2, t1, a)),  n1 = fmaf(s2, t4, s1 * t3),  n2 = fmaf(-s1, t4, s2 * t3) per component;  y1 =
 *            (m1.re + n1.im, m1.im - n1.re), y4 = (m1.re - n1.im, m1.im + n1.re), y2 and y3 likewise from m2, n2;  c1, s1 = cos,
 *            sin(2 pi / 5), c2, s2 = cos, sin(4 pi / 5)
 *   split    k = 0 .. M:  A = Z[k mod M], B = conj Z[(M - k) mod M], t = t[k] = exp(-2 pi i k / N);
 *            e = 0.5 (A + B), d = A - B, o = (0.5 d.im, -0.5 d.re)                                  ((A - B) / (2 i))
 *            X.re = fmaf(-t.im, o.im, fmaf(t.re, o.re, e.re)),  X.im = fmaf(t.im, o.re, fmaf(t.re, o.im, e.im))
 *   power    p[k] = fmaf(X.im, X.im, X.re * X.re)
 * Every twiddle and root constant is a float32 table entry: the integer reduction first, (2 pi r) / n, cos and sin in double,
 * rounded once (a twiddle is stored as {cos, -sin}). Every float operation above is written out in this order and none is
 * contracted: the functions run under `#pragma clang fp contract(off)` (the g++ build runs with -ffp-contract=off), so up to the
 * log the device and a CPU build of this header agree bit for bit. Frames do not share a transform: a NaN or an infinity stays
 * in the frames that contain it.
 *
 * The tables. twiddle = [8 roots: -0.5, s3, c1, s1, c2, s2, 0, 0] [pass 0: L (r - 1) complex] .. [pass P - 1] [t[0 .. M]: M + 1
 * complex], floats; window = w32[N]; pos[M] (uint32) is derived from the radices and not reported. make_passes builds the
 * twiddle table and pos, make_plan the window; fbw and first are alacmel::make_plan's, which this plan runs without its basis.
 * fill_params hands them to the device, for this pass and for alac_fbankfft.h's.
 *
 * A TILE is alac_mel.h's: tile_frames frames of one row, one workgroup of 256, staged by stage_tile. Its frames are transformed
 * `batch` at a time (batch = tile_frames except at the largest N, where the buffer of a whole tile does not fit): pack (window
 * and digit reversal, out of the staged image into the transform buffer), barrier, the passes with the whole workgroup over all
 * butterflies of the batch and a barrier behind each, the split step into the power tile [tile_frames][KP], barrier. Only the
 * batches that hold a frame of the row run: behind them the power tile's rows keep what LDS held, and what mel_tile or log_tile
 * make of those is never stored. A pass is
 * in place butterfly by butterfly (a work item reads its r legs, computes, writes them back), so no second buffer exists. LDS:
 * [staged inputs / output tile: a_floats] [power tile: tile_frames * KP, rounded up to 4] [transform buffer: batch frames of
 * `pitch` complex]. Element a of a frame lies at a + (a >> 4): a power-of-two stride of 4, 8, 16 .. complex between the lanes of
 * a wave would otherwise fall on few banks; pitch = M + (M - 1 >> 4), made odd.
 */
#ifndef ALAC_MELFFT_H
#define ALAC_MELFFT_H

#include "alac_mel.h"

namespace alacmelfft {

using alacmel::kLdsFloats;
using alacmel::kMaxTile;
using alacmel::kMinTile;
using alacmel::Tile;
using alacwf::kThreads;

constexpr uint32_t kMaxPasses = 8, kRootFloats = 8;
enum : uint32_t { kDirect = 0, kFft = 1 };

/* one complex number, 8 bytes moved by one instruction */
typedef float F2 __attribute__((vector_size(8), may_alias));

struct Pass {
    uint32_t r, L;        /* the radix; the length of the transforms it joins */
    uint32_t per;         /* butterflies of a frame: M / r */
    uint32_t inv_per, inv_L;
    uint32_t tw;          /* where its twiddles [L][r - 1] begin in the table, floats */
};

struct Params {
    alacmel::Params m;    /* bt unused */
    const float* w32;     /* [N], 8-byte aligned */
    const float* tw;      /* the twiddle table, 8-byte aligned */
    const uint32_t* pos;  /* [M] */
    uint32_t M, pitch, batch, p_floats, n_pass, split; /* split: where t[0 .. M] begins in the table, floats */
    uint32_t inv_M, inv_M1;
    float s3, c1, s1, c2, s2;
    Pass pass[kMaxPasses];
};

/* i / d for i < 2^16 and 1 <= d <= 2^11, inv = ceil(2^32 / d): the product's error i (inv d - 2^32) stays below 2^32 */
ALAC_WF_FN uint32_t qdiv(uint32_t i, uint32_t d, uint32_t inv) { return d == 1u ? i : (uint32_t)(((uint64_t)i * inv) >> 32); }

/* where element a of a frame lies in the transform buffer */
ALAC_WF_FN uint32_t at(uint32_t a) { return a + (a >> 4); }

ALAC_WF_FN F2 cmul(const F2 a, const F2 w) {
#pragma clang fp contract(off)
    F2 r;
    r[0] = fmaf(a[0], w[0], -(a[1] * w[1]));
    r[1] = fmaf(a[0], w[1], a[1] * w[0]);
    return r;
}

/* Window and pack: work item `tid` puts z[m] of the frames f0 .. f0 + batch - 1 of the tile at buf[f * pitch + at(pos[m])]. */
ALAC_WF_FN void pack_batch(const Params& p, const Tile& t, const float* stage, F2* buf, uint32_t f0, uint32_t tid) {
#pragma clang fp contract(off)
    const uint32_t M = p.M, items = p.batch * M;
    for (uint32_t i = tid; i < items; i += kThreads) {
        const uint32_t f = qdiv(i, M, p.inv_M), m = i - f * M;
        const float* xs = stage + t.sh + (f0 + f) * p.m.fs + 2u * m;
        const F2 w = *(const F2*)(p.w32 + 2u * m);
        F2 z;
        z[0] = w[0] * xs[0];
        z[1] = w[1] * xs[1];
        buf[f * p.pitch + at(p.pos[m])] = z;
    }
}

ALAC_WF_FN void radix2(F2* b, uint32_t i0, uint32_t L, const F2* tw, bool first) {
#pragma clang fp contract(off)
    F2* p0 = b + at(i0);
    F2* p1 = b + at(i0 + L);
    const F2 a = *p0;
    F2 c = *p1;
    if (!first) c = cmul(c, tw[0]);
    *p0 = a + c;
    *p1 = a - c;
}

ALAC_WF_FN void radix4(F2* b, uint32_t i0, uint32_t L, const F2* tw, bool first) {
#pragma clang fp contract(off)
    F2* p0 = b + at(i0);
    F2* p1 = b + at(i0 + L);
    F2* p2 = b + at(i0 + 2u * L);
    F2* p3 = b + at(i0 + 3u * L);
    const F2 a = *p0;
    F2 x1 = *p1, x2 = *p2, x3 = *p3;
    if (!first) {
        x1 = cmul(x1, tw[0]);
        x2 = cmul(x2, tw[1]);
        x3 = cmul(x3, tw[2]);
    }
    const F2 t0 = a + x2, t1 = a - x2, t2 = x1 + x3, t3 = x1 - x3;
    F2 y1, y3;
    y1[0] = t1[0] + t3[1];
    y1[1] = t1[1] - t3[0];
    y3[0] = t1[0] - t3[1];
    y3[1] = t1[1] + t3[0];
    *p0 = t0 + t2;
    *p1 = y1;
    *p2 = t0 - t2;
    *p3 = y3;
}

ALAC_WF_FN void radix3(const Params& p, F2* b, uint32_t i0, uint32_t L, const F2* tw, bool first) {
#pragma clang fp contract(off)
    F2* p0 = b + at(i0);
    F2* p1 = b + at(i0 + L);
    F2* p2 = b + at(i0 + 2u * L);
    const F2 a = *p0;
    F2 x1 = *p1, x2 = *p2;
    if (!first) {
        x1 = cmul(x1, tw[0]);
        x2 = cmul(x2, tw[1]);
    }
    const F2 t = x1 + x2, d = x1 - x2;
    F2 m, y1, y2;
    m[0] = fmaf(-0.5f, t[0], a[0]);
    m[1] = fmaf(-0.5f, t[1], a[1]);
    y1[0] = fmaf(p.s3, d[1], m[0]);
    y1[1] = fmaf(-p.s3, d[0], m[1]);
    y2[0] = fmaf(-p.s3, d[1], m[0]);
    y2[1] = fmaf(p.s3, d[0], m[1]);
    *p0 = a + t;
    *p1 = y1;
    *p2 = y2;
}

ALAC_WF_FN void radix5(const Params& p, F2* b, uint32_t i0, uint32_t L, const F2* tw, bool first) {
#pragma clang fp contract(off)
    F2* p0 = b + at(i0);
    F2* p1 = b + at(i0 + L);
    F2* p2 = b + at(i0 + 2u * L);
    F2* p3 = b + at(i0 + 3u * L);
    F2* p4 = b + at(i0 + 4u * L);
    const F2 a = *p0;
    F2 x1 = *p1, x2 = *p2, x3 = *p3, x4 = *p4;
    if (!first) {
        x1 = cmul(x1, tw[0]);
        x2 = cmul(x2, tw[1]);
        x3 = cmul(x3, tw[2]);
        x4 = cmul(x4, tw[3]);
    }
    const F2 t1 = x1 + x4, t2 = x2 + x3, t3 = x1 - x4, t4 = x2 - x3;
    F2 m1, m2, n1, n2, y1, y2, y3, y4;
    for (uint32_t c = 0; c < 2u; c++) {
        m1[c] = fmaf(p.c2, t2[c], fmaf(p.c1, t1[c], a[c]));
        m2[c] = fmaf(p.c1, t2[c], fmaf(p.c2, t1[c], a[c]));
        n1[c] = fmaf(p.s2, t4[c], p.s1 * t3[c]);
        n2[c] = fmaf(-p.s1, t4[c], p.s2 * t3[c]);
    }
    y1[0] = m1[0] + n1[1];
    y1[1] = m1[1] - n1[0];
    y4[0] = m1[0] - n1[1];
    y4[1] = m1[1] + n1[0];
    y2[0] = m2[0] + n2[1];
    y2[1] = m2[1] - n2[0];
    y3[0] = m2[0] - n2[1];
    y3[1] = m2[1] + n2[0];
    *p0 = a + (t1 + t2);
    *p1 = y1;
    *p2 = y2;
    *p3 = y3;
    *p4 = y4;
}

/* Pass s over the batch: work item `tid` runs the butterflies i = tid, tid + 256, .. (frame i / per, butterfly i % per = g L +
 * k), each in place. */
ALAC_WF_FN void pass_batch(const Params& p, uint32_t s, F2* buf, uint32_t tid) {
    const Pass ps = p.pass[s];
    const uint32_t items = p.batch * ps.per, r = ps.r, L = ps.L;
    const bool first = L == 1u;
    const F2* table = (const F2*)(p.tw + ps.tw);
    for (uint32_t i = tid; i < items; i += kThreads) {
        const uint32_t f = qdiv(i, ps.per, ps.inv_per), j = i - f * ps.per;
        const uint32_t g = qdiv(j, L, ps.inv_L), k = j - g * L;
        F2* b = buf + f * p.pitch;
        const uint32_t i0 = g * L * r + k;
        const F2* tw = table + k * (r - 1u);
        if (r == 4u) radix4(b, i0, L, tw, first);
        else if (r == 2u) radix2(b, i0, L, tw, first);
        else if (r == 3u) radix3(p, b, i0, L, tw, first);
        else radix5(p, b, i0, L, tw, first);
    }
}

/* The split step: work item `tid` turns Z of the batch's frames into the powers p[0 .. M] of the rows f0 .. of ptile. */
ALAC_WF_FN void split_batch(const Params& p, const F2* buf, float* ptile, uint32_t f0, uint32_t tid) {
#pragma clang fp contract(off)
    const uint32_t M = p.M, M1 = M + 1u, items = p.batch * M1;
    const F2* tk = (const F2*)(p.tw + p.split);
    for (uint32_t i = tid; i < items; i += kThreads) {
        const uint32_t f = qdiv(i, M1, p.inv_M1), k = i - f * M1;
        const F2* b = buf + f * p.pitch;
        const F2 A = b[at(k == M ? 0u : k)], Bc = b[at(k == 0u ? 0u : M - k)], t = tk[k];
        const float br = Bc[0], bi = -Bc[1];
        const float er = 0.5f * (A[0] + br), ei = 0.5f * (A[1] + bi);
        const float dr = A[0] - br, di = A[1] - bi;
        const float o_r = 0.5f * di, o_i = -0.5f * dr;
        float xr = fmaf(t[0], o_r, er);
        xr = fmaf(-t[1], o_i, xr);
        float xi = fmaf(t[0], o_i, ei);
        xi = fmaf(t[1], o_r, xi);
        ptile[(f0 + f) * p.m.KP + k] = fmaf(xi, xi, xr * xr);
    }
}

/* ---- the plan: host only ------------------------------------------------------------------------------------------- */
struct Plan {
    alacmel::Plan base;  /* without a basis; tile_frames, a_floats and lds_floats are this transform's own */
    uint32_t M = 0, n_pass = 0, pitch = 0, batch = 0, p_floats = 0, split = 0;
    uint32_t radix[kMaxPasses] = {};
    Pass pass[kMaxPasses] = {};
    std::vector<float> w32;    /* [N] */
    std::vector<float> tw;     /* roots, the passes' twiddles, t[0 .. M] */
    std::vector<uint32_t> pos; /* [M] */
};

/* true: n_fft is even and n_fft / 2 = 2^a 3^b 5^c */
inline bool size_ok(uint32_t n_fft) {
    if (n_fft < 2u || (n_fft & 1u) || n_fft > alacmel::kMaxFft) return false;
    uint32_t m = n_fft / 2u;
    for (uint32_t r : {2u, 3u, 5u})
        while (m % r == 0u) m /= r;
    return m == 1u;
}

inline uint32_t inv_of(uint32_t d) { return d <= 1u ? 0u : (uint32_t)((((uint64_t)1 << 32) + d - 1u) / d); }

inline uint64_t lds_need(const Plan& pl, uint32_t tf, uint32_t batch, uint32_t* a_floats, uint32_t* p_floats) {
    uint32_t a = 0;
    const uint64_t direct = alacmel::lds_need(pl.base, tf, &a); /* a + tf * KP */
    const uint64_t pt = ((direct - a) + 3u) & ~(uint64_t)3u;
    if (a_floats) *a_floats = a;
    if (p_floats) *p_floats = (uint32_t)pt;
    return a + pt + (uint64_t)2u * batch * pl.pitch;
}

/* The transform of size N alone (size_ok(N)): M, the radices and passes, the twiddle table with `split`, pos and the pitch of
 * *pl; nothing else of it is touched. false: more passes than kMaxPasses. alac_fbankfft.h's plan calls it as well. */
inline bool make_passes(uint32_t N, Plan* out) {
    Plan& pl = *out;
    const uint32_t M = pl.M = N / 2u;
    const double pi = 3.14159265358979323846;

    uint32_t left = M;
    for (uint32_t r : {5u, 3u, 4u, 2u})
        while (left % r == 0u) {
            if (pl.n_pass == kMaxPasses) return false;
            pl.radix[pl.n_pass++] = r;
            left /= r;
        }

    pl.tw.assign(kRootFloats, 0.0f);
    pl.tw[0] = -0.5f;
    pl.tw[1] = (float)std::sin(2.0 * pi / 3.0);
    pl.tw[2] = (float)std::cos(2.0 * pi / 5.0);
    pl.tw[3] = (float)std::sin(2.0 * pi / 5.0);
    pl.tw[4] = (float)std::cos(2.0 * pi * 2.0 / 5.0);
    pl.tw[5] = (float)std::sin(2.0 * pi * 2.0 / 5.0);
    uint32_t L = 1u;
    for (uint32_t s = 0; s < pl.n_pass; s++) {
        const uint32_t r = pl.radix[s], n = L * r;
        pl.pass[s] = Pass{r, L, M / r, inv_of(M / r), inv_of(L), (uint32_t)pl.tw.size()};
        for (uint32_t k = 0; k < L; k++)
            for (uint32_t q = 1; q < r; q++) {
                const double ang = 2.0 * pi * (double)((q * k) % n) / (double)n;
                pl.tw.push_back((float)std::cos(ang));
                pl.tw.push_back((float)-std::sin(ang));
            }
        L = n;
    }
    pl.split = (uint32_t)pl.tw.size();
    for (uint32_t k = 0; k <= M; k++) {
        const double ang = 2.0 * pi * (double)(k % N) / (double)N;
        pl.tw.push_back((float)std::cos(ang));
        pl.tw.push_back((float)-std::sin(ang));
    }

    pl.pos.assign(M, 0u);
    for (uint32_t m = 0; m < M; m++) {
        uint32_t n = m, at_ = 0;
        for (uint32_t s = pl.n_pass; s-- > 0u;) {
            at_ += (n % pl.radix[s]) * pl.pass[s].L;
            n /= pl.radix[s];
        }
        pl.pos[m] = at_;
    }

    pl.pitch = (M + ((M - 1u) >> 4)) | 1u;
    return true;
}

/* false: no plan: what alacmel::make_plan refuses, an n_fft that is odd or whose half has a prime factor above 5, or four
 * frames that do not fit the LDS budget */
inline bool make_plan(const alacmel::Config& c, Plan* out) {
    if (!size_ok(c.n_fft)) return false;
    Plan pl;
    if (!alacmel::make_plan(c, &pl.base, false)) return false;
    const uint32_t N = pl.base.N;

    const std::vector<double> w = alacmel::hann_window(N, pl.base.W);
    pl.w32.resize(N);
    for (uint32_t n = 0; n < N; n++) pl.w32[n] = (float)w[n];

    if (!make_passes(N, &pl)) return false;
    uint32_t tf = kMaxTile;
    while (tf > kMinTile && lds_need(pl, tf, tf, nullptr, nullptr) > kLdsFloats) tf /= 2u;
    uint32_t batch = tf;
    while (batch > 1u && lds_need(pl, tf, batch, nullptr, nullptr) > kLdsFloats) batch /= 2u;
    const uint64_t need = lds_need(pl, tf, batch, &pl.base.a_floats, &pl.p_floats);
    if (need > kLdsFloats) return false;
    pl.base.tile_frames = tf;
    pl.base.lds_floats = (uint32_t)need;
    pl.batch = batch;
    *out = std::move(pl);
    return true;
}

/* Everything of *q behind Params::m: the three device tables (a window [N], the twiddle table, pos) and what make_passes left in
 * pl, with the batch and the power tile's size that the caller's fit arrived at. alac_fbankfft.h's make_params calls it as well,
 * with its own window and fit. */
inline void fill_params(const Plan& pl, uint32_t batch, uint32_t p_floats, const float* w32, const float* tw, const uint32_t* pos,
                        Params* q) {
    q->w32 = w32;
    q->tw = tw;
    q->pos = pos;
    q->M = pl.M;
    q->pitch = pl.pitch;
    q->batch = batch;
    q->p_floats = p_floats;
    q->n_pass = pl.n_pass;
    q->split = pl.split;
    q->inv_M = inv_of(pl.M);
    q->inv_M1 = inv_of(pl.M + 1u);
    q->s3 = pl.tw[1];
    q->c1 = pl.tw[2];
    q->s1 = pl.tw[3];
    q->c2 = pl.tw[4];
    q->s2 = pl.tw[5];
    for (uint32_t s = 0; s < kMaxPasses; s++) q->pass[s] = pl.pass[s];
}

/* the arguments of one pass with frames to write; false for what the entry rejects (alacmel::make_params) */
inline bool make_params(const Plan& pl, const float* in, uint64_t in_stride, uint64_t rows, uint64_t in_frames, float* out,
                        uint64_t out_row_stride, uint64_t out_bin_stride, const float* w32, const float* tw, const uint32_t* pos,
                        const float* fbw, const int32_t* first, Params* p) {
    Params q{};
    if (!alacmel::make_params(pl.base, in, in_stride, rows, in_frames, out, out_row_stride, out_bin_stride, nullptr, fbw, first, &q.m))
        return false;
    fill_params(pl, pl.batch, pl.p_floats, w32, tw, pos, &q);
    *p = q;
    return true;
}

}  // namespace alacmelfft

#if defined(__HIPCC__)
/* k_melfft.hip */
namespace alack {
/* All kernels of one pass on `stream`. */
hipError_t melfft_launch(hipStream_t stream, const alacmelfft::Params& p, uint32_t lds_bytes);
}  // namespace alack
#endif
#endif /* ALAC_MELFFT_H */
