/*
 * alac_enc.h — per-lane logic of the batch ALAC encoder (k_enc.hip), written once for the gfx950 kernels and for the
 * host build of the test-suite (tests/host_sim/enc_sim.cpp compiles this very text with g++).
 *
 * A batch is one interleaved little-endian PCM stream (the decoder's output format: 20-bit samples left-aligned in three
 * bytes, their low four bits ignored) cut into packets of frame_length frames; only the last one may be short. Every
 * packet is encoded on its own: nothing carries from one packet to the next. The encoder is the inverse of the decode
 * path, step for step the one of saprobe-alac_amd/synth/alac_synth.c:
 *
 *   shift split + mid/side mix   inverse of matrix.go:40-41,129-132
 *   adaptive predictor           inverse of predictor.go (orders other than 4/5/6/8 wrap their coefficients to int16)
 *   adaptive Golomb writer       inverse of golomb.go:112-253, MSB-first, 9-ones escape, zero runs capped at 65 535
 *
 * Policy, per element: mode 0, denShift 9, pbFactor 4, order 8, mixBits 2 / mixRes 2 for a CPE, bytesShifted
 * 0 / 0 / 1 / 2 for 16 / 20 / 24 / 32 bits; Apple's initial coefficients warmed by one adaptation pass over the element's
 * own samples (the header carries the warmed ones). An element whose compressed form is not smaller than raw is escaped.
 *
 * The stages, each a kernel (one thread or wave per item) and a loop of the host build:
 *   encode_chain   one lane per channel chain of a packet (the U and V chains of a CPE apart): warm pass, then predictor
 *                  and Golomb writer into the chain's scratch words; its bit length and coefficients
 *   build_layout   one lane per packet: escape per element, the packet's segment table (headers as literal words, the
 *                  shift block and escaped samples generated from the PCM, the chain bitstreams) and its byte size
 *   window         32 bits of a packet's bitstream at any bit position: the pack stage funnel-shifts the segments into
 *                  the dense blob, one output dword per lane
 */
#ifndef ALAC_ENC_H
#define ALAC_ENC_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/alacgpu.h"

#ifndef ALAC_ENC_FN
#if defined(__HIPCC__)
#define ALAC_ENC_FN __host__ __device__ inline
#else
#define ALAC_ENC_FN inline
#endif
#endif

namespace alacenc {

/* ---- fixed parameters of the policy ------------------------------------------------------------------------------ */
constexpr int kOrder = 8;
constexpr int kAhead = 8; /* chain inputs loaded ahead of the serial steps (encode_chain) */
constexpr uint32_t kDenShift = 9, kPbFactor = 4, kMixBits = 2;
constexpr int32_t kMixRes = 2;
constexpr int kMaxElems = 5;                 /* 8 channels: SCE CPE CPE CPE LFE */
constexpr int kMaxSegs = 4 * kMaxElems + 1;  /* per element header, shift block, U, V; END */
constexpr int kHdrWords = 12;                /* a CPE header: 23 + 32 + 16 + 2 x (16 + 16 x 8) = 359 bits */
constexpr int kLitWords = kMaxElems * kHdrWords + 4; /* + END, + a word of slack for the funnel's second read */

ALAC_ENC_FN int bytes_per_sample(int depth) { return depth == 16 ? 2 : depth == 32 ? 4 : (depth == 20 || depth == 24) ? 3 : 0; }
ALAC_ENC_FN uint32_t bytes_shifted(int depth) { return depth == 24 ? 1u : depth == 32 ? 2u : 0u; }

/* element tags per channel count (decoder.go:41-50, layout_elems of alac_synth.c): a nibble per element, 0 SCE 1 CPE 3 LFE */
ALAC_ENC_FN uint32_t layout_tags(int nch) {
    switch (nch) {
        case 1: return 0x0; case 2: return 0x1; case 3: return 0x10; case 4: return 0x010;
        case 5: return 0x110; case 6: return 0x3110; case 7: return 0x30110; default: return 0x31110;
    }
}
ALAC_ENC_FN int num_elements(int nch) {
    switch (nch) {
        case 1: case 2: return 1; case 3: return 2; case 4: case 5: return 3; case 6: return 4; default: return 5;
    }
}
/* channelLayoutOffsets (decoder.go:55-64): output channel of the k-th channel in bitstream order, a nibble each */
ALAC_ENC_FN uint32_t layout_offsets(int nch) {
    switch (nch) {
        case 1: return 0x0; case 2: return 0x10; case 3: return 0x102; case 4: return 0x3102; case 5: return 0x43102;
        case 6: return 0x354102; case 7: return 0x3654102; default: return 0x35410762;
    }
}
ALAC_ENC_FN int elem_tag(int nch, int e) { return (int)((layout_tags(nch) >> (4 * e)) & 0xf); }
ALAC_ENC_FN int out_channel(int nch, int k) { return (int)((layout_offsets(nch) >> (4 * k)) & 0xf); }

ALAC_ENC_FN int32_t sar(int32_t x, uint32_t n) { return n >= 32 ? (x < 0 ? -1 : 0) : x >> n; }
ALAC_ENC_FN uint32_t shl(uint32_t x, uint32_t n) { return n >= 32 ? 0u : x << n; }
ALAC_ENC_FN int32_t sext(int32_t x, uint32_t chan_shift) { return sar((int32_t)shl((uint32_t)x, chan_shift), chan_shift); }
ALAC_ENC_FN int32_t sign_of(int32_t v) { return (int32_t)((uint32_t)(-v) >> 31) | (v >> 31); }
ALAC_ENC_FN uint32_t lead(uint32_t m) { return m == 0 ? 32u : (uint32_t)__builtin_clz(m); }
ALAC_ENC_FN uint32_t mask_bits(uint32_t n) { return n >= 32 ? 0xffffffffu : (1u << n) - 1u; }

/* ---- what the stages share ----------------------------------------------------------------------------------------- */
struct Params {
    uint32_t frame_length;
    uint32_t depth, nch, bps, bs; /* bit depth, channels, bytes per input sample, bytesShifted */
    uint32_t pb, mb, kb;
    uint32_t chain_words;         /* scratch words per chain */
    uint64_t total_frames;
    uint64_t n_packets;
};

ALAC_ENC_FN Params make_params(const alacgpu_config& c, uint64_t total_frames) {
    Params p;
    p.frame_length = c.frame_length;
    p.depth = c.bit_depth;
    p.nch = c.num_channels;
    p.bps = (uint32_t)bytes_per_sample(c.bit_depth);
    p.bs = bytes_shifted(c.bit_depth);
    p.pb = ((uint32_t)c.pb * kPbFactor) / 4u; /* decoder.go:296-299 */
    p.mb = c.mb;
    p.kb = c.kb;
    /* a chain's stream is only kept while it is smaller than its element's escape form (<= 2 x frame_length x depth bits) */
    p.chain_words = (uint32_t)(((uint64_t)c.frame_length * c.bit_depth * 2u + 31u) / 32u + 2u);
    p.total_frames = total_frames;
    p.n_packets = c.frame_length ? (total_frames + c.frame_length - 1) / c.frame_length : 0;
    return p;
}

ALAC_ENC_FN uint32_t packet_frames(const Params& p, uint64_t pk) {
    uint64_t left = p.total_frames - pk * p.frame_length;
    return left < p.frame_length ? (uint32_t)left : p.frame_length;
}

/* One sample of the input stream in the PCM domain of the bit depth (a 20-bit sample is the top 20 of its 24 bits). */
ALAC_ENC_FN int32_t load_sample(const uint8_t* pcm, uint64_t idx, uint32_t depth) {
    if (depth == 16) {
        const uint8_t* q = pcm + idx * 2u;
        return (int32_t)(int16_t)(uint16_t)(q[0] | (q[1] << 8));
    }
    if (depth == 32) {
        const uint8_t* q = pcm + idx * 4u;
        return (int32_t)((uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24));
    }
    const uint8_t* q = pcm + idx * 3u;
    int32_t v = (int32_t)(((uint32_t)q[0] << 8) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 24)) >> 8;
    return depth == 20 ? (v >> 4) : v;
}

/* Per chain: bit length of its Golomb stream (saturates once past the escape size: the writer stops there) and the warmed
 * coefficients its header carries. */
struct ChainResult {
    uint32_t bits;
    uint32_t unencodable; /* escape the element: a zero run the decoder cannot follow (pb > 127, golomb.go:215), a frame
                             length the order-8 filter does not fit in, or KB = 0 (no code but the escape exists) */
    int16_t coefs[kOrder];
};

/* ---- MSB-first bit writer of one chain: whole dwords, byte order of the stream (word 0 = bits 0..31, bit 0 the MSB) --- */
struct BitW {
    uint32_t* words;
    uint32_t cap_words;
    uint32_t widx, acc, nacc;
    uint32_t bits;
};

ALAC_ENC_FN void bw_put(BitW& w, uint32_t val, uint32_t n) {
    if (n == 0) return;
    val &= mask_bits(n);
    const uint32_t room = 32u - w.nacc;
    if (n < room) {
        w.acc |= val << (room - n);
        w.nacc += n;
    } else {
        const uint32_t rem = n - room; /* < 32: room >= 1 */
        w.acc |= val >> rem;
        if (w.widx < w.cap_words) w.words[w.widx] = w.acc;
        w.widx++;
        w.acc = rem ? val << (32u - rem) : 0u;
        w.nacc = rem;
    }
    w.bits += n;
}
ALAC_ENC_FN void bw_flush(BitW& w) {
    if (w.nacc && w.widx < w.cap_words) w.words[w.widx] = w.acc;
}

/* One Golomb code (m, k): the inverse of dynGet32Bit (golomb.go:178-203, is_run = 0, escape literal of esc_bits) and of
 * dynGet (golomb.go:112-144, is_run = 1), as ag_put of alac_synth.c. */
ALAC_ENC_FN void ag_put(BitW& w, uint32_t x, uint32_t m, uint32_t k, uint32_t esc_bits, bool is_run) {
    uint32_t q = m ? x / m : 9u, r = m ? x % m : 0u;
    if (m == 0 && x == 0) q = 0;
    if (q >= 9) {
        bw_put(w, 0x1ffu, 9);
        bw_put(w, x & mask_bits(esc_bits), esc_bits);
        return;
    }
    bw_put(w, ((1u << q) - 1u) << 1, q + 1); /* q ones, a zero */
    if (k == 1 && !is_run) return;
    if (r == 0) {
        if (k >= 1) bw_put(w, 0, k - 1);
    } else {
        bw_put(w, r + 1u, k);
    }
}

/* Golomb state of one chain, fed one residual at a time (ag_encode of alac_synth.c as a state machine: the zero run that
 * follows a small mean is counted as the residuals arrive). */
struct Golomb {
    uint32_t mean, zmode, in_run, run, run_m, run_k;
};

ALAC_ENC_FN void ag_start(Golomb& g, uint32_t mb) {
    g.mean = mb;
    g.zmode = g.in_run = g.run = g.run_m = g.run_k = 0;
}

/* residual r at index i of n; returns false when the stream cannot be written (unencodable zero run) */
ALAC_ENC_FN bool ag_step(BitW& w, Golomb& g, int32_t r, uint32_t i, uint32_t n, uint32_t pb, uint32_t kb, uint32_t chan_bits) {
    if (g.in_run) {
        if (r == 0) {
            if (++g.run == 65535u) { /* golomb.go:243: a full run leaves zmode off */
                ag_put(w, g.run, g.run_m, g.run_k, 16, true);
                g.in_run = 0;
                g.zmode = 0;
                g.mean = 0;
            }
            return true;
        }
        ag_put(w, g.run, g.run_m, g.run_k, 16, true);
        g.in_run = 0;
        g.zmode = 1;
        g.mean = 0;
    }
    uint32_t m = g.mean >> 9;
    uint32_t k = 31u - lead(m + 3u);
    if (kb < k) k = kb;
    m = shl(1u, k) - 1u;
    const uint32_t nn = r >= 0 ? 2u * (uint32_t)r : 2u * (uint32_t)(-(int64_t)r) - 1u;
    const uint32_t x = nn - g.zmode;
    ag_put(w, x, m, k, chan_bits, false);
    g.mean = pb * nn + g.mean - ((pb * g.mean) >> 9);
    if (x > 0xffffu) g.mean = 0xffff;
    g.zmode = 0;
    if ((g.mean << 2) < 512u && i + 1u < n) {
        int32_t k32 = (int32_t)lead(g.mean) - 24 + (int32_t)((g.mean + 16u) >> 6);
        if (k32 < 0) k32 = 0;
        if (k32 > 24) return false;
        g.run_k = (uint32_t)k32;
        g.run_m = (shl(1u, g.run_k) - 1u) & (shl(1u, kb) - 1u);
        g.in_run = 1;
        g.run = 0;
    }
    return true;
}
ALAC_ENC_FN void ag_finish(BitW& w, Golomb& g) {
    if (g.in_run) ag_put(w, g.run, g.run_m, g.run_k, 16, true);
    g.in_run = 0;
}

/* ---- forward adaptive predictor: the inverse of predictor.go, streamed one sample at a time --------------------------
 * hist[0..ORDER] = the last ORDER + 1 inputs (hist[ORDER] the newest). The fixed orders 4/5/6/8 keep int32 coefficients
 * (predictor.go:107-110) and leave the last tap's del0 alone; the others wrap to int16 (:664,:675). */
template <int ORDER>
ALAC_ENC_FN int32_t predict_step(int32_t (&hist)[ORDER + 1], int32_t (&c)[ORDER], int32_t in, uint32_t chan_shift) {
    constexpr bool wrap16 = !(ORDER == 4 || ORDER == 5 || ORDER == 6 || ORDER == 8);
    constexpr int32_t den_half = 1 << (kDenShift - 1);
    const int32_t top = hist[0];
    int32_t dd[ORDER];
    int32_t acc = den_half;
#pragma unroll
    for (int j = 0; j < ORDER; j++) {
        dd[j] = top - hist[ORDER - j]; /* top - in[idx-1-j] */
        acc -= c[j] * dd[j];
    }
    const int32_t del = sext(in - top - (acc >> kDenShift), chan_shift);
    int32_t del0 = del;
    const int32_t sign = sign_of(del);
    if (sign != 0) {
        bool go = true;
#pragma unroll
        for (int j = ORDER - 1; j >= 0; j--) {
            if (go) {
                const int32_t sgn = sign > 0 ? sign_of(dd[j]) : -sign_of(dd[j]);
                c[j] -= sgn;
                if (wrap16) c[j] = (int16_t)c[j];
                if (j == 0 && !wrap16) {
                    go = false;
                } else {
                    del0 -= (ORDER - j) * ((sgn * dd[j]) >> kDenShift);
                    if (sign > 0 ? del0 <= 0 : del0 >= 0) go = false;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < ORDER; j++) hist[j] = hist[j + 1];
    hist[ORDER] = in;
    return del;
}

/* Residual of sample i of a chain (predictor state in hist / c): the first ORDER + 1 samples are a copy and differences
 * (predictor.go:53-69), the rest run the adaptive filter. */
template <int ORDER>
ALAC_ENC_FN int32_t predict(int32_t (&hist)[ORDER + 1], int32_t (&c)[ORDER], int32_t in, uint32_t i, uint32_t chan_shift) {
    if (i > (uint32_t)ORDER) return predict_step<ORDER>(hist, c, in, chan_shift);
    const int32_t prev = hist[ORDER];
#pragma unroll
    for (int j = 0; j < ORDER; j++) hist[j] = hist[j + 1];
    hist[ORDER] = in;
    return i == 0 ? in : sext(in - prev, chan_shift);
}

/* Chain input: sample i of chain `which` (0 = U / the mono channel, 1 = V) of an element whose channels are output channels
 * o (and o + 1), after the shift split and, for a CPE, the mid/side mix (inverse of matrix.go:40-41,129-132). */
ALAC_ENC_FN int32_t chain_input(const Params& p, const uint8_t* pcm, uint64_t frame, uint32_t o, bool stereo, int which,
                                uint32_t chan_shift) {
    const uint64_t base = frame * p.nch + o;
    const int32_t a = sar(load_sample(pcm, base, p.depth), 8u * p.bs);
    if (!stereo) return sext(a, chan_shift);
    const int32_t b = sar(load_sample(pcm, base + 1u, p.depth), 8u * p.bs);
    const int32_t v = a - b;
    if (which) return sext(v, chan_shift);
    return sext(b + sar(kMixRes * v, kMixBits), chan_shift);
}

struct ChainDesc {
    uint32_t elem, first_chain; /* element index, its first chain */
    uint32_t out_ch;            /* output channel of the element's first channel */
    bool stereo;
    int which;
};
ALAC_ENC_FN ChainDesc chain_desc(uint32_t nch, uint32_t chain) {
    ChainDesc d;
    uint32_t k = 0;
    d.elem = 0;
    for (int e = 0; e < num_elements((int)nch); e++) {
        const uint32_t w = elem_tag((int)nch, e) == 1 ? 2u : 1u;
        if (chain < k + w) {
            d.elem = (uint32_t)e;
            d.first_chain = k;
            break;
        }
        k += w;
    }
    d.stereo = elem_tag((int)nch, (int)d.elem) == 1;
    d.which = (int)(chain - d.first_chain);
    d.out_ch = (uint32_t)out_channel((int)nch, (int)d.first_chain);
    return d;
}

/* Apple's start (AINIT 38, BINIT -29, CINIT -2, scaled by 2^denShift / 16) warmed by one pass over the chain, then the
 * residuals of a second pass from the warmed coefficients into the Golomb writer (alac_synth.c: prepare_channel, WARM).
 * `words` holds p.chain_words words; the writer stops storing at the element's escape size. */
ALAC_ENC_FN void encode_chain(const Params& p, const uint8_t* pcm, uint64_t pk, uint32_t chain, uint32_t* words, ChainResult* out) {
    const ChainDesc d = chain_desc(p.nch, chain);
    const uint32_t num = packet_frames(p, pk);
    const uint64_t f0 = pk * p.frame_length;
    const uint32_t chan_bits = p.depth - 8u * p.bs + (d.stereo ? 1u : 0u);
    const uint32_t chan_shift = 32u - chan_bits;
    const uint64_t esc_bits = (uint64_t)num * p.depth * (d.stereo ? 2u : 1u);
    ChainResult r;
    if (p.frame_length <= (uint32_t)kOrder || p.kb == 0) {
        /* frame_length <= 8: the decoder's warm-up runs to numActive whatever the sample count and indexes buffers of
         * frame_length entries (predictor.go:58-69), so an order-8 element makes the reference panic.
         * KB = 0: k is clamped to 0, and the decoder's regular code then reads q ones, yields residual q * 0 = 0 and moves
         * on by q + 1 + (k - 1) = q bits (golomb.go:185-199): a '0' bit is never consumed and no residual but 0 has a
         * regular code. Only escaped elements decode to their samples under such a config. */
        for (int j = 0; j < kOrder; j++) r.coefs[j] = 0;
        r.bits = 0;
        r.unencodable = 1;
        *out = r;
        return;
    }

    int32_t c[kOrder], hist[kOrder + 1];
    constexpr int32_t den = 1 << kDenShift;
#pragma unroll
    for (int j = 0; j < kOrder; j++) c[j] = 0;
    c[0] = (38 * den) >> 4;
    c[1] = (-29 * den) >> 4;
    c[2] = (-2 * den) >> 4;
#pragma unroll
    for (int j = 0; j <= kOrder; j++) hist[j] = 0;
    /* the inputs of kAhead steps are loaded together, so that a step does not wait for its own load (each lane walks its
     * own packet: one memory latency per kAhead samples instead of per sample) */
    for (uint32_t i0 = 0; i0 < num; i0 += kAhead) {
        int32_t xs[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; k++)
            xs[k] = i0 + k < num ? chain_input(p, pcm, f0 + i0 + k, d.out_ch, d.stereo, d.which, chan_shift) : 0;
#pragma unroll
        for (int k = 0; k < kAhead; k++)
            if (i0 + k < num) (void)predict<kOrder>(hist, c, xs[k], i0 + k, chan_shift);
    }
#pragma unroll
    for (int j = 0; j < kOrder; j++) { /* the header's 16-bit fields are where the second pass starts from */
        r.coefs[j] = (int16_t)c[j];
        c[j] = r.coefs[j];
    }

    const uint32_t cap_bits = esc_bits < 0xffffffffull ? (uint32_t)esc_bits : 0xffffffffu;
    BitW w;
    w.words = words;
    w.cap_words = (uint32_t)((esc_bits + 31u) / 32u);
    if (w.cap_words > p.chain_words) w.cap_words = p.chain_words;
    w.widx = w.acc = w.nacc = w.bits = 0;
    Golomb g;
    ag_start(g, p.mb);
#pragma unroll
    for (int j = 0; j <= kOrder; j++) hist[j] = 0;
    r.unencodable = 0;
    bool more = true;
    for (uint32_t i0 = 0; i0 < num && more; i0 += kAhead) {
        int32_t xs[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; k++)
            xs[k] = i0 + k < num ? chain_input(p, pcm, f0 + i0 + k, d.out_ch, d.stereo, d.which, chan_shift) : 0;
#pragma unroll
        for (int k = 0; k < kAhead; k++) {
            const uint32_t i = i0 + k;
            if (more && i < num) {
                const int32_t res = predict<kOrder>(hist, c, xs[k], i, chan_shift);
                if (!ag_step(w, g, res, i, num, p.pb, p.kb, chan_bits)) {
                    r.unencodable = 1;
                    more = false;
                }
                if (w.bits >= cap_bits) more = false; /* past the escape size: the element is escaped whatever follows */
            }
        }
    }
    if (!r.unencodable && w.bits < cap_bits) ag_finish(w, g);
    bw_flush(w);
    r.bits = w.bits;
    *out = r;
}

/* ---- the packet: segments of its bitstream ------------------------------------------------------------------------- */
enum : uint32_t { kSegLit = 0, kSegStream = 1, kSegGen = 2 };
struct Seg {
    uint64_t start;  /* bit offset in the packet */
    uint32_t len;    /* bits */
    uint32_t kind;   /* kSeg* | item width << 8 | element channels << 16 | output channel << 20 (kSegGen) */
    uint64_t arg;    /* kSegLit: word of Layout::lit; kSegStream: word of the chain scratch; kSegGen: first frame */
};
struct Layout {
    Seg seg[kMaxSegs];
    uint32_t nseg;
    uint32_t bytes;          /* the packet's size */
    uint32_t escaped;        /* bit e: element e is escaped */
    uint32_t pad0;
    uint32_t lit[kLitWords]; /* element headers, END */
};

/* a small MSB-first writer into the layout's literal words */
struct LitW {
    uint32_t* w;
    uint32_t pos;
};
ALAC_ENC_FN void lit_put(LitW& l, uint32_t val, uint32_t n) {
    val &= mask_bits(n);
    const uint32_t wi = l.pos >> 5, sh = l.pos & 31u;
    const uint32_t room = 32u - sh;
    if (n <= room) {
        l.w[wi] |= n == 32 ? val : val << (room - n);
    } else {
        l.w[wi] |= val >> (n - room);
        l.w[wi + 1] |= val << (32u - (n - room));
    }
    l.pos += n;
}

ALAC_ENC_FN void add_seg(Layout& L, uint64_t& pos, uint32_t len, uint32_t kind, uint64_t arg) {
    if (len == 0) return;
    Seg& s = L.seg[L.nseg++];
    s.start = pos;
    s.len = len;
    s.kind = kind;
    s.arg = arg;
    pos += len;
}

/* One packet: escape decision per element (the compressed form is kept when the Golomb streams and the shift block are
 * smaller than the raw samples, encode_element of alac_synth.c), segment table, size. `res` = the packet's chain results,
 * `stream_word0` = scratch word of its first chain. An element is escaped whenever either of its chains is unencodable. */
ALAC_ENC_FN void build_layout(const Params& p, uint64_t pk, const ChainResult* res, uint64_t stream_word0, Layout* out) {
    Layout& L = *out; /* written in place: a private copy of its segment table would live in scratch memory on the GPU */
    L.nseg = 0;
    L.escaped = 0;
    L.pad0 = 0;
    for (int i = 0; i < kLitWords; i++) L.lit[i] = 0;
    const uint32_t num = packet_frames(p, pk);
    const uint32_t partial = num != p.frame_length ? 1u : 0u;
    const uint64_t f0 = pk * p.frame_length;
    uint64_t pos = 0;
    uint32_t chain = 0, ch = 0;
    const int ne = num_elements((int)p.nch);
    for (int e = 0; e < ne; e++) {
        const int tag = elem_tag((int)p.nch, e);
        const bool stereo = tag == 1;
        const uint32_t ech = stereo ? 2u : 1u;
        const uint32_t o = (uint32_t)out_channel((int)p.nch, (int)ch);
        const uint64_t esc_bits = (uint64_t)num * p.depth * ech;
        const uint64_t shift_bits = (uint64_t)p.bs * 8u * num * ech;
        const ChainResult& u = res[chain];
        const bool escape = u.unencodable || (stereo && res[chain + 1].unencodable) ||
                            (uint64_t)u.bits + (stereo ? res[chain + 1].bits : 0u) + shift_bits >= esc_bits;
        LitW lw;
        lw.w = L.lit + e * kHdrWords;
        lw.pos = 0;
        lit_put(lw, (uint32_t)tag, 3);
        lit_put(lw, (uint32_t)e & 0xfu, 4);
        lit_put(lw, 0, 12);
        lit_put(lw, (partial << 3) | ((escape ? 0u : p.bs) << 1) | (escape ? 1u : 0u), 4);
        if (partial) {
            lit_put(lw, num >> 16, 16);
            lit_put(lw, num & 0xffffu, 16);
        }
        if (escape) {
            L.escaped |= 1u << e;
            add_seg(L, pos, lw.pos, kSegLit, (uint64_t)e * kHdrWords);
            add_seg(L, pos, (uint32_t)esc_bits, kSegGen | (p.depth << 8) | (ech << 16) | (o << 20), f0);
        } else {
            lit_put(lw, stereo ? kMixBits : 0u, 8);
            lit_put(lw, stereo ? (uint32_t)(uint8_t)kMixRes : 0u, 8);
            for (uint32_t k = 0; k < ech; k++) {
                lit_put(lw, 0, 4); /* mode */
                lit_put(lw, kDenShift, 4);
                lit_put(lw, kPbFactor, 3);
                lit_put(lw, kOrder, 5);
                for (int j = 0; j < kOrder; j++) lit_put(lw, (uint16_t)res[chain + k].coefs[j], 16);
            }
            add_seg(L, pos, lw.pos, kSegLit, (uint64_t)e * kHdrWords);
            add_seg(L, pos, (uint32_t)shift_bits, kSegGen | ((8u * p.bs) << 8) | (ech << 16) | (o << 20), f0);
            for (uint32_t k = 0; k < ech; k++)
                add_seg(L, pos, res[chain + k].bits, kSegStream, stream_word0 + (uint64_t)(chain + k) * p.chain_words);
        }
        chain += ech;
        ch += ech;
    }
    L.lit[ne * kHdrWords] = 7u << 29; /* END */
    add_seg(L, pos, 3, kSegLit, (uint64_t)ne * kHdrWords);
    L.bytes = (uint32_t)((pos + 7u) / 8u);
}

/* 32 bits of word-stored MSB-first bits from bit `rel` on */
ALAC_ENC_FN uint32_t funnel(const uint32_t* w, uint64_t rel) {
    const uint64_t wi = rel >> 5;
    const uint32_t sh = (uint32_t)(rel & 31u);
    const uint32_t hi = w[wi];
    return sh ? (hi << sh) | (w[wi + 1] >> (32u - sh)) : hi;
}

/* bits [rel, rel + 32) of a segment, 0 <= rel < len, zero past its end */
ALAC_ENC_FN uint32_t seg_bits(const Params& p, const Seg& s, const uint32_t* lit, const uint32_t* streams, const uint8_t* pcm,
                              uint64_t rel) {
    const uint32_t kind = s.kind & 0xffu;
    uint32_t v;
    if (kind == kSegLit) {
        v = funnel(lit + s.arg, rel);
    } else if (kind == kSegStream) {
        v = funnel(streams + s.arg, rel);
    } else {
        /* fixed-width items from the PCM: frame-major, the element's channels in turn; value & mask(width) */
        const uint32_t W = (s.kind >> 8) & 0xffu, ech = (s.kind >> 16) & 0xfu, o = (s.kind >> 20) & 0xfu;
        const uint64_t items = s.len / W;
        uint64_t j = rel / W;
        const int32_t d0 = -(int32_t)(rel - j * W);
        uint64_t acc = 0;
        for (int32_t d = d0; d < 32 && j < items; d += (int32_t)W, j++) {
            const uint64_t frame = s.arg + j / ech;
            const uint32_t item = (uint32_t)load_sample(pcm, frame * p.nch + o + (uint32_t)(j % ech), p.depth) & mask_bits(W);
            acc |= (uint64_t)item << (64 - (int32_t)W - d);
        }
        v = (uint32_t)(acc >> 32);
    }
    const uint64_t left = s.len - rel;
    if (left < 32) v &= ~(0xffffffffu >> left);
    return v;
}

/* 32 bits of the packet's bitstream from bit `bitpos` on (negative: before the packet, zero there). `cursor`: the first
 * segment that may still overlap — callers walk forward through the packet, so it only grows. */
ALAC_ENC_FN uint32_t window(const Params& p, const Layout& L, const uint32_t* streams, const uint8_t* pcm, int64_t bitpos,
                            uint32_t& cursor) {
    uint32_t v = 0;
    while (cursor < L.nseg && (int64_t)(L.seg[cursor].start + L.seg[cursor].len) <= bitpos) cursor++;
    for (uint32_t i = cursor; i < L.nseg; i++) {
        const Seg& s = L.seg[i];
        const int64_t S = (int64_t)s.start;
        if (S >= bitpos + 32) break;
        if (bitpos >= S) v |= seg_bits(p, s, L.lit, streams, pcm, (uint64_t)(bitpos - S));
        else v |= seg_bits(p, s, L.lit, streams, pcm, 0) >> (uint32_t)(S - bitpos);
    }
    return v;
}

/* ---- host-side helpers of the C ABI -------------------------------------------------------------------------------- */
/* A blob capacity that always suffices: every element at most its escape size plus the largest header. */
ALAC_ENC_FN uint64_t max_bytes(const alacgpu_config& c, uint64_t total_frames) {
    if (!c.frame_length || !bytes_per_sample(c.bit_depth) || c.num_channels < 1 || c.num_channels > 8) return 0;
    const uint64_t n = (total_frames + c.frame_length - 1) / c.frame_length;
    const uint64_t per = ((uint64_t)c.frame_length * c.num_channels * c.bit_depth + 7u) / 8u +
                         (uint64_t)num_elements(c.num_channels) * 48u + 8u;
    return n * per;
}

/* ALACSpecificConfig (config.go:64-79), big-endian, compatible version 0 */
ALAC_ENC_FN void cookie(const alacgpu_config& c, uint32_t max_frame_bytes, uint32_t avg_bit_rate, uint8_t out[24]) {
    const uint32_t f[3] = {max_frame_bytes, avg_bit_rate, c.sample_rate};
    out[0] = (uint8_t)(c.frame_length >> 24);
    out[1] = (uint8_t)(c.frame_length >> 16);
    out[2] = (uint8_t)(c.frame_length >> 8);
    out[3] = (uint8_t)c.frame_length;
    out[4] = 0;
    out[5] = c.bit_depth;
    out[6] = c.pb;
    out[7] = c.mb;
    out[8] = c.kb;
    out[9] = c.num_channels;
    out[10] = (uint8_t)(c.max_run >> 8);
    out[11] = (uint8_t)c.max_run;
    for (int k = 0; k < 3; k++)
        for (int b = 0; b < 4; b++) out[12 + 4 * k + b] = (uint8_t)(f[k] >> (24 - 8 * b));
}

} /* namespace alacenc */
#endif
