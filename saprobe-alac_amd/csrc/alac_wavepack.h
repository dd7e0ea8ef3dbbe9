/*
 * alac_wavepack.h — planar float32 / int32 waveforms -> the encoder's interleaved PCM: the per-sample quantise and pack,
 * the index arithmetic and the two phases of a tile, as plain host + device code. It is the inverse of alac_waveform.h.
 * k_wavepack.hip builds the gfx950 kernel from this text; tests/host_sim/pack_sim.cpp builds the same text with g++ for
 * the CPU suite.
 *
 * Input: 4-byte elements at wave, float32 (FLOAT) or int32 (INT), strides in elements:
 *   STREAM   frame t of channel c at wave[c * channel_stride + t],                                   t < total_frames
 *   PACKETS  frame t of clip i, channel c at wave[i * packet_stride + c * channel_stride + t], i < ceil(total_frames /
 *            frame_length); only the last clip may be short, and its columns behind its frames are not read
 * Output: total_frames interleaved little-endian frames at pcm, 2 / 3 / 3 / 4 bytes per sample at depth 16 / 20 / 24 / 32
 * (alacgpu_encode_device's input), and nothing outside those bytes.
 *
 * Value, with q = the depth:
 *   FLOAT  v = rint(x * 2^(q - 1)) in float32 (the product is exact, the rounding is to nearest even), saturated to
 *          [-2^(q - 1), 2^(q - 1) - 1], NaN -> 0; at depth 20 the three bytes hold v << 4 (left-aligned)
 *   INT    x saturated to the container's width 16 / 24 / 24 / 32; at depth 20 the low four bits cleared
 * A sample that was saturated or was NaN counts as clipped; cleared low bits do not.
 *
 * A SEGMENT is a run of frames whose channel rows are contiguous: the whole stream (STREAM) or one clip (PACKETS). A tile
 * is kTileBytes worth of consecutive frames of one segment, all channels. Phase 1 walks the tile's input QUADS: four
 * elements of a channel row that share a 16-byte-aligned address. Eight consecutive work items take eight consecutive
 * quads (32 frames, one 128-byte line) of one channel; the next eight the next channel. A quad whose four elements all lie
 * inside the segment's columns comes in as one 16-byte load (also where it reaches over the tile's edge into a neighbour's
 * frames: those elements are read and dropped), the quads at a row's two ends element by element. Every sample of the
 * tile is quantised and scattered into a staging image of the interleaved bytes (LDS on the device), which keeps the
 * destination's offset within its first 16-byte chunk. Phase 2 writes the image out in 16-byte chunks of the ABSOLUTE
 * address space: whole chunks with one 16-byte store, the chunks at the two ends, which the tile shares with its
 * neighbours or with bytes that are not the stream's, byte by byte. So every alignment of wave, the strides and pcm takes
 * the wide loads and the wide stores in the body.
 */
#ifndef ALAC_WAVEPACK_H
#define ALAC_WAVEPACK_H

#include <stddef.h>
#include <stdint.h>

#ifndef ALAC_WP_FN
#if defined(__HIPCC__)
#define ALAC_WP_FN __host__ __device__ inline
#else
#define ALAC_WP_FN inline
#endif
#endif

namespace alacwp {

constexpr uint32_t kStream = 0, kPackets = 1; /* alacgpu_wave_layout */
constexpr uint32_t kFloat = 0, kInt = 1;      /* alacgpu_wave_type */

constexpr uint32_t kThreads = 256;    /* work items of a tile */
constexpr uint32_t kTileBytes = 8192; /* PCM bytes of a tile: 256 frames of the largest frame (8 channels x 4 bytes) */
/* staging image: the tile and the offset within the first 16-byte chunk, rounded up to whole chunks */
constexpr uint32_t kStageBytes = kTileBytes + 16u + 16u;
/* the kernel goes in slices of this many workgroups, far below a dispatch's 2^32 work-items (2^22 x 256 = 2^30) */
constexpr uint64_t kTilesPerLaunch = (uint64_t)1 << 22;

/* 16 bytes moved by one instruction */
typedef uint32_t U4 __attribute__((vector_size(16)));
/* the staging image is bytes that are also written two and four at a time */
typedef uint16_t H1 __attribute__((may_alias));
typedef uint32_t W1 __attribute__((may_alias));

struct Params {
    const uint8_t* wave; /* 4-byte aligned */
    uint8_t* pcm;
    uint64_t channel_stride, packet_stride; /* elements */
    uint64_t total_frames;
    uint64_t seg_frames;    /* frames of a full segment: total_frames (STREAM) or frame_length (PACKETS) */
    uint64_t n_seg;         /* segments */
    uint64_t tiles_per_seg; /* ceil(seg_frames / tile_frames) */
    uint32_t nch, bps, bpf, depth;
    uint32_t layout, type;
    uint32_t tile_frames; /* a multiple of 64 */
    float scale;          /* 2^(q - 1): the multiplier, and the first float above the range */
    int32_t lo, hi;       /* the range a sample is saturated to */
    uint32_t shift;       /* FLOAT at depth 20: 4 */
    uint32_t keep;        /* INT at depth 20: ~15 */
};

ALAC_WP_FN uint32_t bytes_per_sample(uint32_t depth) { return depth == 16 ? 2u : (depth == 20 || depth == 24) ? 3u : depth == 32 ? 4u : 0u; }

/* frames of a tile: kTileBytes worth, a multiple of 64, at least 256 (its bytes are a multiple of 16 and at most kTileBytes) */
ALAC_WP_FN uint32_t tile_frames_of(uint32_t bpf) {
    const uint32_t t = (kTileBytes / bpf) & ~63u;
    return t < 256u ? 256u : t;
}

ALAC_WP_FN uint64_t packets_of(uint64_t total_frames, uint32_t frame_length) {
    return total_frames / frame_length + (total_frames % frame_length ? 1u : 0u);
}

ALAC_WP_FN Params make_params(uint32_t frame_length, uint32_t depth, uint32_t nch, uint32_t layout, uint32_t type, uint64_t total_frames) {
    Params p{};
    p.total_frames = total_frames;
    p.nch = nch;
    p.depth = depth;
    p.bps = bytes_per_sample(depth);
    p.bpf = p.bps * nch;
    p.layout = layout;
    p.type = type;
    p.tile_frames = tile_frames_of(p.bpf);
    p.seg_frames = layout == kPackets ? frame_length : total_frames;
    p.n_seg = layout == kPackets ? packets_of(total_frames, frame_length) : (total_frames ? 1u : 0u);
    p.tiles_per_seg = p.seg_frames / p.tile_frames + (p.seg_frames % p.tile_frames ? 1u : 0u);
    /* FLOAT: q bits; INT: the container's width */
    const uint32_t w = type == kFloat ? depth : 8u * p.bps;
    p.hi = (int32_t)(0x7fffffffu >> (32u - w));
    p.lo = -p.hi - 1;
    union {
        uint32_t u;
        float f;
    } s;
    s.u = (127u + depth - 1u) << 23; /* 2^(q - 1) from its bits */
    p.scale = s.f;
    p.shift = type == kFloat && depth == 20 ? 4u : 0u;
    p.keep = type == kInt && depth == 20 ? ~15u : ~0u;
    return p;
}

/* slices of the tile space: slice k of ceil(tiles / per) is [first, first + count) */
struct Slice {
    uint64_t first, count;
};
ALAC_WP_FN uint64_t slice_count(uint64_t tiles, uint64_t per) { return tiles / per + (tiles % per ? 1u : 0u); }
ALAC_WP_FN Slice slice_of(uint64_t tiles, uint64_t per, uint64_t k) {
    Slice s;
    s.first = k * per;
    s.count = tiles - s.first < per ? tiles - s.first : per;
    return s;
}

/* the element's 32 bits -> the sample's integer as the bytes hold it; clipped is raised by one for a saturated sample or a NaN */
ALAC_WP_FN uint32_t quantize(const Params& p, uint32_t bits, uint32_t& clipped) {
    int32_t v;
    if (p.type == kInt) {
        v = (int32_t)bits;
        if (v > p.hi) {
            v = p.hi;
            clipped++;
        } else if (v < p.lo) {
            v = p.lo;
            clipped++;
        }
        return (uint32_t)v & p.keep;
    }
    union {
        uint32_t u;
        float f;
    } x;
    x.u = bits;
    const float r = __builtin_rintf(x.f * p.scale); /* a power of two times x: exact; then one rounding to nearest even */
    /* the comparisons come before the conversion: r is an integer (or infinite), so r > hi is r >= 2^(q - 1) */
    if (!(r == r)) {
        v = 0;
        clipped++;
    } else if (r >= p.scale) {
        v = p.hi;
        clipped++;
    } else if (r < -p.scale) {
        v = p.lo;
        clipped++;
    } else {
        v = (int32_t)r;
    }
    return (uint32_t)v << p.shift;
}

/* the low bps bytes of u at stage + o, any alignment: the widest stores the offset's parity allows */
ALAC_WP_FN void put_sample(uint8_t* stage, uint32_t o, uint32_t u, uint32_t bps) {
    if (bps == 4u && !(o & 3u)) {
        *(W1*)(stage + o) = u;
    } else if (bps == 2u && !(o & 1u)) {
        *(H1*)(stage + o) = (uint16_t)u;
    } else if (bps == 3u && !(o & 1u)) {
        *(H1*)(stage + o) = (uint16_t)u;
        stage[o + 2u] = (uint8_t)(u >> 16);
    } else if (bps == 3u) {
        stage[o] = (uint8_t)u;
        *(H1*)(stage + o + 1u) = (uint16_t)(u >> 8);
    } else {
        for (uint32_t b = 0; b < bps; b++) stage[o + b] = (uint8_t)(u >> (8u * b));
    }
}

/* what a tile works on */
struct Tile {
    uint64_t t0;   /* first frame of the tile within its segment: a multiple of 4 */
    uint64_t cols; /* frames of the segment */
    uint64_t row0; /* byte offset of channel 0's column 0 of the segment from p.wave */
    uint64_t dst;  /* byte offset of the tile's first frame from p.pcm */
    uint32_t nf;   /* frames of the tile; 0: nothing to do */
    uint32_t sh;   /* offset of the first frame's first byte within its 16-byte chunk = its offset in the staging image */
    uint32_t rows; /* groups of 8 quads per channel */
};

ALAC_WP_FN Tile make_tile(const Params& p, uint64_t seg, uint64_t tile) {
    Tile t{};
    const uint64_t first = seg * p.seg_frames; /* the segment's first frame of the stream */
    const uint64_t left = p.total_frames - first;
    t.cols = left < p.seg_frames ? left : p.seg_frames;
    t.t0 = tile * p.tile_frames;
    if (t.t0 >= t.cols) return t;
    t.nf = t.cols - t.t0 < p.tile_frames ? (uint32_t)(t.cols - t.t0) : p.tile_frames;
    t.row0 = 4u * (p.layout == kPackets ? seg * p.packet_stride : 0u);
    t.dst = (first + t.t0) * p.bpf;
    t.sh = (uint32_t)((uintptr_t)(p.pcm + t.dst) & 15u);
    /* a row that is off its 16-byte boundary pushes up to three frames into one more quad */
    const uint64_t a0 = ((uint64_t)(uintptr_t)p.wave + t.row0) >> 2;
    const bool off = (a0 & 3u) || (p.nch > 1u && (p.channel_stride & 3u));
    t.rows = (t.nf + 31u) / 32u + (off ? 1u : 0u);
    return t;
}

/* Phase 1: work item `tid` of kThreads loads its quads, quantises them and scatters the samples into stage (16-byte
 * aligned, kStageBytes). -> its count of clipped samples. */
ALAC_WP_FN uint32_t load_tile(const Params& p, const Tile& t, uint8_t* stage, uint32_t tid) {
    uint32_t clipped = 0;
    const uint32_t items = t.rows * p.nch * 8u;
    /* group g = k / 8 is channel g % nch of quad row g / nch: divided once, then carried (g grows by kThreads / 8 a turn) */
    const uint32_t step_c = (kThreads / 8u) % p.nch, step_r = (kThreads / 8u) / p.nch;
    uint32_t c = (tid >> 3) % p.nch, r = (tid >> 3) / p.nch;
    for (uint32_t k = tid; k < items; k += kThreads, c += step_c, r += step_r) {
        if (c >= p.nch) {
            c -= p.nch;
            r++;
        }
        const uint32_t q = r * 8u + (k & 7u); /* quad of the tile */
        const uint64_t row = t.row0 + 4u * (uint64_t)c * p.channel_stride; /* the row's column 0, in bytes from p.wave */
        const uint32_t m = (uint32_t)(((uint64_t)(uintptr_t)p.wave + row) >> 2) & 3u; /* its distance from a 16-byte boundary, in elements */
        const int32_t k0 = (int32_t)(4u * q) - (int32_t)m; /* the quad's first frame, counted from the tile's first */
        if (k0 >= (int32_t)t.nf) continue;
        const int64_t col = (int64_t)t.t0 + k0; /* its first column of the row */
        /* 16-byte aligned; may begin in front of the row, then those elements are not read (an offset from p.wave, so
         * that the device build knows the pointer for a global one) */
        const uint32_t* src = (const uint32_t*)(p.wave + (int64_t)row + 4 * col);
        U4 e = {0u, 0u, 0u, 0u};
        if (col >= 0 && col + 3 < (int64_t)t.cols) {
            e = *(const U4*)src;
        } else {
            if (k0 >= 0 && k0 < (int32_t)t.nf) e[0] = src[0];
            if (k0 + 1 >= 0 && k0 + 1 < (int32_t)t.nf) e[1] = src[1];
            if (k0 + 2 >= 0 && k0 + 2 < (int32_t)t.nf) e[2] = src[2];
            if (k0 + 3 >= 0 && k0 + 3 < (int32_t)t.nf) e[3] = src[3];
        }
        const uint32_t o = t.sh + (uint32_t)k0 * p.bpf + c * p.bps; /* wraps for k0 < 0; used only where k0 + j >= 0 */
        if (k0 >= 0 && k0 < (int32_t)t.nf) put_sample(stage, o, quantize(p, e[0], clipped), p.bps);
        if (k0 + 1 >= 0 && k0 + 1 < (int32_t)t.nf) put_sample(stage, o + p.bpf, quantize(p, e[1], clipped), p.bps);
        if (k0 + 2 >= 0 && k0 + 2 < (int32_t)t.nf) put_sample(stage, o + 2u * p.bpf, quantize(p, e[2], clipped), p.bps);
        if (k0 + 3 >= 0 && k0 + 3 < (int32_t)t.nf) put_sample(stage, o + 3u * p.bpf, quantize(p, e[3], clipped), p.bps);
    }
    return clipped;
}

/* Phase 2: work item `tid` of kThreads writes its chunks of the staged image. */
ALAC_WP_FN void store_tile(const Params& p, const Tile& t, const uint8_t* stage, uint32_t tid) {
    const uint32_t end = t.sh + t.nf * p.bpf;
    uint8_t* base = p.pcm + t.dst - t.sh; /* 16-byte aligned */
    for (uint32_t j = tid; j * 16u < end; j += kThreads) {
        const uint32_t a = j * 16u;
        if (a >= t.sh && a + 16u <= end) {
            *(U4*)(base + a) = *(const U4*)(stage + a);
        } else {
            for (uint32_t b = 0; b < 16u; b++)
                if (a + b >= t.sh && a + b < end) base[a + b] = stage[a + b];
        }
    }
}

}  // namespace alacwp

#if defined(__HIPCC__)
/* k_wavepack.hip, called by the encoder's waveform entries (k_enc.hip) */
namespace alack {
/* The pass on `stream`: clears *p_clipped (when given) and launches alac_wave_pack in slices of tiles_per_launch workgroups. */
hipError_t wavepack_launch(hipStream_t stream, alacwp::Params p, uint64_t* d_clipped, uint64_t tiles_per_launch);
}  // namespace alack
#endif
#endif /* ALAC_WAVEPACK_H */
