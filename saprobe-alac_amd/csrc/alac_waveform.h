/*
 * alac_waveform.h — decoded PCM slots -> planar float32 / int32 waveforms: the per-sample unpack and convert, the index
 * arithmetic and the two phases of a tile, as plain host + device code. k_wave.hip builds the gfx950 kernels from this
 * text; tests/host_sim/wave_sim.cpp builds the same text with g++ for the CPU suite.
 *
 * Input: the decoder's output (include/alacgpu.h: alacgpu_decode_batch_device): packet i's interleaved little-endian PCM
 * at pcm + i * pcm_stride, frames[i] frames of nch samples of 2 / 3 / 3 / 4 bytes (16 / 20 / 24 / 32 bits; a 20-bit sample
 * is left-aligned in its 3 bytes and is read as the 24-bit value they hold), status[i] != 0 for a failed packet.
 *
 *   f[i]     = (status && status[i] != 0) ? 0 : min(frames[i], frame_length)
 *   start[i] = f[0] + ... + f[i - 1]
 *   STREAM   wave[c * channel_stride + start[i] + t]                   = sample(i, t, c)   for t < f[i]
 *   PACKETS  wave[i * packet_stride + c * channel_stride + t]          = sample(i, t, c)   for t < f[i]
 *                                                                       = 0                 for f[i] <= t < frame_length
 *   FLOAT    float32(int32 sample) * 2^-(w - 1), w = 16 / 24 / 24 / 32  (one rounding, to nearest even, at 32 bits only)
 *   INT      the int32 sample
 *
 * A tile is kTileBytes worth of consecutive frames of one packet, all channels. Phase 1 copies the tile's bytes into a
 * staging buffer (LDS on the device) in 16-byte chunks of the ABSOLUTE address space: whole chunks with one 16-byte load,
 * the chunks at the two ends, which the tile shares with its neighbours, byte by byte — so every pcm / pcm_stride alignment
 * takes the wide loads in the body, and the staged image keeps the source's offset within its first chunk. Phase 2 walks
 * the tile's output QUADS: four elements of a channel row that share a 16-byte-aligned address. Eight consecutive work
 * items take eight consecutive quads (32 frames, one 128-byte line) of one channel; the next eight the next channel. A quad
 * whose four elements all lie inside the row's columns goes out as one 16-byte store, the quads at a row's two ends element
 * by element — so every wave base, channel_stride and start[i] takes the wide stores in the body as well. Because quads
 * are aligned in the destination and not in the packet, a tile stages up to three frames in front of its own (kHalo), and
 * the last tile of a packet takes one more group of quads for the frames its row's misalignment pushes over its end.
 */
#ifndef ALAC_WAVEFORM_H
#define ALAC_WAVEFORM_H

#include <stddef.h>
#include <stdint.h>

#ifndef ALAC_WF_FN
#if defined(__HIPCC__)
#define ALAC_WF_FN __host__ __device__ inline
#else
#define ALAC_WF_FN inline
#endif
#endif

namespace alacwf {

constexpr uint32_t kStream = 0, kPackets = 1; /* alacgpu_wave_layout */
constexpr uint32_t kFloat = 0, kInt = 1;      /* alacgpu_wave_type */

constexpr uint32_t kThreads = 256;     /* work items of a tile */
constexpr uint32_t kTileBytes = 8192;  /* PCM bytes of a tile: 256 frames of the largest frame (8 channels x 4 bytes) */
constexpr uint32_t kHalo = 3;          /* frames staged in front of the tile's own */
/* staging buffer: the tile, the halo, the offset within the first 16-byte chunk, and the second dword of the last sample's read */
constexpr uint32_t kStageBytes = kTileBytes + kHalo * 32u + 16u + 16u;

/* 16 bytes moved by one instruction (a struct of four words is taken apart by the compiler, and its stores regrouped) */
typedef uint32_t U4 __attribute__((vector_size(16)));

struct Params {
    const uint8_t* pcm;
    uint64_t pcm_stride;
    const uint32_t* frames;
    const int32_t* status;  /* may be null */
    const uint64_t* starts; /* STREAM: n + 1 exclusive prefix sums of f; unused for PACKETS */
    uint8_t* wave;          /* 4-byte aligned */
    uint64_t channel_stride, packet_stride; /* elements */
    uint64_t n;
    uint32_t frame_length, nch, bps, bpf;
    uint32_t layout, type;
    uint32_t tile_frames;      /* a multiple of 32 */
    uint32_t tiles_per_packet; /* ceil(frame_length / tile_frames) */
    float scale;               /* 2^-(w - 1) */
};

ALAC_WF_FN uint32_t bytes_per_sample(uint32_t depth) { return depth == 16 ? 2u : (depth == 20 || depth == 24) ? 3u : depth == 32 ? 4u : 0u; }

/* the width w of the integer a sample's bytes hold */
ALAC_WF_FN uint32_t sample_width(uint32_t depth) { return 8u * bytes_per_sample(depth); }

/* frames of a tile: kTileBytes worth, a multiple of 64, at least 256 */
ALAC_WF_FN uint32_t tile_frames_of(uint32_t bpf) {
    const uint32_t t = (kTileBytes / bpf) & ~63u;
    return t < 256u ? 256u : t;
}

ALAC_WF_FN Params make_params(uint32_t frame_length, uint32_t depth, uint32_t nch, uint32_t layout, uint32_t type) {
    Params p{};
    p.frame_length = frame_length;
    p.nch = nch;
    p.bps = bytes_per_sample(depth);
    p.bpf = p.bps * nch;
    p.layout = layout;
    p.type = type;
    p.tile_frames = tile_frames_of(p.bpf);
    p.tiles_per_packet = (frame_length + p.tile_frames - 1u) / p.tile_frames;
    /* 2^-(w - 1) from its bits: exponent 127 - (w - 1) */
    union {
        uint32_t u;
        float f;
    } s;
    s.u = (127u - (sample_width(depth) - 1u)) << 23;
    p.scale = s.f;
    return p;
}

/* f[i] */
ALAC_WF_FN uint32_t frames_of(const Params& p, uint64_t i) {
    if (p.status && p.status[i] != 0) return 0u;
    const uint32_t f = p.frames[i];
    return f < p.frame_length ? f : p.frame_length;
}

/* the sample whose first byte is byte `shift` (0..3) of the dword lo; hi is the dword behind it */
ALAC_WF_FN int32_t unpack_sample(uint32_t lo, uint32_t hi, uint32_t shift, uint32_t bps) {
    const uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * shift));
    if (bps == 2u) return (int32_t)(int16_t)(uint16_t)v;
    if (bps == 3u) return (int32_t)(v << 8) >> 8;
    return (int32_t)v;
}

/* the output element's 32 bits */
ALAC_WF_FN uint32_t convert(int32_t v, uint32_t type, float scale) {
    if (type == kInt) return (uint32_t)v;
    union {
        float f;
        uint32_t u;
    } o;
    o.f = (float)v * scale; /* int32 -> float32 rounds to nearest even; the scale is a power of two */
    return o.u;
}

/* what a tile works on */
struct Tile {
    uint32_t f;        /* frames of the packet with samples */
    uint32_t cols;     /* columns of a row this packet writes: f (STREAM) or frame_length (PACKETS) */
    uint32_t t0;       /* first frame of the tile */
    uint32_t lo, hi;   /* frames staged: [lo, hi) */
    uint32_t sh;       /* offset of frame lo's first byte within its 16-byte chunk = its offset in the staging buffer */
    uint32_t groups;   /* groups of 8 quads per channel row */
    uint64_t row0;     /* byte offset of channel 0's column 0 from p.wave */
    const uint8_t* src; /* frame lo's first byte */
    bool any;
};

ALAC_WF_FN Tile make_tile(const Params& p, uint64_t pk, uint32_t tile) {
    Tile t{};
    t.f = frames_of(p, pk);
    t.cols = p.layout == kPackets ? p.frame_length : t.f;
    t.t0 = tile * p.tile_frames;
    /* the first column a quad of this tile can hold is t0 - 3 */
    t.any = t.t0 < t.cols + kHalo;
    if (!t.any) return t;
    t.lo = t.t0 >= kHalo ? t.t0 - kHalo : 0u;
    const uint64_t end = (uint64_t)t.t0 + p.tile_frames;
    t.hi = end < t.f ? (uint32_t)end : t.f;
    if (t.hi < t.lo) t.hi = t.lo;
    t.src = p.pcm + pk * p.pcm_stride + (uint64_t)t.lo * p.bpf;
    t.sh = (uint32_t)((uintptr_t)t.src & 15u);
    t.groups = p.tile_frames / 32u + (tile + 1u == p.tiles_per_packet ? 1u : 0u);
    const uint64_t first = p.layout == kPackets ? pk * p.packet_stride : p.starts[pk];
    t.row0 = 4u * first;
    return t;
}

/* Phase 1: work item `tid` of kThreads copies its chunks of the tile's bytes into stage (16-byte aligned, kStageBytes). */
ALAC_WF_FN void stage_tile(const Params& p, const Tile& t, uint8_t* stage, uint32_t tid) {
    const uint32_t nbytes = (t.hi - t.lo) * p.bpf;
    if (!nbytes) return;
    const uint32_t end = t.sh + nbytes;
    const uint8_t* base = t.src - t.sh; /* 16-byte aligned */
    for (uint32_t j = tid; j * 16u < end; j += kThreads) {
        const uint32_t a = j * 16u;
        if (a >= t.sh && a + 16u <= end) {
            *(U4*)(stage + a) = *(const U4*)(base + a);
        } else {
            for (uint32_t b = 0; b < 16u; b++)
                if (a + b >= t.sh && a + b < end) stage[a + b] = base[a + b];
        }
    }
}

/* the element of (frame fr, channel c): a sample of the staged tile, or the zero behind a short packet */
ALAC_WF_FN uint32_t element(const Params& p, const Tile& t, const uint8_t* stage, int64_t fr, uint32_t c) {
    if (fr >= (int64_t)t.f) return 0u; /* PACKETS: the columns behind the packet's frames (0.0f and 0 are the same bits) */
    const uint32_t o = t.sh + ((uint32_t)fr - t.lo) * p.bpf + c * p.bps;
    const uint32_t* w = (const uint32_t*)(stage + (o & ~3u));
    return convert(unpack_sample(w[0], w[1], o & 3u, p.bps), p.type, p.scale);
}

/* Phase 2: work item `tid` of kThreads converts and stores its quads. */
ALAC_WF_FN void store_tile(const Params& p, const Tile& t, const uint8_t* stage, uint32_t tid) {
    const uint32_t items = t.groups * p.nch * 8u;
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
        const int64_t fr0 = (int64_t)t.t0 + 4 * (int64_t)q - (int64_t)m;   /* the quad's first column */
        if (fr0 + 3 < 0 || fr0 >= (int64_t)t.cols) continue;
        /* 16-byte aligned; may lie in front of the row, then it is not stored to (an offset from p.wave, so that the device
         * build knows the pointer for a global one) */
        uint32_t* dst = (uint32_t*)(p.wave + (int64_t)row + 4 * fr0);
        if (fr0 >= 0 && fr0 + 3 < (int64_t)t.cols) {
            const U4 v = {element(p, t, stage, fr0, c), element(p, t, stage, fr0 + 1, c), element(p, t, stage, fr0 + 2, c),
                          element(p, t, stage, fr0 + 3, c)};
            *(U4*)dst = v;
        } else {
            for (int j = 0; j < 4; j++)
                if (fr0 + j >= 0 && fr0 + j < (int64_t)t.cols) dst[j] = element(p, t, stage, fr0 + j, c);
        }
    }
}

}  // namespace alacwf

#if defined(__HIPCC__)
/* k_wave.hip, called by alacgpu_waveform_device (alacgpu.hip) */
namespace alack {
/* bytes of the scan's scratch for n packets: the workgroup sums, then n + 1 prefix sums (used when the caller passes no d_starts) */
size_t wave_scratch_bytes(size_t n);
/* All kernels of one pass on `stream`. p.starts is ignored: the prefix sums go to d_starts when it is given and to the
 * scratch otherwise, and the convert kernel reads them from there; PACKETS without d_starts runs no scan. */
hipError_t wave_launch(hipStream_t stream, alacwf::Params p, uint64_t* d_starts, void* scratch);
}  // namespace alack
#endif
#endif /* ALAC_WAVEFORM_H */
