/*
 * alac_clips.h — decoded PCM slots -> a batch of fixed-length crops [clips][channels][clip_frames], float32 / int32: the
 * index arithmetic and the two phases of a tile, as plain host + device code over alac_waveform.h's unpack and convert.
 * k_clips.hip builds the gfx950 kernels from this text; tests/host_sim/clip_sim.cpp builds the same text with g++ for the
 * CPU suite.
 *
 * Input: the decoder's output as alacgpu_waveform_device takes it (pcm / pcm_stride / frames / status, n slots). Slot i
 * occupies the frames [i * FL, (i + 1) * FL) of a grid over the batch, FL = frame_length. Clip j has two descriptors:
 * begin[j], its first grid frame, and limit[j], the first slot that is not its source's any more.
 *
 *   f[i]   = (status && status[i] != 0) ? 0 : min(frames[i], FL)
 *   g      = begin[j] + t,  i = g / FL,  r = g % FL                                     for t < L = clip_frames
 *   has    = g does not overflow && i < min(limit[j], n) && r < f[i]
 *   clips[j * clip_stride + c * channel_stride + t] = has ? sample(i, r, c) : 0         FLOAT / INT as in alac_waveform.h
 *   valid[j]       = number of t < L with has
 *   clip_status[j] = status[i] of the lowest slot i the clip touches (i < min(limit[j], n)) with status[i] != 0, else 0
 *
 * With lim = min(limit[j], n), the columns t >= end = clamp(lim * FL - begin[j], 0, L) are zero whatever the slots hold,
 * and no column below end overflows or leaves the slots [0, lim): everything past that point works on t < end only.
 *
 * A tile is tile_cols consecutive columns of one clip, all channels. Its source is a run of SEGMENTS, one per slot it
 * touches: the frames [ra, rb) of slot i0 + s, cut to the slot's f. Segments are not contiguous in memory (pcm_stride, short
 * slots), so segment s is staged at s * pitch of the staging buffer (LDS on the device), in 16-byte chunks of the ABSOLUTE
 * address space as alacwf::stage_tile does per packet: whole chunks with one 16-byte load, the chunks at a segment's two
 * ends byte by byte, the staged image keeping the source's offset within its first chunk. Nothing outside a slot's first
 * f frames is read. Beside the bytes the staging phase writes one entry per segment: f, and where frame 0 of the slot
 * would lie in the staging buffer. tile_cols is chosen so that the segments of a tile fit kStageBytes at their pitch:
 * 8 KB of PCM when FL is large, fewer columns when FL is so small that the 16-byte alignment slack dominates.
 * Phase 2 walks the tile's output quads exactly as alacwf::store_tile does (eight work items take eight consecutive quads
 * of one channel, 16-byte stores in the body, element by element at a row's two ends, three columns of halo in front and
 * one more group of quads in the last tile). A work item divides once, for its first quad, and then carries (segment,
 * frame in the slot) from quad to quad with steps that make_params divided on the host; the four elements of a quad are
 * reached by stepping back from its last column.
 */
#ifndef ALAC_CLIPS_H
#define ALAC_CLIPS_H

#include "alac_waveform.h"

namespace alacclip {

using alacwf::kThreads;
using alacwf::U4;

constexpr uint32_t kHalo = alacwf::kHalo;
constexpr uint32_t kStageBytes = 20480; /* two segments of a full tile (8 KB + halo + alignment slack each), with room */
constexpr uint32_t kSlack = 32;         /* per segment: the offset within the first chunk, the second dword of the last sample's read */
constexpr uint32_t kMaxSegs = kStageBytes / (16u + kSlack); /* the smallest pitch is one chunk plus the slack */

/* what the staging phase leaves per segment */
struct Seg {
    uint32_t f;   /* f of the segment's slot */
    uint32_t off; /* offset in the staging buffer of the slot's frame 0 (modulo 2^32: frames in front of ra are not there) */
};

struct Params {
    const uint8_t* pcm;
    uint64_t pcm_stride;
    const uint32_t* frames;
    const int32_t* status; /* may be null */
    uint64_t n;            /* slots */
    const uint64_t* begin;
    const uint64_t* limit;
    uint64_t n_clips;
    uint8_t* clips;        /* 4-byte aligned */
    uint64_t channel_stride, clip_stride; /* elements */
    uint32_t* valid;       /* may be null */
    int32_t* clip_status;  /* may be null */
    uint32_t clip_frames, frame_length, nch, bps, bpf, type;
    uint32_t tile_cols;      /* a multiple of 32 */
    uint32_t tiles_per_clip; /* ceil(clip_frames / tile_cols) */
    uint32_t pitch, chunks;  /* bytes and 16-byte chunks of a segment's place in the staging buffer */
    uint32_t stage_dq, stage_dr; /* kThreads / chunks, kThreads % chunks: a work item's step through (segment, chunk) */
    uint32_t turn_dq, turn_dr;   /* (32 * step_r) / FL, % FL: its step through (segment, frame) from turn to turn of phase 2 */
    uint32_t group_dq, group_dr; /* 32 / FL, 32 % FL: one more group of quads, when the channel wraps */
    float scale;
};

/* frames of one slot a tile of tc columns can touch, and the slots */
ALAC_WF_FN uint32_t seg_frames(uint32_t fl, uint32_t tc) { return fl < tc + kHalo ? fl : tc + kHalo; }
ALAC_WF_FN uint32_t seg_pitch(uint32_t fl, uint32_t bpf, uint32_t tc) { return ((seg_frames(fl, tc) * bpf + 15u) & ~15u) + kSlack; }
ALAC_WF_FN uint32_t max_segs(uint32_t fl, uint32_t tc) { return (tc + kHalo - 1u) / fl + 2u; }

ALAC_WF_FN Params make_params(uint32_t frame_length, uint32_t depth, uint32_t nch, uint32_t type, uint32_t clip_frames) {
    Params p{};
    p.frame_length = frame_length;
    p.clip_frames = clip_frames;
    p.nch = nch;
    p.bps = alacwf::bytes_per_sample(depth);
    p.bpf = p.bps * nch;
    p.type = type;
    uint32_t tc = alacwf::tile_frames_of(p.bpf);
    while (tc > 32u && (uint64_t)max_segs(frame_length, tc) * seg_pitch(frame_length, p.bpf, tc) > kStageBytes) tc = (tc / 2u) & ~31u;
    p.tile_cols = tc;
    p.tiles_per_clip = (uint32_t)(((uint64_t)clip_frames + tc - 1u) / tc);
    p.pitch = seg_pitch(frame_length, p.bpf, tc);
    p.chunks = p.pitch / 16u;
    p.stage_dq = kThreads / p.chunks;
    p.stage_dr = kThreads % p.chunks;
    const uint32_t turn = 32u * ((kThreads / 8u) / nch);
    p.turn_dq = turn / frame_length;
    p.turn_dr = turn % frame_length;
    p.group_dq = 32u / frame_length;
    p.group_dr = 32u % frame_length;
    p.scale = alacwf::make_params(frame_length, depth, nch, alacwf::kPackets, type).scale;
    return p;
}

/* f[i] */
ALAC_WF_FN uint32_t frames_of(const Params& p, uint64_t i) {
    if (p.status && p.status[i] != 0) return 0u;
    const uint32_t f = p.frames[i];
    return f < p.frame_length ? f : p.frame_length;
}

/* end: the columns [end, L) of clip j are zero; no column below it overflows or leaves the clip's slots */
ALAC_WF_FN uint32_t clip_end(const Params& p, uint64_t j) {
    const uint64_t b = p.begin[j];
    const uint64_t lim = p.limit[j] < p.n ? p.limit[j] : p.n;
    const uint64_t span = lim * p.frame_length; /* n < 2^31 and FL < 2^32 */
    if (b >= span) return 0u;
    return span - b < p.clip_frames ? (uint32_t)(span - b) : p.clip_frames;
}

/* (segment, frame in its slot) of a column; frame is below FL */
struct Pos {
    uint32_t s;
    uint64_t r;
};
ALAC_WF_FN void forward(Pos& q, uint32_t dq, uint32_t dr, uint32_t fl) {
    q.s += dq;
    q.r += dr;
    if (q.r >= fl) {
        q.r -= fl;
        q.s++;
    }
}
ALAC_WF_FN void back_one(Pos& q, uint32_t fl) {
    if (q.r == 0) {
        q.s--;
        q.r = fl - 1u;
    } else {
        q.r--;
    }
}

/* what a tile works on */
struct Tile {
    uint64_t i0;     /* slot of column lo */
    uint32_t r0;     /* its frame in that slot */
    uint32_t end;    /* clip_end */
    uint32_t t0;     /* first column of the tile */
    uint32_t lo, hi; /* columns staged: [lo, hi), hi <= end */
    uint32_t nseg;   /* segments staged */
    uint32_t groups; /* groups of 8 quads per channel row */
    uint64_t row0;   /* byte offset of channel 0's column 0 from p.clips */
};

ALAC_WF_FN Tile make_tile(const Params& p, uint64_t j, uint32_t tile) {
    Tile t{};
    t.end = clip_end(p, j);
    t.t0 = tile * p.tile_cols;
    t.lo = t.t0 >= kHalo ? t.t0 - kHalo : 0u;
    const uint64_t stop = (uint64_t)t.t0 + p.tile_cols;
    t.hi = stop < t.end ? (uint32_t)stop : t.end;
    if (t.hi < t.lo) t.hi = t.lo;
    if (t.hi > t.lo) {
        const uint64_t g = p.begin[j] + t.lo; /* the one division of the grid frame: everything else is carried from it */
        t.i0 = g / p.frame_length;
        t.r0 = (uint32_t)(g - t.i0 * p.frame_length);
        const uint64_t last = (uint64_t)t.r0 + (t.hi - t.lo - 1u); /* below FL + tile_cols + kHalo */
        t.nseg = last < p.frame_length ? 1u : 2u + (uint32_t)(last - p.frame_length) / p.frame_length;
    }
    t.groups = p.tile_cols / 32u + (tile + 1u == p.tiles_per_clip ? 1u : 0u);
    t.row0 = 4u * j * p.clip_stride;
    return t;
}

/* segment s of a tile: the frames [ra, rb) of slot i0 + s, rb cut to the slot's f (rb <= ra: nothing) */
struct Segment {
    uint32_t f, ra, rb;
    const uint8_t* src; /* frame ra's first byte */
};
ALAC_WF_FN Segment segment(const Params& p, const Tile& t, uint32_t s) {
    Segment g;
    const uint64_t i = t.i0 + s;
    g.f = frames_of(p, i);
    g.ra = s ? 0u : t.r0;
    /* the columns in front of this segment, and so the frames left for it */
    const uint64_t before = s ? (uint64_t)s * p.frame_length - t.r0 : 0u;
    const uint64_t left = (uint64_t)(t.hi - t.lo) - before;
    const uint64_t rb = g.ra + left;
    g.rb = rb < g.f ? (uint32_t)rb : g.f;
    g.src = p.pcm + i * p.pcm_stride + (uint64_t)g.ra * p.bpf;
    return g;
}

/* Phase 1: work item `tid` of kThreads copies its chunks of the tile's segments into stage (16-byte aligned, kStageBytes)
 * and writes its entries of segs (kMaxSegs). */
ALAC_WF_FN void stage_tile(const Params& p, const Tile& t, uint8_t* stage, Seg* segs, uint32_t tid) {
    for (uint32_t s = tid; s < t.nseg; s += kThreads) {
        const Segment g = segment(p, t, s);
        const uint32_t sh = (uint32_t)((uintptr_t)g.src & 15u);
        segs[s].f = g.f;
        segs[s].off = s * p.pitch + sh - g.ra * p.bpf;
    }
    /* item k = (segment k / chunks, chunk k % chunks): divided once, then carried (k grows by kThreads a turn) */
    uint32_t s = tid / p.chunks, c = tid % p.chunks;
    uint32_t have = ~0u, sh = 0, end = 0;
    const uint8_t* base = nullptr;
    for (; s < t.nseg; s += p.stage_dq, c += p.stage_dr) {
        if (c >= p.chunks) {
            c -= p.chunks;
            if (++s >= t.nseg) break;
        }
        if (s != have) {
            const Segment g = segment(p, t, s);
            sh = (uint32_t)((uintptr_t)g.src & 15u);
            end = g.rb > g.ra ? sh + (g.rb - g.ra) * p.bpf : 0u;
            base = g.src - sh; /* 16-byte aligned */
            have = s;
        }
        const uint32_t a = c * 16u;
        if (a >= end) continue;
        uint8_t* dst = stage + s * p.pitch;
        if (a >= sh && a + 16u <= end) {
            *(U4*)(dst + a) = *(const U4*)(base + a);
        } else {
            for (uint32_t b = 0; b < 16u; b++)
                if (a + b >= sh && a + b < end) dst[a + b] = base[a + b];
        }
    }
}

/* the element of (column x at position q, channel c): a sample of a staged segment, or zero */
ALAC_WF_FN uint32_t element(const Params& p, const Tile& t, const uint8_t* stage, const Seg* segs, int64_t x, const Pos& q, uint32_t c) {
    if (x < 0 || x >= (int64_t)t.end) return 0u; /* (0.0f and 0 are the same bits) */
    const Seg g = segs[q.s];
    if (q.r >= g.f) return 0u; /* behind a short slot's frames, or a failed slot */
    const uint32_t o = g.off + (uint32_t)q.r * p.bpf + c * p.bps;
    const uint32_t* w = (const uint32_t*)(stage + (o & ~3u));
    return alacwf::convert(alacwf::unpack_sample(w[0], w[1], o & 3u, p.bps), p.type, p.scale);
}

/* Phase 2: work item `tid` of kThreads converts and stores its quads. */
ALAC_WF_FN void store_tile(const Params& p, const Tile& t, const uint8_t* stage, const Seg* segs, uint32_t tid) {
    const uint32_t items = t.groups * p.nch * 8u;
    const uint32_t fl = p.frame_length, L = p.clip_frames;
    /* group g = k / 8 is channel g % nch of quad row g / nch, as in alacwf::store_tile */
    const uint32_t step_c = (kThreads / 8u) % p.nch, step_r = (kThreads / 8u) / p.nch;
    uint32_t c = (tid >> 3) % p.nch, r = (tid >> 3) / p.nch;
    /* at: the position of column t0 + 4 * quad + 3, the last column of this work item's quad in a row that starts on a
     * 16-byte boundary; a row that starts m elements behind one has its quads m columns earlier. It is never in front of
     * column lo. */
    Pos at;
    {
        const uint32_t d = (t.t0 - t.lo) + 4u * (r * 8u + (tid & 7u)) + 3u;
        at.s = d / fl;
        at.r = (uint64_t)t.r0 + d % fl;
        if (at.r >= fl) {
            at.r -= fl;
            at.s++;
        }
    }
    for (uint32_t k = tid; k < items; k += kThreads, c += step_c, r += step_r, forward(at, p.turn_dq, p.turn_dr, fl)) {
        if (c >= p.nch) {
            c -= p.nch;
            r++;
            forward(at, p.group_dq, p.group_dr, fl);
        }
        const uint32_t q = r * 8u + (k & 7u); /* quad of the tile */
        const uint64_t row = t.row0 + 4u * (uint64_t)c * p.channel_stride; /* the row's column 0, in bytes from p.clips */
        const uint32_t m = (uint32_t)(((uint64_t)(uintptr_t)p.clips + row) >> 2) & 3u; /* its distance from a 16-byte boundary, in elements */
        const int64_t fr0 = (int64_t)t.t0 + 4 * (int64_t)q - (int64_t)m; /* the quad's first column */
        if (fr0 + 3 < 0 || fr0 >= (int64_t)L) continue;
        Pos w = at;
        for (uint32_t b = 0; b < m; b++) back_one(w, fl);
        uint32_t v[4];
        for (int e = 3; e >= 0; e--) {
            v[e] = element(p, t, stage, segs, fr0 + e, w, c);
            back_one(w, fl);
        }
        /* 16-byte aligned; may lie in front of the row, then it is not stored to */
        uint32_t* dst = (uint32_t*)(p.clips + (int64_t)row + 4 * fr0);
        if (fr0 >= 0 && fr0 + 3 < (int64_t)L) {
            const U4 u = {v[0], v[1], v[2], v[3]};
            *(U4*)dst = u;
        } else {
            for (int e = 0; e < 4; e++)
                if (fr0 + e >= 0 && fr0 + e < (int64_t)L) dst[e] = v[e];
        }
    }
}

/* valid[j] and clip_status[j]: one walk over the slots the clip touches, at most min(L / FL + 2, n) steps on one lane (serial:
 * long where FL is tiny and L huge; the entry launches it only when the caller asks for either output) */
ALAC_WF_FN void clip_meta(const Params& p, uint64_t j) {
    uint32_t left = clip_end(p, j), valid = 0;
    int32_t st = 0;
    if (left) {
        uint64_t i = p.begin[j] / p.frame_length;
        uint32_t r = (uint32_t)(p.begin[j] - i * p.frame_length);
        for (; left; i++, r = 0) {
            const uint32_t take = p.frame_length - r < left ? p.frame_length - r : left;
            const uint32_t f = frames_of(p, i);
            if (f > r) valid += (f - r < take ? f - r : take);
            if (!st && p.status) st = p.status[i];
            left -= take;
        }
    }
    if (p.valid) p.valid[j] = valid;
    if (p.clip_status) p.clip_status[j] = st;
}

}  // namespace alacclip

#if defined(__HIPCC__)
/* k_clips.hip, called by alacgpu_clips_device (alacgpu.hip) */
namespace alack {
/* All kernels of one gather on `stream`. */
hipError_t clips_launch(hipStream_t stream, const alacclip::Params& p);
}  // namespace alack
#endif
#endif /* ALAC_CLIPS_H */
