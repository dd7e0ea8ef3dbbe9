/*
 * pack_sim.cpp — TEST-ONLY host build of the pack pass (waveforms -> the encoder's PCM).
 *
 * Compiles saprobe-alac_amd/csrc/alac_wavepack.h (the text the gfx950 kernel of k_wavepack.hip is built from) with g++
 * and runs it the way k_wavepack.hip launches it: slice by slice, and for every tile of a slice the load phase for work
 * items 0..255, the barrier, and the store phase for work items 0..255; the work items' clipped counts are summed as the
 * workgroup's atomics sum them. The CPU suite (-m "not gpu") checks it against a numpy restatement. It lives under tests/
 * and is never linked into libalacgpu.so.
 */
#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/csrc/alac_wavepack.h"

using namespace alacwp;

extern "C" {

/* The arguments of alacgpu_pcm_from_waveform_device with host pointers, the configuration spelled out, and the slice
 * size (0: the library's). -> 0, or -2 for what the entry rejects. *launches_out: the slices that ran. */
int pack_sim_run(uint32_t frame_length, uint32_t depth, uint32_t nch, const void* wave, int layout, int type,
                 uint64_t channel_stride, uint64_t packet_stride, uint64_t total_frames, uint8_t* pcm, uint64_t* clipped_out,
                 uint64_t tiles_per_launch, uint64_t* launches_out) {
    if (!wave || !pcm) return -2;
    if ((layout != (int)kStream && layout != (int)kPackets) || (type != (int)kFloat && type != (int)kInt)) return -2;
    if (!bytes_per_sample(depth) || nch < 1 || nch > 8 || !frame_length) return -2;
    if ((uintptr_t)wave & 3u) return -2;
    if (layout == (int)kStream ? channel_stride < total_frames : (channel_stride < frame_length || packet_stride / nch < channel_stride))
        return -2;
    if (packets_of(total_frames, frame_length) > (((uint64_t)1 << 31) - 1)) return -2;
    Params p = make_params(frame_length, depth, nch, (uint32_t)layout, (uint32_t)type, total_frames);
    p.wave = (const uint8_t*)wave;
    p.pcm = pcm;
    p.channel_stride = channel_stride;
    p.packet_stride = packet_stride;
    const uint64_t per = tiles_per_launch ? tiles_per_launch : kTilesPerLaunch;
    const uint64_t tiles = p.n_seg * p.tiles_per_seg;
    const uint64_t slices = slice_count(tiles, per);
    uint64_t clipped = 0;
    alignas(16) static thread_local uint8_t stage[kStageBytes];
    for (uint64_t k = 0; k < slices; k++) {
        const Slice s = slice_of(tiles, per, k);
        for (uint64_t blk = 0; blk < s.count; blk++) {
            const uint64_t b = s.first + blk;
            const uint64_t seg = b / p.tiles_per_seg;
            if (seg >= p.n_seg) continue;
            const Tile t = make_tile(p, seg, b % p.tiles_per_seg);
            if (!t.nf) continue;
            memset(stage, 0xA5, sizeof(stage)); /* LDS holds whatever the last workgroup left */
            for (uint32_t tid = 0; tid < kThreads; tid++) clipped += load_tile(p, t, stage, tid);
            for (uint32_t tid = 0; tid < kThreads; tid++) store_tile(p, t, stage, tid);
        }
    }
    if (clipped_out) *clipped_out = clipped;
    if (launches_out) *launches_out = slices;
    return 0;
}

uint32_t pack_sim_tile_frames(uint32_t depth, uint32_t nch) { return tile_frames_of(bytes_per_sample(depth) * nch); }

}  // extern "C"
