/*
 * wave_sim.cpp — TEST-ONLY host build of the waveform pass.
 *
 * Compiles saprobe-alac_amd/csrc/alac_waveform.h (the text the gfx950 kernels of k_wave.hip are built from) with g++ and
 * runs it the way k_wave.hip launches it: the prefix sum of f[i], then for every tile of every packet the staging phase
 * for work items 0..255, the barrier, and the store phase for work items 0..255. The CPU suite (-m "not gpu") checks it
 * against a numpy restatement. It lives under tests/ and is never linked into libalacgpu.so.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../saprobe-alac_amd/csrc/alac_waveform.h"

using namespace alacwf;

extern "C" {

/* The arguments of alacgpu_waveform_device with host pointers, the configuration spelled out. -> 0, or -2 for what the
 * entry rejects. */
int wave_sim_run(uint32_t frame_length, uint32_t depth, uint32_t nch, const uint8_t* pcm, uint64_t pcm_stride,
                 const uint32_t* frames, const int32_t* status, uint64_t n, int layout, int type, void* wave,
                 uint64_t channel_stride, uint64_t packet_stride, uint64_t* starts_out) {
    if ((layout != (int)kStream && layout != (int)kPackets) || (type != (int)kFloat && type != (int)kInt)) return -2;
    if (!bytes_per_sample(depth) || nch < 1 || nch > 8 || !frame_length) return -2;
    Params p = make_params(frame_length, depth, nch, (uint32_t)layout, (uint32_t)type);
    if (n) {
        if (!pcm || !frames || !wave || ((uintptr_t)wave & 3u)) return -2;
        if (pcm_stride < (uint64_t)frame_length * p.bpf) return -2;
        if (layout == (int)kStream ? channel_stride < n * frame_length
                                   : (channel_stride < frame_length || packet_stride / nch < channel_stride))
            return -2;
    }
    p.pcm = pcm;
    p.pcm_stride = pcm_stride;
    p.frames = frames;
    p.status = status;
    p.wave = (uint8_t*)wave;
    p.channel_stride = channel_stride;
    p.packet_stride = packet_stride;
    p.n = n;
    std::vector<uint64_t> starts(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) starts[i + 1] = starts[i] + frames_of(p, i);
    if (starts_out) memcpy(starts_out, starts.data(), (n + 1) * sizeof(uint64_t));
    p.starts = starts.data();
    alignas(16) static thread_local uint8_t stage[kStageBytes];
    for (uint64_t pk = 0; pk < n; pk++)
        for (uint32_t tile = 0; tile < p.tiles_per_packet; tile++) {
            const Tile t = make_tile(p, pk, tile);
            if (!t.any) continue;
            memset(stage, 0xA5, sizeof(stage)); /* LDS holds whatever the last workgroup left */
            for (uint32_t tid = 0; tid < kThreads; tid++) stage_tile(p, t, stage, tid);
            for (uint32_t tid = 0; tid < kThreads; tid++) store_tile(p, t, stage, tid);
        }
    return 0;
}

uint32_t wave_sim_tile_frames(uint32_t depth, uint32_t nch) { return tile_frames_of(bytes_per_sample(depth) * nch); }

}  // extern "C"
