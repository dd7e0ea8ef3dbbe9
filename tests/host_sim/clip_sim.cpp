/*
 * clip_sim.cpp — TEST-ONLY host build of the clip gather.
 *
 * Compiles saprobe-alac_amd/csrc/alac_clips.h (the text the gfx950 kernels of k_clips.hip are built from) with g++ and
 * runs it the way k_clips.hip launches it: for every tile of every clip the staging phase for work items 0..255, the
 * barrier, and the store phase for work items 0..255; then one clip_meta per clip. The CPU suite (-m "not gpu") checks it
 * against a numpy restatement. It lives under tests/ and is never linked into libalacgpu.so.
 */
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/csrc/alac_clips.h"

using namespace alacclip;

extern "C" {

/* The arguments of alacgpu_clips_device with host pointers, the configuration spelled out. -> 0, or -2 for what the entry
 * rejects. guard_bytes != 0: the first guard_bytes bytes at pcm are copied so that they END at an inaccessible page, and the
 * pass reads the copy: a read behind them is fatal. */
int clip_sim_run(uint32_t frame_length, uint32_t depth, uint32_t nch, const uint8_t* pcm, uint64_t pcm_stride,
                 const uint32_t* frames, const int32_t* status, uint64_t n, const uint64_t* begin, const uint64_t* limit,
                 uint64_t n_clips, uint32_t clip_frames, int type, void* clips, uint64_t channel_stride, uint64_t clip_stride,
                 uint32_t* valid, int32_t* clip_status, uint64_t guard_bytes) {
    if (n_clips && (!pcm || !frames || !begin || !limit || !clips)) return -2;
    if (type != (int)alacwf::kFloat && type != (int)alacwf::kInt) return -2;
    if (!alacwf::bytes_per_sample(depth) || nch < 1 || nch > 8 || !frame_length) return -2;
    if (n > 0x7fffffffu || n_clips > 0x7fffffffu) return -2;
    if (n_clips == 0) return 0;
    if (clip_frames == 0) return -2;
    const uint64_t frame_bytes = (uint64_t)frame_length * nch * alacwf::bytes_per_sample(depth);
    if (n && (pcm_stride < frame_bytes || pcm_stride > SIZE_MAX / n)) return -2;
    if ((uintptr_t)clips & 3u) return -2;
    if (channel_stride < clip_frames || clip_stride / nch < channel_stride || clip_stride > (SIZE_MAX / 8) / n_clips) return -2;

    uint8_t* region = nullptr;
    size_t region_len = 0;
    if (guard_bytes) {
        const size_t page = (size_t)sysconf(_SC_PAGESIZE);
        region_len = (guard_bytes + page - 1) / page * page + page;
        region = (uint8_t*)mmap(nullptr, region_len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (region == MAP_FAILED) return -3;
        uint8_t* copy = region + region_len - page - guard_bytes;
        memcpy(copy, pcm, guard_bytes);
        mprotect(region + region_len - page, page, PROT_NONE);
        pcm = copy;
    }
    Params p = make_params(frame_length, depth, nch, (uint32_t)type, clip_frames);
    p.pcm = pcm;
    p.pcm_stride = pcm_stride;
    p.frames = frames;
    p.status = status;
    p.n = n;
    p.begin = begin;
    p.limit = limit;
    p.n_clips = n_clips;
    p.clips = (uint8_t*)clips;
    p.channel_stride = channel_stride;
    p.clip_stride = clip_stride;
    p.valid = valid;
    p.clip_status = clip_status;
    alignas(16) static thread_local uint8_t stage[kStageBytes];
    static thread_local Seg segs[kMaxSegs];
    for (uint64_t j = 0; j < n_clips; j++)
        for (uint32_t tile = 0; tile < p.tiles_per_clip; tile++) {
            const Tile t = make_tile(p, j, tile);
            memset(stage, 0xA5, sizeof(stage)); /* LDS holds whatever the last workgroup left */
            memset(segs, 0xA5, sizeof(segs));
            for (uint32_t tid = 0; tid < kThreads; tid++) stage_tile(p, t, stage, segs, tid);
            for (uint32_t tid = 0; tid < kThreads; tid++) store_tile(p, t, stage, segs, tid);
        }
    if (valid || clip_status)
        for (uint64_t j = 0; j < n_clips; j++) clip_meta(p, j);
    if (region) munmap(region, region_len);
    return 0;
}

/* the tile shape make_params chooses: columns of a tile, and the staging buffer its segments can take */
uint32_t clip_sim_tile_cols(uint32_t frame_length, uint32_t depth, uint32_t nch) {
    return make_params(frame_length, depth, nch, alacwf::kFloat, 1).tile_cols;
}
uint32_t clip_sim_stage_need(uint32_t frame_length, uint32_t depth, uint32_t nch) {
    const Params p = make_params(frame_length, depth, nch, alacwf::kFloat, 1);
    return max_segs(frame_length, p.tile_cols) * p.pitch;
}
uint32_t clip_sim_stage_bytes(void) { return kStageBytes; }

}  // extern "C"
