/*
 * k_clips.hip — decoded PCM slots -> [clips][channels][clip_frames] crops at arbitrary frame offsets: the gfx950 kernels
 * over csrc/alac_clips.h (one translation unit of libalacgpu.so; nothing here touches the decode or waveform kernels).
 *
 * One gather = these launches on the handle's stream, behind the decode:
 *   alac_clips_gather  one workgroup per tile (tile_cols consecutive columns of one clip, all channels): the tile's slot
 *                      segments with 16-byte loads into LDS, then 16-byte stores of four columns of one channel per lane
 *   alac_clips_meta    one lane per clip: valid[j] and clip_status[j], when the caller asks for either
 * Everything is written with vector stores.
 */
#include <hip/hip_runtime.h>

#include "alac_clips.h"

using namespace alacclip;

namespace {

constexpr int kMetaThreads = 256;
/* alac_clips_gather goes in slices, each far below a dispatch's 2^32 work-items: 2^22 workgroups of 256 */
constexpr uint64_t kTilesPerLaunch = (uint64_t)1 << 22;

__global__ void __launch_bounds__(kThreads) alac_clips_gather(Params p, uint64_t first_tile) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ Seg segs[kMaxSegs];
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t j = b / p.tiles_per_clip;
    if (j >= p.n_clips) return;
    const Tile t = make_tile(p, j, (uint32_t)(b % p.tiles_per_clip));
    stage_tile(p, t, stage, segs, threadIdx.x);
    __syncthreads();
    store_tile(p, t, stage, segs, threadIdx.x);
}

__global__ void __launch_bounds__(kMetaThreads) alac_clips_meta(Params p) {
    const uint64_t j = (uint64_t)blockIdx.x * kMetaThreads + threadIdx.x;
    if (j < p.n_clips) clip_meta(p, j);
}

} /* namespace */

namespace alack {

hipError_t clips_launch(hipStream_t stream, const Params& p) {
    if (p.n_clips == 0) return hipSuccess;
    const uint64_t tiles = p.n_clips * p.tiles_per_clip;
    for (uint64_t t0 = 0; t0 < tiles; t0 += kTilesPerLaunch) {
        const uint64_t m = tiles - t0 < kTilesPerLaunch ? tiles - t0 : kTilesPerLaunch;
        hipLaunchKernelGGL(alac_clips_gather, dim3((unsigned)m), dim3(kThreads), 0, stream, p, t0);
    }
    if (p.valid || p.clip_status) {
        const uint64_t blocks = (p.n_clips + kMetaThreads - 1) / kMetaThreads;
        hipLaunchKernelGGL(alac_clips_meta, dim3((unsigned)blocks), dim3(kMetaThreads), 0, stream, p);
    }
    return hipGetLastError();
}

} /* namespace alack */
