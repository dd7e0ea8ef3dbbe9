/*
 * k_wavepack.hip — planar float32 / int32 waveforms -> the encoder's interleaved PCM: the gfx950 kernel over
 * csrc/alac_wavepack.h (one translation unit of libalacgpu.so; nothing here touches the decode or encode kernels, the
 * waveform pass or their launches).
 *
 * One pass = these launches on the encoder handle's stream, in front of an encode:
 *   alac_wave_pack  one workgroup per tile (8 KB of consecutive output frames, all channels): 16-byte loads of four
 *                   frames of one channel per lane, quantised and scattered into an LDS image of the interleaved bytes,
 *                   then 16-byte stores of the image; the workgroup's count of clipped samples goes out with one
 *                   global atomic, and only when it is not zero
 * Everything is written with vector stores and vector atomics.
 */
#include <hip/hip_runtime.h>

#include "alac_wavepack.h"

using namespace alacwp;

namespace {

__global__ void __launch_bounds__(kThreads) alac_wave_pack(Params p, uint64_t first_tile, unsigned long long* __restrict__ clipped) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    __shared__ uint32_t count;
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t seg = b / p.tiles_per_seg;
    if (seg >= p.n_seg) return;
    const Tile t = make_tile(p, seg, b % p.tiles_per_seg);
    if (!t.nf) return;
    if (clipped) {
        if (threadIdx.x == 0) count = 0;
        __syncthreads();
    }
    const uint32_t mine = load_tile(p, t, stage, threadIdx.x);
    if (clipped && mine) atomicAdd(&count, mine);
    __syncthreads();
    store_tile(p, t, stage, threadIdx.x);
    if (clipped && threadIdx.x == 0 && count) atomicAdd(clipped, (unsigned long long)count);
}

} /* namespace */

namespace alack {

hipError_t wavepack_launch(hipStream_t stream, Params p, uint64_t* d_clipped, uint64_t tiles_per_launch) {
    if (d_clipped) {
        const hipError_t e = hipMemsetAsync(d_clipped, 0, sizeof(uint64_t), stream);
        if (e != hipSuccess) return e;
    }
    const uint64_t tiles = p.n_seg * p.tiles_per_seg;
    const uint64_t slices = slice_count(tiles, tiles_per_launch);
    for (uint64_t k = 0; k < slices; k++) {
        const Slice s = slice_of(tiles, tiles_per_launch, k);
        hipLaunchKernelGGL(alac_wave_pack, dim3((unsigned)s.count), dim3(kThreads), 0, stream, p, s.first, (unsigned long long*)d_clipped);
    }
    return hipGetLastError();
}

} /* namespace alack */
