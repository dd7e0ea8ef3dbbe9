/*
 * k_wave.hip — decoded PCM slots -> planar float32 / int32 waveforms: the gfx950 kernels over csrc/alac_waveform.h (one
 * translation unit of libalacgpu.so; nothing here touches the decode kernels or their launches).
 *
 * One pass = these launches on the handle's stream, behind the decode:
 *   alac_wave_sums     one lane per packet: f[i]; the workgroup's sum            } STREAM, or whenever the caller asks
 *   alac_wave_scan     one workgroup: exclusive scan of the workgroup sums       } for d_starts
 *   alac_wave_offsets  one lane per packet: start[i]; start[n] = the total       }
 *   alac_wave_convert  one workgroup per tile (8 KB of consecutive frames of one packet, all channels): 16-byte loads
 *                      into LDS, then 16-byte stores of four frames of one channel per lane
 * Everything is written with vector stores.
 */
#include <hip/hip_runtime.h>

#include "alac_waveform.h"

using namespace alacwf;

namespace {

constexpr int kScanThreads = 256;
/* alac_wave_convert goes in slices, each far below a dispatch's 2^32 work-items: 2^22 workgroups of 256 */
constexpr uint64_t kTilesPerLaunch = (uint64_t)1 << 22;

/* block-wide inclusive scan of one uint64 per thread (kScanThreads threads) */
__device__ uint64_t block_scan(uint64_t v, uint64_t* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const uint64_t add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    return sh[t];
}

__global__ void __launch_bounds__(kScanThreads) alac_wave_sums(Params p, uint64_t* __restrict__ block_sums) {
    __shared__ uint64_t sh[kScanThreads];
    const uint64_t pk = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const uint64_t sum = block_scan(pk < p.n ? frames_of(p, pk) : 0u, sh);
    if (threadIdx.x == kScanThreads - 1) block_sums[blockIdx.x] = sum;
}

/* one workgroup: block_sums[b] -> exclusive prefix; starts[n] = total */
__global__ void __launch_bounds__(kScanThreads) alac_wave_scan(uint64_t* __restrict__ block_sums, uint64_t nblocks,
                                                               uint64_t* __restrict__ starts, uint64_t n) {
    __shared__ uint64_t sh[kScanThreads];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nblocks; base += kScanThreads) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < nblocks ? block_sums[i] : 0;
        const uint64_t inc = block_scan(v, sh);
        if (i < nblocks) block_sums[i] = carry + inc - v;
        carry += sh[kScanThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) starts[n] = carry;
}

__global__ void __launch_bounds__(kScanThreads) alac_wave_offsets(Params p, const uint64_t* __restrict__ block_base,
                                                                  uint64_t* __restrict__ starts) {
    __shared__ uint64_t sh[kScanThreads];
    const uint64_t pk = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const uint32_t f = pk < p.n ? frames_of(p, pk) : 0u;
    const uint64_t inc = block_scan(f, sh);
    if (pk < p.n) starts[pk] = block_base[blockIdx.x] + inc - f;
}

__global__ void __launch_bounds__(kThreads) alac_wave_convert(Params p, uint64_t first_tile) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t pk = b / p.tiles_per_packet;
    if (pk >= p.n) return;
    const Tile t = make_tile(p, pk, (uint32_t)(b % p.tiles_per_packet));
    if (!t.any) return;
    stage_tile(p, t, stage, threadIdx.x);
    __syncthreads();
    store_tile(p, t, stage, threadIdx.x);
}

} /* namespace */

namespace alack {

size_t wave_scratch_bytes(size_t n) {
    const size_t blocks = (n + kScanThreads - 1) / kScanThreads;
    return (blocks + n + 1) * sizeof(uint64_t);
}

hipError_t wave_launch(hipStream_t stream, Params p, uint64_t* d_starts, void* scratch) {
    const uint64_t n = p.n;
    const uint64_t blocks = (n + kScanThreads - 1) / kScanThreads;
    uint64_t* sums = (uint64_t*)scratch;
    uint64_t* starts = d_starts ? d_starts : sums + blocks;
    if (n == 0) return d_starts ? hipMemsetAsync(d_starts, 0, sizeof(uint64_t), stream) : hipSuccess;
    if (p.layout == kStream || d_starts) {
        hipLaunchKernelGGL(alac_wave_sums, dim3((unsigned)blocks), dim3(kScanThreads), 0, stream, p, sums);
        hipLaunchKernelGGL(alac_wave_scan, dim3(1), dim3(kScanThreads), 0, stream, sums, blocks, starts, n);
        hipLaunchKernelGGL(alac_wave_offsets, dim3((unsigned)blocks), dim3(kScanThreads), 0, stream, p, (const uint64_t*)sums, starts);
    }
    p.starts = starts;
    const uint64_t tiles = n * p.tiles_per_packet;
    for (uint64_t t0 = 0; t0 < tiles; t0 += kTilesPerLaunch) {
        const uint64_t m = tiles - t0 < kTilesPerLaunch ? tiles - t0 : kTilesPerLaunch;
        hipLaunchKernelGGL(alac_wave_convert, dim3((unsigned)m), dim3(kThreads), 0, stream, p, t0);
    }
    return hipGetLastError();
}

} /* namespace alack */
