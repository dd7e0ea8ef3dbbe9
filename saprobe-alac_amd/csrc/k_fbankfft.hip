/*
 * k_fbankfft.hip — the Kaldi feature pass with transform = fft: the gfx950 kernel over csrc/alac_fbankfft.h (one translation unit
 * of libalacgpu.so; the handle and its entries are k_fbank.hip's, whose own kernel is untouched).
 *
 * One pass = launches of one kernel on the handle's stream:
 *   alac_fbankfft_rows  one workgroup per tile, as alac_fbank_rows: alacfb::stage_tile; the energies and, with all 256 work
 *                       items, the frames' sums by residue classes and a tree, the mean by one division per frame; then,
 *                       `batch` frames at a time, mean removal, pre-emphasis, window and pack into the transform buffer in
 *                       digit-reversed order, the radix 5 / 3 / 4 / 2 passes in place and the split step into the power tile
 *                       (alac_melfft.h's); the mel chains, the log, the DCT and the stores of alac_fbank.h
 * No matrix instruction, no atomic; everything is written with vector stores.
 */
#include <hip/hip_runtime.h>

#include "alac_fbankfft.h"
#include "alac_host.h"

using namespace alacfbfft;

namespace {

__global__ void __launch_bounds__(kThreads) alac_fbankfft_rows(Params p, uint64_t first_tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[]; /* the plan's lds_floats */
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.fb.m.tiles_per_row;
    if (row >= p.fb.m.rows) return;
    const Tile t = alacfb::make_tile(p.fb, row, b - row * p.fb.m.tiles_per_row);
    if (t.count == 0) return;
    const uint32_t tid = threadIdx.x;
    for_each_phase(p, t, [&](uint32_t phase, uint32_t arg) {
        tile_phase(p, t, lds, phase, arg, tid);
        __syncthreads();
    });
}

} /* namespace */

namespace alack {

hipError_t fbankfft_launch(hipStream_t stream, const Params& p, uint32_t lds_bytes) {
    if (p.fb.m.rows == 0 || p.fb.m.out_frames == 0) return hipSuccess;
    return launch_tiles(alac_fbankfft_rows, p.fb.m.rows * p.fb.m.tiles_per_row, kThreads, lds_bytes, stream, p);
}

} /* namespace alack */
