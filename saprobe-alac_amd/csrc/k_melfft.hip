/*
 * k_melfft.hip — the spectrogram pass with transform = fft: the gfx950 kernel over csrc/alac_melfft.h (one translation unit of
 * libalacgpu.so; the handle and its entries are k_mel.hip's, whose own kernel is untouched).
 *
 * One pass = launches of one kernel on the handle's stream:
 *   alac_melfft_rows  one workgroup per tile, as alac_mel_rows: alacmel::stage_tile; then, `batch` frames at a time, window and
 *                     pack into the transform buffer in digit-reversed order, the radix 5 / 3 / 4 / 2 passes in place with the
 *                     whole workgroup over all butterflies of the batch and a barrier behind each, and the split step into the
 *                     power tile; alacmel::mel_tile or log_tile, alacmel::store_tile
 * No matrix instruction, no atomic; everything is written with vector stores.
 */
#include <hip/hip_runtime.h>

#include "alac_host.h"
#include "alac_melfft.h"

using namespace alacmelfft;

namespace {

__global__ void __launch_bounds__(kThreads) alac_melfft_rows(Params p, uint64_t first_tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[]; /* the plan's lds_floats */
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.m.tiles_per_row;
    if (row >= p.m.rows) return;
    const Tile t = alacmel::make_tile(p.m, row, b - row * p.m.tiles_per_row);
    if (t.count == 0) return;
    float* ptile = lds + p.m.a_floats;
    F2* buf = (F2*)(ptile + p.p_floats);
    const uint32_t tid = threadIdx.x;
    alacmel::stage_tile(p.m, t, lds, tid);
    __syncthreads();
    for (uint32_t f0 = 0; f0 < t.count; f0 += p.batch) { /* the batches that hold a frame to store; t.count is uniform */
        pack_batch(p, t, lds, buf, f0, tid);
        __syncthreads();
        for (uint32_t s = 0; s < p.n_pass; s++) {
            pass_batch(p, s, buf, tid);
            __syncthreads();
        }
        split_batch(p, buf, ptile, f0, tid);
        __syncthreads();
    }
    if (p.m.n_mels) alacmel::mel_tile(p.m, ptile, lds, tid); /* the output tile takes the staged inputs' place */
    else alacmel::log_tile(p.m, ptile, tid);
    __syncthreads();
    if (p.m.n_mels) alacmel::store_tile(p.m, t, lds, p.m.tile_frames, 1u, tid);
    else alacmel::store_tile(p.m, t, ptile, 1u, p.m.KP, tid);
}

} /* namespace */

namespace alack {

hipError_t melfft_launch(hipStream_t stream, const Params& p, uint32_t lds_bytes) {
    if (p.m.rows == 0 || p.m.out_frames == 0) return hipSuccess;
    return launch_tiles(alac_melfft_rows, p.m.rows * p.m.tiles_per_row, kThreads, lds_bytes, stream, p);
}

} /* namespace alack */
