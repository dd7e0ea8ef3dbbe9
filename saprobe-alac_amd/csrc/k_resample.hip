/*
 * k_resample.hip — float32 rows at one sample rate -> another (torchaudio's sinc_interp_hann): the gfx950 kernel over
 * csrc/alac_resample.h and the resampler handle's entries (one translation unit of libalacgpu.so; nothing here touches the
 * decode, waveform, clip or encode kernels).
 *
 * One pass = launches of one kernel on the handle's stream:
 *   alac_resample_rows  one workgroup per tile (tile_out consecutive columns of one output row): the tile's inputs with
 *                       16-byte loads into LDS, zeros outside the row; every lane the fmaf chains of up to four columns,
 *                       table entries from global memory ([taps][n]: a wave reads consecutive addresses), inputs from LDS;
 *                       the results through LDS into 16-byte stores
 * Everything is written with vector stores.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "alac_host.h"
#include "alac_resample.h"

using namespace alacrs;
using alack::set_err;

namespace {

__global__ void __launch_bounds__(kThreads) alac_resample_rows(Params p, uint64_t first_tile) {
    __shared__ __attribute__((aligned(16))) float stage[kStageFloats];
    __shared__ __attribute__((aligned(16))) float outb[kOutFloats];
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.tiles_per_row;
    if (row >= p.rows) return;
    const Tile t = make_tile(p, row, b - row * p.tiles_per_row);
    if (t.count == 0) return;
    stage_tile(p, t, stage, threadIdx.x);
    __syncthreads();
    compute_tile(p, t, stage, outb, threadIdx.x);
    __syncthreads();
    store_tile(p, t, outb, threadIdx.x);
}

} /* namespace */

namespace alack {

hipError_t resample_launch(hipStream_t stream, const Params& p) {
    if (p.rows == 0 || p.out_frames == 0) return hipSuccess;
    return launch_tiles(alac_resample_rows, p.rows * p.tiles_per_row, kThreads, 0, stream, p);
}

} /* namespace alack */

/* ---- host side (alac_host.h) ---------------------------------------------------------------------------------------- */
struct __attribute__((visibility("hidden"))) alacgpu_resampler : alack::PassHandle { /* hidden: its destructor is no export */
    Plan plan;
    float* d_ht = nullptr;
    int32_t* d_first = nullptr;
};

extern "C" {

int alacgpu_resampler_create(int device, uint32_t orig_freq, uint32_t new_freq, uint32_t lowpass_filter_width, double rolloff,
                             alacgpu_resampler** out) {
    if (!out) return alack::null_argument();
    *out = nullptr;
    alacgpu_resampler* r = new (std::nothrow) alacgpu_resampler();
    if (!r) {
        set_err("out of memory");
        return ALACGPU_E_ARG;
    }
    if (!make_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, &r->plan)) {
        set_err("no resampling plan for %u -> %u Hz, width %u, rolloff %g: the rates must be positive and differ, the width "
                "positive, rolloff in (0, 1], the table at most %llu bytes and the inputs of 64 outputs at most %u",
                orig_freq, new_freq, lowpass_filter_width, rolloff, (unsigned long long)kMaxTableBytes, kStageFloats);
        delete r;
        return ALACGPU_E_ARG;
    }
    r->open(device);
    r->upload(&r->d_ht, r->plan.ht);
    r->upload(&r->d_first, r->plan.first);
    if (r->err != hipSuccess) {
        set_err("resampler creation failed: %s", hipGetErrorString(r->err));
        alacgpu_resampler_destroy(r);
        return ALACGPU_E_HIP;
    }
    *out = r;
    return ALACGPU_E_OK;
}

void alacgpu_resampler_destroy(alacgpu_resampler* r) {
    if (!r) return;
    r->close();
    delete r;
}

void* alacgpu_resampler_stream(alacgpu_resampler* r) { return r ? (void*)r->stream : nullptr; }

int alacgpu_resampler_synchronize(alacgpu_resampler* r) { return r ? r->synchronize() : ALACGPU_E_ARG; }

int alacgpu_resampler_last_ms(alacgpu_resampler* r, float* ms) { return r ? r->last_ms(ms, "resampling") : alack::null_argument(); }

uint64_t alacgpu_resample_out_frames(const alacgpu_resampler* r, uint64_t in_frames) {
    uint64_t of = 0;
    if (!r || !out_frames_of(r->plan.o, r->plan.n, in_frames, &of)) return 0;
    return of;
}

int alacgpu_resampler_plan(const alacgpu_resampler* r, alacgpu_resample_info* info, float* h_out, size_t h_cap,
                           int32_t* first_out, size_t first_cap) {
    if (!r || !info) return alack::null_argument();
    const Plan& pl = r->plan;
    if ((h_out && h_cap < pl.h.size()) || (first_out && first_cap < pl.first.size())) {
        set_err("capacity below the plan's %zu table entries / %zu phases", pl.h.size(), pl.first.size());
        return ALACGPU_E_ARG;
    }
    info->o = pl.o;
    info->n = pl.n;
    info->width = pl.width;
    info->taps = pl.taps;
    info->tile_out = pl.tile_out;
    if (h_out) memcpy(h_out, pl.h.data(), pl.h.size() * sizeof(float));
    if (first_out) memcpy(first_out, pl.first.data(), pl.first.size() * sizeof(int32_t));
    return ALACGPU_E_OK;
}

int alacgpu_resample_device(alacgpu_resampler* r, const float* d_in, size_t in_row_stride, size_t rows, size_t in_frames,
                            float* d_out, size_t out_row_stride, int sync) {
    if (!r) return alack::null_argument();
    if (rows == 0 || in_frames == 0) return ALACGPU_E_OK;
    Params p;
    if (!make_params(r->plan, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, r->d_ht, r->d_first, &p)) {
        set_err("resample: a NULL or misaligned buffer, a row stride (%zu in, %zu out) below the row's %zu / %llu frames, or sizes "
                "that overflow", in_row_stride, out_row_stride, in_frames,
                (unsigned long long)alacgpu_resample_out_frames(r, in_frames));
        return ALACGPU_E_ARG;
    }
    return r->run(sync, [&](hipStream_t s) { return alack::resample_launch(s, p); });
}

} /* extern "C" */
