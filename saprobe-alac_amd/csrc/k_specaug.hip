/*
 * k_specaug.hip — SpecAugment with per-row lengths: the gfx950 kernel over csrc/alac_specaug.h and the handle's entries (one
 * translation unit of libalacgpu.so; nothing here touches the normalisation pass, the stacking pass or any other kernel).
 *
 * One pass = one launch on the handle's stream:
 *   alac_specaug  one workgroup per (row, tile_out output frames): the row's draws into LDS by the first wave, each frame's source
 *                 frames and weight once by the first tile_out work items, the tile of y into an LDS image with loads along the
 *                 input's contiguous axis, masks and padding applied as it is written, the image out along the output's
 *                 contiguous axis. Tile 0 of a row writes its draws.
 * No atomic; everything is written with vector stores.
 */
#include <hip/hip_runtime.h>

#include "alac_specaug.h"
#include "alac_host.h"

using namespace alacsa;
using alack::set_err;

namespace {

__global__ void __launch_bounds__(kThreads) alac_specaug(Params p, uint64_t first_tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[]; /* plan_of(config).lds_words */
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.tiles;
    if (row >= p.rows) return;
    const Tile t = make_tile(p, row, b - row * p.tiles);
    const Lds l = carve(p, lds);
    const uint32_t tid = threadIdx.x;
    resolve_draws(p, t, l.draws, tid);
    __syncthreads();
    frame_plan(p, t, l, tid);
    bin_plan(p, l, tid);
    __syncthreads();
    build_image(p, t, l, tid);
    __syncthreads();
    store_image(p, t, l, tid);
}

} /* namespace */

namespace alack {

hipError_t specaug_launch(hipStream_t stream, const Params& p, uint32_t lds_bytes) {
    if (p.rows == 0 || p.frames == 0) return hipSuccess;
    return launch_tiles(alac_specaug, p.rows * p.tiles, kThreads, lds_bytes, stream, p);
}

} /* namespace alack */

/* ---- host side (alac_host.h) ---------------------------------------------------------------------------------------- */
struct __attribute__((visibility("hidden"))) alacgpu_specaug : alack::PassHandle { /* hidden: its destructor is no export */
    Config cfg{};
    Plan plan{};
};

extern "C" {

int alacgpu_specaug_create(int device, const alacgpu_specaug_config* config, alacgpu_specaug** out) {
    if (!out) return alack::null_argument();
    *out = nullptr;
    if (!config) return alack::null_argument();
    const Config c{config->bins,           config->freq_masks, config->freq_width, config->time_masks, config->time_width,
                   config->time_ratio_q16, config->warp,       config->mask_value, config->pad_value};
    if (!config_ok(c)) {
        set_err("no SpecAugment plan: bins %u outside [1, %u], freq_masks %u above %u, freq_width %u above the bins, time_masks %u "
                "above %u, time_width %u above %u, time_ratio_q16 %u above %u, or warp %u above %u", c.bins, kMaxBins, c.freq_masks,
                kMaxFreqMasks, c.freq_width, c.time_masks, kMaxTimeMasks, c.time_width, kMaxTimeWidth, c.time_ratio_q16, kMaxRatioQ16,
                c.warp, kMaxWarp);
        return ALACGPU_E_ARG;
    }
    alacgpu_specaug* h = new (std::nothrow) alacgpu_specaug();
    if (!h) {
        set_err("out of memory");
        return ALACGPU_E_ARG;
    }
    h->cfg = c;
    h->plan = plan_of(c);
    h->open(device);
    if (h->err != hipSuccess) {
        set_err("SpecAugment handle creation failed: %s", hipGetErrorString(h->err));
        alacgpu_specaug_destroy(h);
        return ALACGPU_E_HIP;
    }
    *out = h;
    return ALACGPU_E_OK;
}

void alacgpu_specaug_destroy(alacgpu_specaug* h) {
    if (!h) return;
    h->close();
    delete h;
}

void* alacgpu_specaug_stream(alacgpu_specaug* h) { return h ? (void*)h->stream : nullptr; }

int alacgpu_specaug_synchronize(alacgpu_specaug* h) { return h ? h->synchronize() : ALACGPU_E_ARG; }

int alacgpu_specaug_last_ms(alacgpu_specaug* h, float* ms) { return h ? h->last_ms(ms, "SpecAugment") : alack::null_argument(); }

int alacgpu_specaug_plan(const alacgpu_specaug* h, alacgpu_specaug_info* info) {
    if (!h || !info) return alack::null_argument();
    info->bins = h->cfg.bins;
    info->freq_masks = h->cfg.freq_masks;
    info->freq_width = h->cfg.freq_width;
    info->time_masks = h->cfg.time_masks;
    info->time_width = h->cfg.time_width;
    info->time_ratio_q16 = h->cfg.time_ratio_q16;
    info->warp = h->cfg.warp;
    info->draws = h->plan.draws;
    info->tile_out = h->plan.tile_out;
    info->lds_bytes = h->plan.lds_words * 4u;
    info->mask_value = h->cfg.mask_value;
    info->pad_value = h->cfg.pad_value;
    return ALACGPU_E_OK;
}

int alacgpu_specaug_device(alacgpu_specaug* h, const float* d_in, size_t in_row_stride, size_t in_frame_stride, size_t in_bin_stride,
                           size_t rows, size_t frames, const int32_t* d_lengths, uint64_t seed, uint64_t row_base, const int64_t* d_ids,
                           float* d_out, size_t out_row_stride, size_t out_frame_stride, size_t out_bin_stride, int32_t* d_draws,
                           int sync) {
    if (!h) return alack::null_argument();
    if (rows == 0 || frames == 0) return ALACGPU_E_OK;
    Params p;
    if (!make_params(h->cfg, h->plan, d_in, in_row_stride, in_frame_stride, in_bin_stride, rows, frames, d_lengths, seed, row_base, d_ids,
                     d_out, out_row_stride, out_frame_stride, out_bin_stride, d_draws, &p)) {
        set_err("specaug: a NULL or misaligned buffer, strides (%zu, %zu, %zu in; %zu, %zu, %zu out) of which neither inner one is 1 "
                "or whose axes run into each other, a row stride below the row's extent (%zu frames x %u bins), an output that "
                "overlaps the input (in place takes the input's own base and strides on a handle without a warp), frames above "
                "2^31 - 1, or sizes that overflow", in_row_stride, in_frame_stride, in_bin_stride, out_row_stride, out_frame_stride,
                out_bin_stride, frames, h->cfg.bins);
        return ALACGPU_E_ARG;
    }
    const uint32_t lds_bytes = h->plan.lds_words * 4u;
    return h->run(sync, [&](hipStream_t s) { return alack::specaug_launch(s, p, lds_bytes); });
}

} /* extern "C" */
