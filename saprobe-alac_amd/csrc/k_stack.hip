/*
 * k_stack.hip — deltas, context splicing and subsampling with per-row lengths: the gfx950 kernel over csrc/alac_stack.h and the
 * handle's entries (one translation unit of libalacgpu.so; nothing here touches the normalisation pass or any other kernel).
 *
 * One pass = one launch on the handle's stream:
 *   alac_stack  one workgroup per (row, tile_out output frames): per slab of bins the tile's input frames into LDS with loads
 *               along the contiguous axis, d_1 and d_2 once each into LDS behind them, the output out of LDS along its contiguous
 *               axis; the padding frames straight from pad_value. Tile 0 of a row writes its out_lengths.
 * No atomic; everything is written with vector stores.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "alac_stack.h"
#include "alac_host.h"

using namespace alacst;
using alack::set_err;

namespace {

__global__ void __launch_bounds__(kThreads) alac_stack(Params p, uint64_t first_tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[]; /* plan_of(config).lds_floats */
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.tiles;
    if (row >= p.rows) return;
    const Tile t = make_tile(p, row, b - row * p.tiles);
    const uint32_t tid = threadIdx.x;
    put_length(p, t, tid);
    for (uint32_t b0 = 0; b0 < p.bins; b0 += p.tile_bins) { /* t.gv and the slabs are the workgroup's: every barrier is uniform */
        if (b0) __syncthreads();
        if (t.gv) {
            stage_slab(p, t, b0, lds, tid);
            __syncthreads();
            if (p.order) {
                delta_slab(p, t, b0, lds, tid);
                __syncthreads();
            }
        }
        store_slab(p, t, b0, lds, tid);
    }
}

} /* namespace */

namespace alack {

hipError_t stack_launch(hipStream_t stream, const Params& p, uint32_t lds_bytes) {
    if (p.rows == 0 || p.frames == 0) return hipSuccess;
    return launch_tiles(alac_stack, p.rows * p.tiles, kThreads, lds_bytes, stream, p);
}

} /* namespace alack */

/* ---- host side (alac_host.h) ---------------------------------------------------------------------------------------- */
struct __attribute__((visibility("hidden"))) alacgpu_stack : alack::PassHandle { /* hidden: its destructor is no export */
    Config cfg{};
    Plan plan{};
    std::vector<float> weights; /* w_1 then w_2 */
    uint32_t counts[2] = {0u, 0u};
    float* d_weights = nullptr;
};

extern "C" {

int alacgpu_stack_create(int device, const alacgpu_stack_config* config, alacgpu_stack** out) {
    if (!out) return alack::null_argument();
    *out = nullptr;
    if (!config) return alack::null_argument();
    const Config c{config->bins, config->order, config->window, config->left, config->right, config->stride, config->pad_value};
    if (!config_ok(c)) {
        set_err("no stacking plan: bins %u outside [1, %u], order %u above %u, window %u outside [1, %u] with an order above 0, left "
                "%u or right %u above %u, stride %u outside [1, %u], or more than %u output columns", c.bins, kMaxBins, c.order,
                kMaxOrder, c.window, kMaxWindow, c.left, c.right, kMaxContext, c.stride, kMaxStride, kMaxCols);
        return ALACGPU_E_ARG;
    }
    alacgpu_stack* h = new (std::nothrow) alacgpu_stack();
    if (!h) {
        set_err("out of memory");
        return ALACGPU_E_ARG;
    }
    h->cfg = c;
    h->plan = plan_of(c);
    h->weights.resize(kMaxWeights);
    h->weights.resize(make_weights(c.order, c.window, h->weights.data(), h->counts));
    h->open(device);
    h->upload(&h->d_weights, h->weights);
    if (h->err != hipSuccess) {
        set_err("stacking handle creation failed: %s", hipGetErrorString(h->err));
        alacgpu_stack_destroy(h);
        return ALACGPU_E_HIP;
    }
    *out = h;
    return ALACGPU_E_OK;
}

void alacgpu_stack_destroy(alacgpu_stack* h) {
    if (!h) return;
    h->close();
    delete h;
}

void* alacgpu_stack_stream(alacgpu_stack* h) { return h ? (void*)h->stream : nullptr; }

int alacgpu_stack_synchronize(alacgpu_stack* h) { return h ? h->synchronize() : ALACGPU_E_ARG; }

int alacgpu_stack_last_ms(alacgpu_stack* h, float* ms) { return h ? h->last_ms(ms, "stacking") : alack::null_argument(); }

uint64_t alacgpu_stack_out_frames(const alacgpu_stack* h, uint64_t in_frames) { return h ? out_frames_of(h->cfg, in_frames) : 0; }

int alacgpu_stack_plan(const alacgpu_stack* h, alacgpu_stack_info* info, float* weights_out, size_t weights_cap) {
    if (!h || !info) return alack::null_argument();
    if (weights_out && weights_cap < h->weights.size()) {
        set_err("capacity below the plan's %zu weights", h->weights.size());
        return ALACGPU_E_ARG;
    }
    info->bins = h->cfg.bins;
    info->order = h->cfg.order;
    info->window = h->cfg.order ? h->cfg.window : 0u;
    info->left = h->cfg.left;
    info->right = h->cfg.right;
    info->stride = h->cfg.stride;
    info->columns = h->plan.cols;
    info->tile_out = h->plan.tile_out;
    info->tile_in = h->plan.tile_in;
    info->tile_bins = h->plan.tile_bins;
    info->lds_bytes = h->plan.lds_floats * (uint32_t)sizeof(float);
    info->w1_entries = h->counts[0];
    info->w2_entries = h->counts[1];
    if (weights_out && !h->weights.empty()) memcpy(weights_out, h->weights.data(), h->weights.size() * sizeof(float));
    return ALACGPU_E_OK;
}

int alacgpu_stack_device(alacgpu_stack* h, const float* d_in, size_t in_row_stride, size_t in_frame_stride, size_t in_bin_stride,
                         size_t rows, size_t frames, const int32_t* d_lengths, float* d_out, size_t out_row_stride,
                         size_t out_frame_stride, size_t out_bin_stride, int32_t* d_out_lengths, int sync) {
    if (!h) return alack::null_argument();
    if (rows == 0 || frames == 0) return ALACGPU_E_OK;
    Params p;
    if (!make_params(h->cfg, h->plan, d_in, in_row_stride, in_frame_stride, in_bin_stride, rows, frames, d_lengths, d_out,
                     out_row_stride, out_frame_stride, out_bin_stride, d_out_lengths, h->d_weights, &p)) {
        set_err("stack: a NULL or misaligned buffer, strides (%zu, %zu, %zu in; %zu, %zu, %zu out) of which neither inner one is 1 or "
                "whose axes run into each other, a row stride below the row's extent (%zu frames x %u bins in, %llu frames x %u "
                "columns out), an output that overlaps the input, or sizes that overflow", in_row_stride, in_frame_stride,
                in_bin_stride, out_row_stride, out_frame_stride, out_bin_stride, frames, h->cfg.bins,
                (unsigned long long)out_frames_of(h->cfg, frames), h->plan.cols);
        return ALACGPU_E_ARG;
    }
    const uint32_t lds_bytes = h->plan.lds_floats * (uint32_t)sizeof(float);
    return h->run(sync, [&](hipStream_t s) { return alack::stack_launch(s, p, lds_bytes); });
}

} /* extern "C" */
