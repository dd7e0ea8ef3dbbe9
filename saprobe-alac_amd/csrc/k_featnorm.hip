/*
 * k_featnorm.hip — feature normalisation with per-row lengths (CMVN, max-clamp, affine, padding): the gfx950 kernels over
 * csrc/alac_featnorm.h and the handle's entries (one translation unit of libalacgpu.so; nothing here touches the feature
 * kernels or any other).
 *
 * One pass = these launches on the handle's stream, in alacfn::for_each_launch's order:
 *   alac_featnorm_partials  one workgroup per (row, chunk of tile_frames frames) that holds a valid frame: the chunk into LDS
 *                           with loads along the contiguous axis; a lane per bin walks the frames for the chunk's sum (of x,
 *                           or of (x - mean)^2), or all lanes for the chunk's maximum
 *   alac_featnorm_finish    per row: the chunks' partial sums in chunk order -> mean, or rstd; or their maximum
 *   alac_featnorm_apply     one workgroup per (row, chunk): the chunk into LDS, statistic, affine and padding in LDS, the
 *                           chunk out along the output's contiguous axis
 * stat none is the apply kernel alone; mean_var runs the first two twice. No atomic; everything is written with vector stores.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "alac_featnorm.h"
#include "alac_host.h"

using namespace alacfn;
using alack::set_err;

namespace {

__global__ void __launch_bounds__(kThreads) alac_featnorm_partials(Params p, uint64_t first_tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[]; /* lds_floats_of(bins, tile_frames) */
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.chunks;
    if (row >= p.rows) return;
    const Tile t = make_tile(p, row, b - row * p.chunks);
    if (t.nv == 0) return;
    const uint32_t tid = threadIdx.x;
    stage_tile(p, t, lds, tid);
    __syncthreads();
    if (p.phase != kLargest) {
        sum_tile(p, t, lds, tid);
        return;
    }
    int32_t* red = (int32_t*)(lds + image_floats_of(p.bins, p.tile_frames));
    max_tile(p, t, lds, red, tid);
    __syncthreads();
    reduce_keys(red, 0u, tid);
    __syncthreads();
    reduce_keys(red, 1u, tid);
    __syncthreads();
    put_tile_max(p, t, red, tid);
}

/* sums: block = (row, 256 bins); maximum: block = row */
__global__ void __launch_bounds__(kThreads) alac_featnorm_finish(Params p, uint64_t first_tile) {
    __shared__ int32_t red[kRed];
    const uint64_t b = first_tile + blockIdx.x;
    const uint32_t tid = threadIdx.x;
    if (p.phase != kLargest) {
        const uint32_t blocks = (p.bins + kThreads - 1u) / kThreads;
        const uint64_t row = b / blocks;
        const uint32_t bin = (uint32_t)(b - row * blocks) * kThreads + tid;
        if (row < p.rows && bin < p.bins) finish_bin(p, row, bin);
        return;
    }
    if (b >= p.rows) return;
    row_max(p, b, red, tid);
    __syncthreads();
    reduce_keys(red, 0u, tid);
    __syncthreads();
    reduce_keys(red, 1u, tid);
    __syncthreads();
    put_row_max(p, b, red, tid);
}

__global__ void __launch_bounds__(kThreads) alac_featnorm_apply(Params p, uint64_t first_tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.chunks;
    if (row >= p.rows) return;
    const Tile t = make_tile(p, row, b - row * p.chunks);
    const uint32_t tid = threadIdx.x;
    if (t.nv) stage_tile(p, t, lds, tid);
    __syncthreads();
    apply_tile(p, t, lds, tid);
    __syncthreads();
    store_tile(p, t, lds, tid);
}

} /* namespace */

namespace alack {

hipError_t featnorm_launch(hipStream_t stream, const Params& p, uint32_t lds_bytes) {
    if (p.rows == 0 || p.frames == 0) return hipSuccess;
    hipError_t err = hipSuccess;
    for_each_launch(p.stat, [&](uint32_t kernel, uint32_t phase) {
        if (err != hipSuccess) return;
        Params q = p;
        q.phase = phase;
        if (kernel == 0u) err = launch_tiles(alac_featnorm_partials, q.rows * q.chunks, kThreads, lds_bytes, stream, q);
        else if (kernel == 1u)
            err = launch_tiles(alac_featnorm_finish, phase == kLargest ? q.rows : q.rows * ((q.bins + kThreads - 1u) / kThreads),
                               kThreads, 0, stream, q);
        else err = launch_tiles(alac_featnorm_apply, q.rows * q.chunks, kThreads, lds_bytes, stream, q);
    });
    return err;
}

} /* namespace alack */

/* ---- host side (alac_host.h) ---------------------------------------------------------------------------------------- */
struct __attribute__((visibility("hidden"))) alacgpu_norm : alack::PassHandle { /* hidden: its destructor is no export */
    Config cfg{};
    std::vector<float> shift, scale; /* empty: none */
    float* d_shift = nullptr;
    float* d_scale = nullptr;
    alack::DevBuf scratch; /* the partials and, where the caller keeps none, the stats: grows, never shrinks */
};

extern "C" {

int alacgpu_norm_create(int device, const alacgpu_norm_config* config, const float* shift, const float* scale, alacgpu_norm** out) {
    if (!out) return alack::null_argument();
    *out = nullptr;
    if (!config) return alack::null_argument();
    const Config c{config->bins, config->stat, config->var_floor, config->range, config->pad_value};
    if (!config_ok(c)) {
        set_err("no normalisation plan: bins %u outside [1, %u], stat %u above %u, var_floor %g not above 0, or stat max with a "
                "range %g that is negative or no number", c.bins, kMaxBins, c.stat, kMax, (double)c.var_floor, (double)c.range);
        return ALACGPU_E_ARG;
    }
    alacgpu_norm* h = new (std::nothrow) alacgpu_norm();
    if (!h) {
        set_err("out of memory");
        return ALACGPU_E_ARG;
    }
    h->cfg = c;
    if (shift) h->shift.assign(shift, shift + c.bins);
    if (scale) h->scale.assign(scale, scale + c.bins);
    h->open(device);
    if (shift) h->upload(&h->d_shift, h->shift);
    if (scale) h->upload(&h->d_scale, h->scale);
    if (h->err == hipSuccess) h->err = (hipError_t)(h->scratch.ensure(256) == ALACGPU_E_OK ? hipSuccess : hipErrorOutOfMemory);
    if (h->err != hipSuccess) {
        set_err("normalisation handle creation failed: %s", hipGetErrorString(h->err));
        alacgpu_norm_destroy(h);
        return ALACGPU_E_HIP;
    }
    *out = h;
    return ALACGPU_E_OK;
}

void alacgpu_norm_destroy(alacgpu_norm* h) {
    if (!h) return;
    h->close();
    h->scratch.release();
    delete h;
}

void* alacgpu_norm_stream(alacgpu_norm* h) { return h ? (void*)h->stream : nullptr; }

int alacgpu_norm_synchronize(alacgpu_norm* h) { return h ? h->synchronize() : ALACGPU_E_ARG; }

int alacgpu_norm_last_ms(alacgpu_norm* h, float* ms) { return h ? h->last_ms(ms, "normalisation") : alack::null_argument(); }

uint64_t alacgpu_norm_out_frames(const alacgpu_norm* h, uint64_t in_frames) { return h ? in_frames : 0; }

int alacgpu_norm_plan(const alacgpu_norm* h, alacgpu_norm_info* info, float* shift_out, size_t shift_cap, float* scale_out,
                      size_t scale_cap) {
    if (!h || !info) return alack::null_argument();
    if ((shift_out && shift_cap < h->shift.size()) || (scale_out && scale_cap < h->scale.size())) {
        set_err("capacity below the plan's %zu shift / %zu scale entries", h->shift.size(), h->scale.size());
        return ALACGPU_E_ARG;
    }
    info->bins = h->cfg.bins;
    info->stat = h->cfg.stat;
    info->tile_frames = tile_frames_of(h->cfg.bins);
    info->lds_bytes = lds_floats_of(h->cfg.bins, info->tile_frames) * (uint32_t)sizeof(float);
    info->shift_entries = (uint32_t)h->shift.size();
    info->scale_entries = (uint32_t)h->scale.size();
    info->scratch_bytes = h->scratch.cap;
    info->scratch_address = (uint64_t)(uintptr_t)h->scratch.p;
    if (shift_out && !h->shift.empty()) memcpy(shift_out, h->shift.data(), h->shift.size() * sizeof(float));
    if (scale_out && !h->scale.empty()) memcpy(scale_out, h->scale.data(), h->scale.size() * sizeof(float));
    return ALACGPU_E_OK;
}

int alacgpu_norm_device(alacgpu_norm* h, const float* d_in, size_t in_row_stride, size_t in_frame_stride, size_t in_bin_stride,
                        size_t rows, size_t frames, const int32_t* d_lengths, float* d_out, size_t out_row_stride,
                        size_t out_frame_stride, size_t out_bin_stride, float* d_stats, int sync) {
    if (!h) return alack::null_argument();
    if (rows == 0 || frames == 0) return ALACGPU_E_OK;
    uint64_t floats = 0;
    Params p;
    if (!scratch_floats_of(h->cfg, rows, frames, d_stats == nullptr, &floats) ||
        !make_params(h->cfg, d_in, in_row_stride, in_frame_stride, in_bin_stride, rows, frames, d_lengths, d_out, out_row_stride,
                     out_frame_stride, out_bin_stride, d_stats, h->d_shift, h->d_scale, &p)) {
        set_err("normalise: a NULL or misaligned buffer, strides (%zu, %zu, %zu in; %zu, %zu, %zu out) of which neither inner one is "
                "1 or whose axes run into each other, a row stride below the row's extent of %zu frames x %u bins, or sizes that "
                "overflow", in_row_stride, in_frame_stride, in_bin_stride, out_row_stride, out_frame_stride, out_bin_stride, frames,
                h->cfg.bins);
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (floats * sizeof(float) > h->scratch.cap) {
        HIP_TRY(hipStreamSynchronize(h->stream)); /* an earlier pass may still read the old block */
        const int rc = h->scratch.ensure(floats * sizeof(float));
        if (rc != ALACGPU_E_OK) return rc;
    }
    set_scratch(&p, (float*)h->scratch.p);
    const uint32_t lds_bytes = lds_floats_of(p.bins, p.tile_frames) * (uint32_t)sizeof(float);
    return h->run(sync, [&](hipStream_t s) {
        if (d_stats && p.stat == kNone) {
            const hipError_t e = hipMemsetAsync(d_stats, 0, rows * 2u * p.bins * sizeof(float), s);
            if (e != hipSuccess) return e;
        }
        return alack::featnorm_launch(s, p, lds_bytes);
    });
}

} /* extern "C" */
