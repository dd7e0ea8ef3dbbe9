/*
 * k_waveaug.hip — waveform augmentation with per-row lengths (gain, noise from a bank at an SNR, dither, clamp, padding): the
 * gfx950 kernels over csrc/alac_waveaug.h and the handle's entries (one translation unit of libalacgpu.so; nothing here touches
 * SpecAugment or any other kernel).
 *
 * One pass = these launches on the handle's stream:
 *   alac_waveaug_partials  one workgroup per (row, chunk of 4096 samples); a chunk at or behind n_r leaves at once. The chunk of x
 *                          into LDS, lane l's chain over the samples l mod 256, the tree over the lanes; where the row's draws say
 *                          applied, the wrapped noise segment the same way -> the chunk's partial Ex and En
 *   alac_waveaug_finish    one workgroup per row: the partials in chunk order -> Ex, En, a, b; the stats and the draws
 *   alac_waveaug_apply     one workgroup per (row, chunk): the noise segment into LDS where b != 0, then y = a x + b z (+ dither
 *                          in alac_waveaug_apply_dither, a kernel of its own, so that no sample pays a Philox block or a branch
 *                          for a dither of 0), clamp and padding, 16 bytes at a time
 * Without a bank and without stats the apply kernel runs alone. No atomic; everything is written with vector stores.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "alac_waveaug.h"
#include "alac_host.h"

using namespace alacwa;
using alack::set_err;

namespace {

__global__ void __launch_bounds__(kThreads) alac_waveaug_partials(Params p, uint64_t first_tile) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.chunks;
    if (row >= p.rows) return;
    const Chunk c = make_chunk(p, row, b - row * p.chunks);
    if (c.nv == 0u) return;
    const Lds l = carve(lds, kTile);
    const uint32_t tid = threadIdx.x;
    lines_in(c.x, 0u, 1u, c.nv, l.image, 0u, 1u, tid);
    row_words(p, c.id, l.words, tid);
    __syncthreads();
    l.lanes[tid] = lane_sum(l.image, c.nv, tid);
    const Draws d = resolve(p, l.words);
    __syncthreads();
    if (d.applied) stage_noise(p, c, d, l.image, tid);
    __syncthreads();
    l.lanes[kThreads + tid] = d.applied ? lane_sum(l.image, c.nv, tid) : 0.0f;
    for (uint32_t s = kThreads / 2u; s > 0u; s >>= 1) {
        __syncthreads();
        fold(l.lanes, s, tid);
    }
    put_partials(p, c, l.lanes, tid);
}

__global__ void __launch_bounds__(kThreads) alac_waveaug_finish(Params p, uint64_t first_tile) {
    __shared__ __attribute__((aligned(16))) float lds[kSideFloats];
    const uint64_t row = first_tile + blockIdx.x;
    if (row >= p.rows) return;
    const Lds l = carve(lds, 0u);
    const uint32_t tid = threadIdx.x;
    const uint64_t nc = chunks_of(p, row);
    finish_start(l.sums, tid);
    row_words(p, id_of(p, row), l.words, tid);
    for (uint64_t c0 = 0; c0 < nc; c0 += kThreads) {
        const uint32_t cnt = nc - c0 < kThreads ? (uint32_t)(nc - c0) : kThreads;
        finish_load(p, row, c0, cnt, l.lanes, tid);
        __syncthreads();
        finish_add(l.lanes, cnt, l.sums, tid);
        __syncthreads();
    }
    __syncthreads();
    finish_row(p, row, l, tid);
}

template <bool Dither>
__device__ __forceinline__ void apply_body(const Params& p, uint64_t first_tile, float* lds) {
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.chunks;
    if (row >= p.rows) return;
    const Chunk c = make_chunk(p, row, b - row * p.chunks);
    const Lds l = carve(lds, kTile);
    const uint32_t tid = threadIdx.x;
    row_words(p, c.id, l.words, tid);
    __syncthreads();
    const Draws d = resolve(p, l.words);
    const float a = gain_of(p, d);
    const float nb = p.reduce ? p.stats[row * kStats + 3u] : 0.0f;
    if (nb != 0.0f && c.nv) stage_noise(p, c, d, l.image, tid);
    if (!p.reduce && p.draws_out && c.t0 == 0u && tid == 0u) put_draws(p, row, d);
    __syncthreads();
    apply_chunk<Dither>(p, c, a, nb, l.image, tid);
}

__global__ void __launch_bounds__(kThreads) alac_waveaug_apply(Params p, uint64_t first_tile) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    apply_body<false>(p, first_tile, lds);
}

__global__ void __launch_bounds__(kThreads) alac_waveaug_apply_dither(Params p, uint64_t first_tile) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    apply_body<true>(p, first_tile, lds);
}

} /* namespace */

namespace alack {

hipError_t waveaug_launch(hipStream_t stream, const Params& p) {
    if (p.rows == 0 || p.T == 0) return hipSuccess;
    hipError_t err = hipSuccess;
    if (p.reduce) {
        err = launch_tiles(alac_waveaug_partials, p.rows * p.chunks, kThreads, 0, stream, p);
        if (err == hipSuccess) err = launch_tiles(alac_waveaug_finish, p.rows, kThreads, 0, stream, p);
    }
    if (err == hipSuccess)
        err = launch_tiles(p.dither != 0.0f ? alac_waveaug_apply_dither : alac_waveaug_apply, p.rows * p.chunks, kThreads, 0, stream, p);
    return err;
}

} /* namespace alack */

/* ---- host side (alac_host.h) ---------------------------------------------------------------------------------------- */
struct __attribute__((visibility("hidden"))) alacgpu_waveaug : alack::PassHandle { /* hidden: its destructor is no export */
    Config cfg{};
    std::vector<float> snr_amp, gain_amp;
    float* d_snr_amp = nullptr;
    float* d_gain_amp = nullptr;
    alack::DevBuf scratch; /* the partials and, where the caller keeps none, the stats: grows, never shrinks */
};

extern "C" {

int alacgpu_waveaug_create(int device, const alacgpu_waveaug_config* config, alacgpu_waveaug** out) {
    if (!out) return alack::null_argument();
    *out = nullptr;
    if (!config) return alack::null_argument();
    const Config c{config->snr_lo_q8, config->snr_hi_q8, config->gain_lo_q8, config->gain_hi_q8, config->noise_prob_q16,
                   config->dither,    config->clamp,     config->pad_value};
    if (!config_ok(c)) {
        set_err("no waveform augmentation plan: snr (%d, %d) or gain (%d, %d) outside [%d, %d] 1/256 dB, out of order or more than "
                "%d apart, noise_prob_q16 %u above %u, dither %g negative or not finite, or clamp %u above 1", c.snr_lo_q8, c.snr_hi_q8,
                c.gain_lo_q8, c.gain_hi_q8, -kMaxQ8, kMaxQ8, kMaxQ8, c.noise_prob_q16, kMaxProbQ16, (double)c.dither, c.clamp);
        return ALACGPU_E_ARG;
    }
    alacgpu_waveaug* h = new (std::nothrow) alacgpu_waveaug();
    if (!h) {
        set_err("out of memory");
        return ALACGPU_E_ARG;
    }
    h->cfg = c;
    h->snr_amp = snr_table(c);
    h->gain_amp = gain_table(c);
    h->open(device);
    h->upload(&h->d_snr_amp, h->snr_amp);
    h->upload(&h->d_gain_amp, h->gain_amp);
    if (h->err == hipSuccess) h->err = (hipError_t)(h->scratch.ensure(256) == ALACGPU_E_OK ? hipSuccess : hipErrorOutOfMemory);
    if (h->err != hipSuccess) {
        set_err("waveform augmentation handle creation failed: %s", hipGetErrorString(h->err));
        alacgpu_waveaug_destroy(h);
        return ALACGPU_E_HIP;
    }
    *out = h;
    return ALACGPU_E_OK;
}

void alacgpu_waveaug_destroy(alacgpu_waveaug* h) {
    if (!h) return;
    h->close();
    h->scratch.release();
    delete h;
}

void* alacgpu_waveaug_stream(alacgpu_waveaug* h) { return h ? (void*)h->stream : nullptr; }

int alacgpu_waveaug_synchronize(alacgpu_waveaug* h) { return h ? h->synchronize() : ALACGPU_E_ARG; }

int alacgpu_waveaug_last_ms(alacgpu_waveaug* h, float* ms) { return h ? h->last_ms(ms, "waveform augmentation") : alack::null_argument(); }

int alacgpu_waveaug_plan(const alacgpu_waveaug* h, alacgpu_waveaug_info* info, float* snr_out, size_t snr_cap, float* gain_out,
                         size_t gain_cap) {
    if (!h || !info) return alack::null_argument();
    if ((snr_out && snr_cap < h->snr_amp.size()) || (gain_out && gain_cap < h->gain_amp.size())) {
        set_err("capacity below the plan's %zu snr / %zu gain entries", h->snr_amp.size(), h->gain_amp.size());
        return ALACGPU_E_ARG;
    }
    info->snr_lo_q8 = h->cfg.snr_lo_q8;
    info->snr_hi_q8 = h->cfg.snr_hi_q8;
    info->gain_lo_q8 = h->cfg.gain_lo_q8;
    info->gain_hi_q8 = h->cfg.gain_hi_q8;
    info->noise_prob_q16 = h->cfg.noise_prob_q16;
    info->clamp = h->cfg.clamp;
    info->tile = kTile;
    info->draws = kDraws;
    info->snr_entries = (uint32_t)h->snr_amp.size();
    info->gain_entries = (uint32_t)h->gain_amp.size();
    info->lds_bytes = kLdsFloats * (uint32_t)sizeof(float);
    info->dither = h->cfg.dither;
    info->pad_value = h->cfg.pad_value;
    info->reserved = 0;
    info->scratch_bytes = h->scratch.cap;
    info->scratch_address = (uint64_t)(uintptr_t)h->scratch.p;
    if (snr_out) memcpy(snr_out, h->snr_amp.data(), h->snr_amp.size() * sizeof(float));
    if (gain_out) memcpy(gain_out, h->gain_amp.data(), h->gain_amp.size() * sizeof(float));
    return ALACGPU_E_OK;
}

int alacgpu_waveaug_device(alacgpu_waveaug* h, const float* d_in, size_t in_row_stride, size_t rows, size_t samples,
                           const int32_t* d_lengths, const float* d_noise, size_t noise_row_stride, size_t noise_rows,
                           size_t noise_samples, const int32_t* d_noise_lengths, uint64_t seed, uint64_t row_base, const int64_t* d_ids,
                           float* d_out, size_t out_row_stride, int32_t* d_draws, float* d_stats, int sync) {
    if (!h) return alack::null_argument();
    if (rows == 0 || samples == 0) return ALACGPU_E_OK;
    uint64_t floats = 0;
    Params p;
    if (!make_params(h->cfg, h->d_snr_amp, h->d_gain_amp, d_in, in_row_stride, rows, samples, d_lengths, d_noise, noise_row_stride,
                     noise_rows, noise_samples, d_noise_lengths, seed, row_base, d_ids, d_out, out_row_stride, d_draws, d_stats, &p) ||
        !scratch_floats_of(rows, samples, p.reduce != 0u, d_stats == nullptr, &floats)) {
        set_err("augment_waveform: a NULL or misaligned buffer, a row stride (%zu in, %zu out, %zu noise) below the row's %zu / %zu "
                "samples, an output that overlaps the input (in place takes the input's own base and stride) or the noise bank, "
                "more than 2^31 - 1 samples or noise clips, or sizes that overflow", in_row_stride, out_row_stride, noise_row_stride,
                samples, noise_samples);
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipSetDevice(h->device));
    if (floats * sizeof(float) > h->scratch.cap) {
        HIP_TRY(hipStreamSynchronize(h->stream)); /* an earlier pass may still read the old block */
        const int rc = h->scratch.ensure(floats * sizeof(float));
        if (rc != ALACGPU_E_OK) return rc;
    }
    set_scratch(&p, (float*)h->scratch.p);
    return h->run(sync, [&](hipStream_t s) { return alack::waveaug_launch(s, p); });
}

} /* extern "C" */
