/*
 * k_mel.hip — float32 rows -> power or (log-)mel spectrograms: the gfx950 kernel over csrc/alac_mel.h and the mel handle's
 * entries (one translation unit of libalacgpu.so; nothing here touches the decode, waveform, clip, resample or encode kernels).
 *
 * One pass = launches of one kernel on the handle's stream:
 *   alac_mel_rows  one workgroup per tile (tile_frames consecutive frames of one row): the tile's inputs with 16-byte loads
 *                  into LDS, reflection and zeros resolved there; every lane the fmaf chains of blocks of 8 frames x 2 bins,
 *                  frames from LDS, the windowed basis from global memory ([n][bin pair]: a wave reads consecutive 16 bytes);
 *                  the powers into an LDS tile, the mel chains and the log out of it; the results through LDS into 16-byte
 *                  stores along time
 * No matrix instruction, no atomic; everything is written with vector stores.
 * A handle made with transform = ALACGPU_MEL_TRANSFORM_FFT runs alac_melfft_rows (k_melfft.hip over alac_melfft.h) in its place:
 * it owns the window, twiddle and position tables and no basis.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "alac_host.h"
#include "alac_mel.h"
#include "alac_melfft.h"

using namespace alacmel;
using alack::set_err;

namespace {

__global__ void __launch_bounds__(kThreads) alac_mel_rows(Params p, uint64_t first_tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[]; /* the plan's lds_floats */
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.tiles_per_row;
    if (row >= p.rows) return;
    const Tile t = make_tile(p, row, b - row * p.tiles_per_row);
    if (t.count == 0) return;
    float* ptile = lds + p.a_floats;
    stage_tile(p, t, lds, threadIdx.x);
    __syncthreads();
    dft_tile(p, t, lds, ptile, threadIdx.x);
    __syncthreads();
    if (p.n_mels) mel_tile(p, ptile, lds, threadIdx.x); /* the output tile takes the staged inputs' place */
    else log_tile(p, ptile, threadIdx.x);
    __syncthreads();
    if (p.n_mels) store_tile(p, t, lds, p.tile_frames, 1u, threadIdx.x);
    else store_tile(p, t, ptile, 1u, p.KP, threadIdx.x);
}

} /* namespace */

namespace alack {

hipError_t mel_launch(hipStream_t stream, const Params& p, uint32_t lds_bytes) {
    if (p.rows == 0 || p.out_frames == 0) return hipSuccess;
    return launch_tiles(alac_mel_rows, p.rows * p.tiles_per_row, kThreads, lds_bytes, stream, p);
}

} /* namespace alack */

/* ---- host side (alac_host.h) ---------------------------------------------------------------------------------------- */
struct __attribute__((visibility("hidden"))) alacgpu_mel : alack::PassHandle { /* hidden: its destructor is no export */
    Plan plan;
    uint32_t transform = ALACGPU_MEL_TRANSFORM_DIRECT;
    alacmelfft::Plan fft; /* transform = fft: the plan in use; `plan` then is its base */
    float* d_w32 = nullptr;
    float* d_tw = nullptr;
    uint32_t* d_pos = nullptr;
    float* d_bt = nullptr;
    float* d_fbw = nullptr;
    int32_t* d_first = nullptr;
};

namespace {
Config config_of(const alacgpu_mel_config* c) {
    Config k;
    k.sample_rate = c->sample_rate;
    k.n_fft = c->n_fft;
    k.win_length = c->win_length;
    k.hop_length = c->hop_length;
    k.f_min = c->f_min;
    k.f_max = c->f_max;
    k.n_mels = c->n_mels;
    k.center = c->center;
    k.norm = c->norm;
    k.mel_scale = c->mel_scale;
    k.log = c->log;
    k.floor = c->floor;
    return k;
}
} /* namespace */

extern "C" {

int alacgpu_mel_create(int device, const alacgpu_mel_config* config, alacgpu_mel** out) {
    if (!out || !config) {
        if (out) *out = nullptr;
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    *out = nullptr;
    alacgpu_mel* r = new (std::nothrow) alacgpu_mel();
    if (!r) {
        set_err("out of memory");
        return ALACGPU_E_ARG;
    }
    if (config->transform > ALACGPU_MEL_TRANSFORM_FFT) {
        set_err("transform %u is neither ALACGPU_MEL_TRANSFORM_DIRECT (0) nor ALACGPU_MEL_TRANSFORM_FFT (1)", config->transform);
        delete r;
        return ALACGPU_E_ARG;
    }
    r->transform = config->transform;
    if (r->transform == ALACGPU_MEL_TRANSFORM_FFT && !alacmelfft::size_ok(config->n_fft)) {
        set_err("no FFT plan for n_fft %u: with transform = fft n_fft is even, in [2, %u], and n_fft / 2 = 2^a 3^b 5^c (the direct "
                "transform takes every n_fft in that range)", config->n_fft, kMaxFft);
        delete r;
        return ALACGPU_E_ARG;
    }
    bool planned;
    if (r->transform == ALACGPU_MEL_TRANSFORM_FFT) {
        planned = alacmelfft::make_plan(config_of(config), &r->fft);
        if (planned) r->plan = r->fft.base;
    } else {
        planned = make_plan(config_of(config), &r->plan);
    }
    if (!planned) {
        set_err("no spectrogram plan for n_fft %u, win_length %u, hop_length %u at %u Hz, %u mels in [%g, %g) Hz, floor %g: n_fft "
                "in [2, %u], 1 <= win_length <= n_fft, hop_length >= 1, center and norm 0 or 1, mel_scale 0..2, log 0..3, floor a "
                "positive float32; with a mel scale 1 <= n_mels <= %u and 0 <= f_min < f_max, without one n_mels and norm 0; and "
                "four frames within %u bytes of LDS",
                config->n_fft, config->win_length, config->hop_length, config->sample_rate, config->n_mels, config->f_min,
                config->f_max, config->floor, kMaxFft, kMaxMels, kLdsFloats * 4u);
        delete r;
        return ALACGPU_E_ARG;
    }
    r->open(device);
    r->upload(&r->d_bt, r->plan.bt); /* transform = fft: no basis, one element that nothing reads */
    r->upload(&r->d_fbw, r->plan.fbw);
    r->upload(&r->d_first, r->plan.first);
    if (r->transform == ALACGPU_MEL_TRANSFORM_FFT) {
        r->upload(&r->d_w32, r->fft.w32);
        r->upload(&r->d_tw, r->fft.tw);
        r->upload(&r->d_pos, r->fft.pos);
    }
    if (r->err != hipSuccess) {
        set_err("spectrogram handle creation failed: %s", hipGetErrorString(r->err));
        alacgpu_mel_destroy(r);
        return ALACGPU_E_HIP;
    }
    *out = r;
    return ALACGPU_E_OK;
}

void alacgpu_mel_destroy(alacgpu_mel* r) {
    if (!r) return;
    r->close();
    delete r;
}

void* alacgpu_mel_stream(alacgpu_mel* r) { return r ? (void*)r->stream : nullptr; }

int alacgpu_mel_synchronize(alacgpu_mel* r) { return r ? r->synchronize() : ALACGPU_E_ARG; }

int alacgpu_mel_last_ms(alacgpu_mel* r, float* ms) { return r ? r->last_ms(ms, "spectrogram") : alack::null_argument(); }

uint64_t alacgpu_mel_out_frames(const alacgpu_mel* r, uint64_t in_frames) {
    if (!r || in_frames > ((uint64_t)1 << 61)) return 0;
    return out_frames_of(r->plan.N, r->plan.hop, r->plan.cfg.center, in_frames);
}

int alacgpu_mel_plan(const alacgpu_mel* r, alacgpu_mel_info* info, float* basis_out, size_t basis_cap, float* fb_out,
                     size_t fb_cap, int32_t* first_out, size_t first_cap) {
    if (!r || !info) return alack::null_argument();
    const Plan& pl = r->plan;
    if ((basis_out && basis_cap < pl.basis.size()) || (fb_out && fb_cap < pl.fbw.size()) || (first_out && first_cap < pl.first.size())) {
        set_err("capacity below the plan's %zu basis entries / %zu filterbank entries / %zu filters", pl.basis.size(), pl.fbw.size(),
                pl.first.size());
        return ALACGPU_E_ARG;
    }
    info->n_fft = pl.N;
    info->win_length = pl.W;
    info->hop_length = pl.hop;
    info->n_freqs = pl.K;
    info->n_mels = pl.n_mels;
    info->taps = pl.n_mels ? pl.taps : 0u;
    info->bins = pl.bins;
    info->tile_frames = pl.tile_frames;
    info->lds_bytes = pl.lds_floats * 4u;
    if (basis_out) memcpy(basis_out, pl.basis.data(), pl.basis.size() * sizeof(float));
    if (fb_out && !pl.fbw.empty()) memcpy(fb_out, pl.fbw.data(), pl.fbw.size() * sizeof(float));
    if (first_out && !pl.first.empty()) memcpy(first_out, pl.first.data(), pl.first.size() * sizeof(int32_t));
    return ALACGPU_E_OK;
}

int alacgpu_mel_fft_plan(const alacgpu_mel* r, alacgpu_mel_fft_info* info, float* window_out, size_t window_cap, float* twiddle_out,
                         size_t twiddle_cap) {
    if (!r || !info) return alack::null_argument();
    const alacmelfft::Plan& fp = r->fft;
    if ((window_out && window_cap < fp.w32.size()) || (twiddle_out && twiddle_cap < fp.tw.size())) {
        set_err("capacity below the plan's %zu window entries / %zu twiddle entries", fp.w32.size(), fp.tw.size());
        return ALACGPU_E_ARG;
    }
    memset(info, 0, sizeof(*info));
    info->transform = r->transform;
    info->tile_frames = r->plan.tile_frames;
    info->lds_bytes = r->plan.lds_floats * 4u;
    if (r->transform == ALACGPU_MEL_TRANSFORM_FFT) {
        info->batch_frames = fp.batch;
        info->pitch = fp.pitch;
        info->n_passes = fp.n_pass;
        for (uint32_t s = 0; s < fp.n_pass; s++) info->radix[s] = fp.radix[s];
        info->window_entries = (uint32_t)fp.w32.size();
        info->twiddle_entries = (uint32_t)fp.tw.size();
        if (window_out) memcpy(window_out, fp.w32.data(), fp.w32.size() * sizeof(float));
        if (twiddle_out) memcpy(twiddle_out, fp.tw.data(), fp.tw.size() * sizeof(float));
    }
    return ALACGPU_E_OK;
}

int alacgpu_mel_device(alacgpu_mel* r, const float* d_in, size_t in_row_stride, size_t rows, size_t in_frames, float* d_out,
                       size_t out_row_stride, size_t out_bin_stride, int sync) {
    if (!r) return alack::null_argument();
    if (rows == 0 || alacgpu_mel_out_frames(r, in_frames) == 0) {
        if (rows && in_frames > ((uint64_t)1 << 61)) {
            set_err("spectrogram: %zu frames are more than one pass takes", in_frames);
            return ALACGPU_E_ARG;
        }
        return ALACGPU_E_OK;
    }
    const bool fft = r->transform == ALACGPU_MEL_TRANSFORM_FFT;
    Params p;
    alacmelfft::Params q;
    if (fft ? !alacmelfft::make_params(r->fft, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, out_bin_stride, r->d_w32,
                                       r->d_tw, r->d_pos, r->d_fbw, r->d_first, &q)
            : !make_params(r->plan, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, out_bin_stride, r->d_bt, r->d_fbw,
                           r->d_first, &p)) {
        set_err("spectrogram: a NULL or misaligned buffer, a stride (%zu in, %zu out rows, %zu out bins) below what it spans (%zu "
                "samples, %u bins of %llu frames), or sizes that overflow", in_row_stride, out_row_stride, out_bin_stride, in_frames,
                r->plan.bins, (unsigned long long)alacgpu_mel_out_frames(r, in_frames));
        return ALACGPU_E_ARG;
    }
    const uint32_t lds_bytes = r->plan.lds_floats * 4u;
    return r->run(sync, [&](hipStream_t s) { return fft ? alack::melfft_launch(s, q, lds_bytes) : alack::mel_launch(s, p, lds_bytes); });
}

} /* extern "C" */
