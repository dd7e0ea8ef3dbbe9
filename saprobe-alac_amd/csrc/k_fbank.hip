/*
 * k_fbank.hip — float32 rows -> Kaldi's fbank or MFCC features: the gfx950 kernel over csrc/alac_fbank.h (which stands on
 * csrc/alac_mel.h) and the fbank handle's entries (one translation unit of libalacgpu.so; nothing here touches the other
 * kernels).
 *
 * One pass = launches of one kernel on the handle's stream:
 *   alac_fbank_rows  one workgroup per tile (tile_frames consecutive frames of one row): the tile's inputs with 16-byte loads
 *                    into LDS, Kaldi's reflection resolved there; the frames' energies out of that image; every lane the fmaf
 *                    chains of blocks of 8 frames x 2 bins against the folded basis (mean removal, pre-emphasis, window and
 *                    scale live in the table); the powers into an LDS tile, the mel chains and the log out of it; for MFCC the
 *                    DCT and lifter out of the log-mel tile; the results through LDS into 16-byte stores
 * No matrix instruction, no atomic; everything is written with vector stores.
 * A handle made with ALACGPU_FBANK_TRANSFORM_FFT runs alac_fbankfft_rows (k_fbankfft.hip over alac_fbankfft.h) in its place: it
 * owns the window, twiddle and position tables and no basis.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "alac_fbank.h"
#include "alac_fbankfft.h"
#include "alac_host.h"

using namespace alacfb;
using alack::set_err;

namespace {

__global__ void __launch_bounds__(kThreads) alac_fbank_rows(Params p, uint64_t first_tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[]; /* the plan's lds_floats */
    const uint64_t b = first_tile + blockIdx.x;
    const uint64_t row = b / p.m.tiles_per_row;
    if (row >= p.m.rows) return;
    const Tile t = make_tile(p, row, b - row * p.m.tiles_per_row);
    if (t.count == 0) return;
    tile_phase(p, t, lds, 0u, threadIdx.x); /* stage */
    __syncthreads();
    tile_phase(p, t, lds, 1u, threadIdx.x); /* energies, DFT */
    __syncthreads();
    tile_phase(p, t, lds, 2u, threadIdx.x); /* mel, log */
    __syncthreads();
    if (p.num_ceps) {
        tile_phase(p, t, lds, 3u, threadIdx.x); /* DCT, lifter */
        __syncthreads();
    }
    tile_phase(p, t, lds, 4u, threadIdx.x); /* store */
}

} /* namespace */

namespace alack {

hipError_t fbank_launch(hipStream_t stream, const Params& p, uint32_t lds_bytes) {
    if (p.m.rows == 0 || p.m.out_frames == 0) return hipSuccess;
    return launch_tiles(alac_fbank_rows, p.m.rows * p.m.tiles_per_row, kThreads, lds_bytes, stream, p);
}

} /* namespace alack */

/* ---- host side (alac_host.h) ---------------------------------------------------------------------------------------- */
struct __attribute__((visibility("hidden"))) alacgpu_fbank : alack::PassHandle { /* hidden: its destructor is no export */
    Plan plan;
    uint32_t transform = ALACGPU_FBANK_TRANSFORM_DIRECT;
    alacfbfft::Plan fft; /* transform = fft: the plan in use; `plan` then is its base */
    float* d_ws = nullptr;
    float* d_tw = nullptr;
    uint32_t* d_pos = nullptr;
    float* d_bt = nullptr;
    float* d_fbw = nullptr;
    int32_t* d_first = nullptr;
    float* d_dct = nullptr;
    float* d_lifter = nullptr;
};

namespace {
Config config_of(const alacgpu_fbank_config* c) {
    Config k;
    k.sample_rate = c->sample_rate;
    k.frame_length = c->frame_length;
    k.frame_shift = c->frame_shift;
    k.round_to_power_of_two = c->round_to_power_of_two;
    k.num_mel_bins = c->num_mel_bins;
    k.num_ceps = c->num_ceps;
    k.snip_edges = c->snip_edges;
    k.remove_dc_offset = c->remove_dc_offset;
    k.window_type = c->window_type;
    k.use_log_fbank = c->use_log_fbank;
    k.use_energy = c->use_energy;
    k.raw_energy = c->raw_energy;
    k.htk_compat = c->htk_compat;
    k.use_power = c->use_power;
    k.log_energy = c->log_energy;
    k.layout = c->layout;
    k.preemphasis = c->preemphasis_coefficient;
    k.blackman_coeff = c->blackman_coeff;
    k.low_freq = c->low_freq;
    k.high_freq = c->high_freq;
    k.energy_floor = c->energy_floor;
    k.scale = c->scale;
    k.cepstral_lifter = c->cepstral_lifter;
    k.dither = c->dither;
    k.vtln_warp = c->vtln_warp;
    return k;
}
} /* namespace */

extern "C" {

int alacgpu_fbank_create(int device, const alacgpu_fbank_config* config, alacgpu_fbank** out) {
    return alacgpu_fbank_create_transform(device, config, ALACGPU_FBANK_TRANSFORM_DIRECT, out);
}

int alacgpu_fbank_create_transform(int device, const alacgpu_fbank_config* config, uint32_t transform, alacgpu_fbank** out) {
    if (!out || !config) {
        if (out) *out = nullptr;
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    *out = nullptr;
    alacgpu_fbank* r = new (std::nothrow) alacgpu_fbank();
    if (!r) {
        set_err("out of memory");
        return ALACGPU_E_ARG;
    }
    if (transform > ALACGPU_FBANK_TRANSFORM_FFT) {
        set_err("transform %u is neither ALACGPU_FBANK_TRANSFORM_DIRECT (0) nor ALACGPU_FBANK_TRANSFORM_FFT (1)", transform);
        delete r;
        return ALACGPU_E_ARG;
    }
    r->transform = transform;
    const Config cfg = config_of(config);
    const uint32_t n_fft = alacfbfft::n_fft_of(cfg);
    if (transform == ALACGPU_FBANK_TRANSFORM_FFT && n_fft && !alacmelfft::size_ok(n_fft)) {
        set_err("no FFT plan for frame_length %u (DFT size %u): with transform = fft the DFT size (the next power of two >= "
                "frame_length with round_to_power_of_two, else frame_length) is even, in [2, %u], and its half is 2^a 3^b 5^c (the "
                "direct transform takes every frame_length in [1, %u])", config->frame_length, n_fft, kMaxFft, kMaxFft);
        delete r;
        return ALACGPU_E_ARG;
    }
    bool planned;
    if (transform == ALACGPU_FBANK_TRANSFORM_FFT) {
        planned = alacfbfft::make_plan(cfg, &r->fft);
        if (planned) r->plan = r->fft.base;
    } else {
        planned = make_plan(cfg, &r->plan);
    }
    if (!planned) {
        set_err("no Kaldi feature plan for frame_length %u, frame_shift %u at %u Hz, %u mel bins in [%g, %g] Hz, %u ceps: "
                "frame_length in [1, %u], frame_shift >= 1, flags 0 or 1, window_type 0..4, layout 0..1, dither 0 (was %g), "
                "vtln_warp 1 (was %g), use_power 1 (was %u), use_energy only with raw_energy, 1 <= num_mel_bins <= %u, num_ceps <= "
                "num_mel_bins, finite numbers, scale not 0, energy_floor >= 0, 0 <= low_freq < Nyquist, 0 < high <= Nyquist, low < "
                "high, every filter one run of weights, and four frames within %u bytes of LDS",
                config->frame_length, config->frame_shift, config->sample_rate, config->num_mel_bins, config->low_freq,
                config->high_freq, config->num_ceps, kMaxFft, config->dither, config->vtln_warp, config->use_power, kMaxMels,
                kLdsFloats * 4u);
        delete r;
        return ALACGPU_E_ARG;
    }
    r->open(device);
    r->upload(&r->d_bt, r->plan.bt); /* transform = fft: no basis, one element that nothing reads */
    r->upload(&r->d_fbw, r->plan.fbw);
    r->upload(&r->d_first, r->plan.first);
    r->upload(&r->d_dct, r->plan.dct);
    r->upload(&r->d_lifter, r->plan.lifter);
    if (transform == ALACGPU_FBANK_TRANSFORM_FFT) {
        r->upload(&r->d_ws, r->fft.ws);
        r->upload(&r->d_tw, r->fft.fft.tw);
        r->upload(&r->d_pos, r->fft.fft.pos);
    }
    if (r->err != hipSuccess) {
        set_err("Kaldi feature handle creation failed: %s", hipGetErrorString(r->err));
        alacgpu_fbank_destroy(r);
        return ALACGPU_E_HIP;
    }
    *out = r;
    return ALACGPU_E_OK;
}

void alacgpu_fbank_destroy(alacgpu_fbank* r) {
    if (!r) return;
    r->close();
    delete r;
}

void* alacgpu_fbank_stream(alacgpu_fbank* r) { return r ? (void*)r->stream : nullptr; }

int alacgpu_fbank_synchronize(alacgpu_fbank* r) { return r ? r->synchronize() : ALACGPU_E_ARG; }

int alacgpu_fbank_last_ms(alacgpu_fbank* r, float* ms) { return r ? r->last_ms(ms, "feature") : alack::null_argument(); }

uint64_t alacgpu_fbank_out_frames(const alacgpu_fbank* r, uint64_t in_frames) {
    if (!r || in_frames > ((uint64_t)1 << 61)) return 0;
    return out_frames_of(r->plan.W, r->plan.hop, r->plan.cfg.snip_edges, in_frames);
}

int alacgpu_fbank_plan(const alacgpu_fbank* r, alacgpu_fbank_info* info, float* basis_out, size_t basis_cap, float* fb_out,
                       size_t fb_cap, int32_t* first_out, size_t first_cap, float* dct_out, size_t dct_cap, float* lifter_out,
                       size_t lifter_cap) {
    if (!r || !info) return alack::null_argument();
    const Plan& pl = r->plan;
    if ((basis_out && basis_cap < pl.basis.size()) || (fb_out && fb_cap < pl.fbw.size()) || (first_out && first_cap < pl.first.size()) ||
        (dct_out && dct_cap < pl.dct.size()) || (lifter_out && lifter_cap < pl.lifter.size())) {
        set_err("capacity below the plan's %zu basis / %zu filterbank / %zu first / %zu DCT / %zu lifter entries", pl.basis.size(),
                pl.fbw.size(), pl.first.size(), pl.dct.size(), pl.lifter.size());
        return ALACGPU_E_ARG;
    }
    info->frame_length = pl.W;
    info->frame_shift = pl.hop;
    info->n_fft = pl.N;
    info->n_freqs = pl.K;
    info->num_mel_bins = pl.n_mels;
    info->taps = pl.taps;
    info->num_ceps = pl.num_ceps;
    info->cols = pl.cols;
    info->tile_frames = pl.tile_frames;
    info->lds_bytes = pl.lds_floats * 4u;
    if (basis_out && !pl.basis.empty()) memcpy(basis_out, pl.basis.data(), pl.basis.size() * sizeof(float));
    if (fb_out) memcpy(fb_out, pl.fbw.data(), pl.fbw.size() * sizeof(float));
    if (first_out) memcpy(first_out, pl.first.data(), pl.first.size() * sizeof(int32_t));
    if (dct_out && !pl.dct.empty()) memcpy(dct_out, pl.dct.data(), pl.dct.size() * sizeof(float));
    if (lifter_out && !pl.lifter.empty()) memcpy(lifter_out, pl.lifter.data(), pl.lifter.size() * sizeof(float));
    return ALACGPU_E_OK;
}

int alacgpu_fbank_fft_plan(const alacgpu_fbank* r, alacgpu_fbank_fft_info* info, float* window_out, size_t window_cap,
                           float* twiddle_out, size_t twiddle_cap) {
    if (!r || !info) return alack::null_argument();
    const alacfbfft::Plan& fp = r->fft;
    if ((window_out && window_cap < fp.ws.size()) || (twiddle_out && twiddle_cap < fp.fft.tw.size())) {
        set_err("capacity below the plan's %zu window entries / %zu twiddle entries", fp.ws.size(), fp.fft.tw.size());
        return ALACGPU_E_ARG;
    }
    memset(info, 0, sizeof(*info));
    info->transform = r->transform;
    info->tile_frames = r->plan.tile_frames;
    info->lds_bytes = r->plan.lds_floats * 4u;
    if (r->transform == ALACGPU_FBANK_TRANSFORM_FFT) {
        info->batch_frames = fp.batch;
        info->pitch = fp.fft.pitch;
        info->n_passes = fp.fft.n_pass;
        for (uint32_t s = 0; s < fp.fft.n_pass; s++) info->radix[s] = fp.fft.radix[s];
        info->window_entries = (uint32_t)fp.ws.size();
        info->twiddle_entries = (uint32_t)fp.fft.tw.size();
        if (window_out) memcpy(window_out, fp.ws.data(), fp.ws.size() * sizeof(float));
        if (twiddle_out) memcpy(twiddle_out, fp.fft.tw.data(), fp.fft.tw.size() * sizeof(float));
    }
    return ALACGPU_E_OK;
}

int alacgpu_fbank_device(alacgpu_fbank* r, const float* d_in, size_t in_row_stride, size_t rows, size_t in_frames, float* d_out,
                         size_t out_row_stride, size_t out_inner_stride, int sync) {
    if (!r) return alack::null_argument();
    if (rows == 0 || alacgpu_fbank_out_frames(r, in_frames) == 0) {
        if (rows && in_frames > ((uint64_t)1 << 61)) {
            set_err("Kaldi features: %zu samples are more than one pass takes", in_frames);
            return ALACGPU_E_ARG;
        }
        return ALACGPU_E_OK;
    }
    const bool fft = r->transform == ALACGPU_FBANK_TRANSFORM_FFT;
    Params p;
    alacfbfft::Params q;
    if (fft ? !alacfbfft::make_params(r->fft, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, out_inner_stride, r->d_ws,
                                      r->d_tw, r->d_pos, r->d_fbw, r->d_first, r->d_dct, r->d_lifter, &q)
            : !make_params(r->plan, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, out_inner_stride, r->d_bt, r->d_fbw,
                           r->d_first, r->d_dct, r->d_lifter, &p)) {
        set_err("Kaldi features: a NULL or misaligned buffer, a stride (%zu in, %zu out rows, %zu out %s) below what it spans (%zu "
                "samples, %llu frames of %u columns), or sizes that overflow", in_row_stride, out_row_stride, out_inner_stride,
                r->plan.cfg.layout == kLayoutBins ? "bins" : "frames", in_frames,
                (unsigned long long)alacgpu_fbank_out_frames(r, in_frames), r->plan.cols);
        return ALACGPU_E_ARG;
    }
    const uint32_t lds_bytes = r->plan.lds_floats * 4u;
    return r->run(sync, [&](hipStream_t s) { return fft ? alack::fbankfft_launch(s, q, lds_bytes) : alack::fbank_launch(s, p, lds_bytes); });
}

} /* extern "C" */
