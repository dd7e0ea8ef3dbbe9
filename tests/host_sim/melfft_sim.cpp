/*
 * melfft_sim.cpp — TEST-ONLY host build of the spectrogram pass with transform = fft.
 *
 * Compiles saprobe-alac_amd/csrc/alac_melfft.h (the text the gfx950 kernel of k_melfft.hip is built from) with g++, contraction
 * off, and runs it the way k_melfft.hip launches it: for every tile of every row the staging phase for work items 0..255, the
 * barrier, then per batch of frames the pack, every pass and the split step, each for work items 0..255 with a barrier behind
 * it, the mel chains (or the log over the power tile), the barrier, and the store phase. The CPU suite (-m "not gpu") checks it
 * against a numpy restatement, and the GPU suite holds the kernel to it bit for bit. It lives under tests/ and is never linked
 * into libalacgpu.so. tests/host_sim/melfft_san_main.cpp calls the same functions from a program of its own.
 */
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../saprobe-alac_amd/csrc/alac_melfft.h"

using namespace alacmelfft;

namespace {
/* cfg = {sample_rate, n_fft, win_length, hop_length, n_mels, center, norm, mel_scale, log}; dbl = {f_min, f_max, floor} */
alacmel::Config config_of(const uint32_t* cfg, const double* dbl) {
    alacmel::Config c;
    c.sample_rate = cfg[0];
    c.n_fft = cfg[1];
    c.win_length = cfg[2];
    c.hop_length = cfg[3];
    c.n_mels = cfg[4];
    c.center = cfg[5];
    c.norm = cfg[6];
    c.mel_scale = cfg[7];
    c.log = cfg[8];
    c.f_min = dbl[0];
    c.f_max = dbl[1];
    c.floor = dbl[2];
    return c;
}
}  // namespace

extern "C" {

/* alacgpu_mel_create with transform = fft + alacgpu_mel_fft_plan (+ what alacgpu_mel_plan adds): info = {transform,
 * tile_frames, lds_bytes, batch_frames, pitch, n_passes, radix[8], window_entries, twiddle_entries, n_mels, taps}; the table
 * pointers may be NULL. -> 0, or -2 where the entries return ALACGPU_E_ARG. */
int melfft_sim_plan(const uint32_t* cfg, const double* dbl, uint32_t* info, float* window_out, uint64_t window_cap, float* tw_out,
                    uint64_t tw_cap, float* fb_out, uint64_t fb_cap, int32_t* first_out, uint64_t first_cap) {
    Plan pl;
    if (!cfg || !dbl || !info || !make_plan(config_of(cfg, dbl), &pl)) return -2;
    if ((window_out && window_cap < pl.w32.size()) || (tw_out && tw_cap < pl.tw.size()) || (fb_out && fb_cap < pl.base.fbw.size()) ||
        (first_out && first_cap < pl.base.first.size()))
        return -2;
    uint32_t numbers[18] = {kFft, pl.base.tile_frames, pl.base.lds_floats * 4u, pl.batch, pl.pitch, pl.n_pass};
    for (uint32_t s = 0; s < pl.n_pass; s++) numbers[6 + s] = pl.radix[s];
    numbers[14] = (uint32_t)pl.w32.size();
    numbers[15] = (uint32_t)pl.tw.size();
    numbers[16] = pl.base.n_mels;
    numbers[17] = pl.base.n_mels ? pl.base.taps : 0u;
    memcpy(info, numbers, sizeof(numbers));
    if (!pl.base.basis.empty() || !pl.base.bt.empty()) return -4; /* an FFT plan builds no basis */
    if (window_out) memcpy(window_out, pl.w32.data(), pl.w32.size() * sizeof(float));
    if (tw_out) memcpy(tw_out, pl.tw.data(), pl.tw.size() * sizeof(float));
    if (fb_out && !pl.base.fbw.empty()) memcpy(fb_out, pl.base.fbw.data(), pl.base.fbw.size() * sizeof(float));
    if (first_out && !pl.base.first.empty()) memcpy(first_out, pl.base.first.data(), pl.base.first.size() * sizeof(int32_t));
    return 0;
}

/* The arguments of alacgpu_mel_device with host pointers. -> 0, or -2 for what the entries reject. guard != 0: the input,
 * (rows - 1) * in_stride + in_frames elements, is copied so that it ENDS at an inaccessible page, and the pass reads the copy:
 * a read behind the last row's samples is fatal. */
int melfft_sim_run(const uint32_t* cfg, const double* dbl, const float* in, uint64_t in_stride, uint64_t rows, uint64_t in_frames,
                   float* out, uint64_t out_row_stride, uint64_t out_bin_stride, int guard) {
    Plan pl;
    if (!make_plan(config_of(cfg, dbl), &pl)) return -2;
    if (in_frames > ((uint64_t)1 << 61)) return rows ? -2 : 0;
    if (rows == 0 || alacmel::out_frames_of(pl.base.N, pl.base.hop, pl.base.cfg.center, in_frames) == 0) return 0;
    Params p;
    if (!make_params(pl, in, in_stride, rows, in_frames, out, out_row_stride, out_bin_stride, pl.w32.data(), pl.tw.data(), pl.pos.data(),
                     pl.base.fbw.data(), pl.base.first.data(), &p))
        return -2;

    uint8_t* region = nullptr;
    size_t region_len = 0;
    if (guard) {
        const size_t bytes = (size_t)((rows - 1) * in_stride + in_frames) * sizeof(float);
        const size_t page = (size_t)sysconf(_SC_PAGESIZE);
        region_len = (bytes + page - 1) / page * page + page;
        region = (uint8_t*)mmap(nullptr, region_len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (region == MAP_FAILED) return -3;
        uint8_t* copy = region + region_len - page - bytes;
        memcpy(copy, in, bytes);
        mprotect(region + region_len - page, page, PROT_NONE);
        p.m.in = (const float*)copy;
    }
    /* exactly the plan's LDS, on the heap: an index past it is the sanitizer's to see */
    float* lds = nullptr;
    if (posix_memalign((void**)&lds, 16, (size_t)pl.base.lds_floats * sizeof(float))) return -3;
    float* ptile = lds + p.m.a_floats;
    F2* buf = (F2*)(ptile + p.p_floats);
    for (uint64_t row = 0; row < rows; row++)
        for (uint64_t tile = 0; tile < p.m.tiles_per_row; tile++) {
            const Tile t = alacmel::make_tile(p.m, row, tile);
            if (t.count == 0) continue;
            memset(lds, 0xA5, (size_t)pl.base.lds_floats * sizeof(float)); /* LDS holds whatever the last workgroup left */
            for (uint32_t tid = 0; tid < kThreads; tid++) alacmel::stage_tile(p.m, t, lds, tid);
            for (uint32_t f0 = 0; f0 < t.count; f0 += p.batch) {
                for (uint32_t tid = 0; tid < kThreads; tid++) pack_batch(p, t, lds, buf, f0, tid);
                for (uint32_t s = 0; s < p.n_pass; s++)
                    for (uint32_t tid = 0; tid < kThreads; tid++) pass_batch(p, s, buf, tid);
                for (uint32_t tid = 0; tid < kThreads; tid++) split_batch(p, buf, ptile, f0, tid);
            }
            for (uint32_t tid = 0; tid < kThreads; tid++) {
                if (p.m.n_mels) alacmel::mel_tile(p.m, ptile, lds, tid);
                else alacmel::log_tile(p.m, ptile, tid);
            }
            for (uint32_t tid = 0; tid < kThreads; tid++) {
                if (p.m.n_mels) alacmel::store_tile(p.m, t, lds, p.m.tile_frames, 1u, tid);
                else alacmel::store_tile(p.m, t, ptile, 1u, p.m.KP, tid);
            }
        }
    free(lds);
    if (region) munmap(region, region_len);
    return 0;
}

}  // extern "C"
