/*
 * fbankfft_sim.cpp — TEST-ONLY host build of the Kaldi feature pass with transform = fft.
 *
 * Compiles saprobe-alac_amd/csrc/alac_fbankfft.h (the text the gfx950 kernel of k_fbankfft.hip is built from) with g++,
 * contraction off, and runs it the way k_fbankfft.hip launches it: for every tile of every row the phases that
 * alacfbfft::for_each_phase names, each for work items 0..255 through alacfbfft::tile_phase, a barrier behind each. The CPU suite
 * (-m "not gpu") checks it against a numpy restatement, and the GPU suite holds the kernel to it bit for bit. It lives under
 * tests/ and is never linked into libalacgpu.so. tests/host_sim/fbankfft_san_main.cpp calls the same functions from a program of
 * its own.
 */
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../saprobe-alac_amd/csrc/alac_fbankfft.h"

using namespace alacfbfft;

namespace {
/* cfg, dbl: as tests/host_sim/fbank_sim.cpp reads them */
Config config_of(const uint32_t* cfg, const double* dbl) {
    Config c;
    c.sample_rate = cfg[0];
    c.frame_length = cfg[1];
    c.frame_shift = cfg[2];
    c.round_to_power_of_two = cfg[3];
    c.num_mel_bins = cfg[4];
    c.num_ceps = cfg[5];
    c.snip_edges = cfg[6];
    c.remove_dc_offset = cfg[7];
    c.window_type = cfg[8];
    c.use_log_fbank = cfg[9];
    c.use_energy = cfg[10];
    c.raw_energy = cfg[11];
    c.htk_compat = cfg[12];
    c.use_power = cfg[13];
    c.log_energy = cfg[14];
    c.layout = cfg[15];
    c.preemphasis = dbl[0];
    c.blackman_coeff = dbl[1];
    c.low_freq = dbl[2];
    c.high_freq = dbl[3];
    c.energy_floor = dbl[4];
    c.scale = dbl[5];
    c.cepstral_lifter = dbl[6];
    c.dither = dbl[7];
    c.vtln_warp = dbl[8];
    return c;
}
}  // namespace

extern "C" {

/* alacgpu_fbank_create_transform with transform = fft + alacgpu_fbank_plan + alacgpu_fbank_fft_plan: info = the ten numbers of
 * alacgpu_fbank_info, then {transform, tile_frames, lds_bytes, batch_frames, pitch, n_passes, radix[8], window_entries,
 * twiddle_entries}, then the places in LDS {a_floats, p_floats, e_off, c_off, s_off, b_off, parts}: 33 numbers; the table pointers
 * may be NULL. -> 0, or -2 where the entries return ALACGPU_E_ARG. */
int fbankfft_sim_plan(const uint32_t* cfg, const double* dbl, uint32_t* info, float* window_out, uint64_t window_cap, float* tw_out,
                      uint64_t tw_cap, float* fb_out, uint64_t fb_cap, int32_t* first_out, uint64_t first_cap, float* dct_out,
                      uint64_t dct_cap, float* lifter_out, uint64_t lifter_cap) {
    Plan plan;
    if (!cfg || !dbl || !info || !make_plan(config_of(cfg, dbl), &plan)) return -2;
    const alacfb::Plan& pl = plan.base;
    if ((window_out && window_cap < plan.ws.size()) || (tw_out && tw_cap < plan.fft.tw.size()) || (fb_out && fb_cap < pl.fbw.size()) ||
        (first_out && first_cap < pl.first.size()) || (dct_out && dct_cap < pl.dct.size()) || (lifter_out && lifter_cap < pl.lifter.size()))
        return -2;
    uint32_t numbers[33] = {pl.W, pl.hop, pl.N, pl.K, pl.n_mels, pl.taps, pl.num_ceps, pl.cols, pl.tile_frames, pl.lds_floats * 4u,
                            kFft, pl.tile_frames, pl.lds_floats * 4u, plan.batch, plan.fft.pitch, plan.fft.n_pass};
    for (uint32_t s = 0; s < plan.fft.n_pass; s++) numbers[16 + s] = plan.fft.radix[s];
    numbers[24] = (uint32_t)plan.ws.size();
    numbers[25] = (uint32_t)plan.fft.tw.size();
    numbers[26] = pl.a_floats;
    numbers[27] = plan.p_floats;
    numbers[28] = pl.e_off;
    numbers[29] = pl.c_off;
    numbers[30] = plan.s_off;
    numbers[31] = plan.b_off;
    numbers[32] = plan.parts;
    memcpy(info, numbers, sizeof(numbers));
    if (!pl.basis.empty() || !pl.bt.empty()) return -4; /* an FFT plan builds no basis */
    if (window_out) memcpy(window_out, plan.ws.data(), plan.ws.size() * sizeof(float));
    if (tw_out) memcpy(tw_out, plan.fft.tw.data(), plan.fft.tw.size() * sizeof(float));
    if (fb_out) memcpy(fb_out, pl.fbw.data(), pl.fbw.size() * sizeof(float));
    if (first_out) memcpy(first_out, pl.first.data(), pl.first.size() * sizeof(int32_t));
    if (dct_out && !pl.dct.empty()) memcpy(dct_out, pl.dct.data(), pl.dct.size() * sizeof(float));
    if (lifter_out && !pl.lifter.empty()) memcpy(lifter_out, pl.lifter.data(), pl.lifter.size() * sizeof(float));
    return 0;
}

/* The arguments of alacgpu_fbank_device with host pointers. -> 0, or -2 for what the entries reject. guard != 0: the input,
 * (rows - 1) * in_stride + in_frames elements, is copied so that it ENDS at an inaccessible page, and the pass reads the copy:
 * a read behind the last row's samples is fatal. */
int fbankfft_sim_run(const uint32_t* cfg, const double* dbl, const float* in, uint64_t in_stride, uint64_t rows, uint64_t in_frames,
                     float* out, uint64_t out_row_stride, uint64_t out_inner_stride, int guard) {
    Plan pl;
    if (!make_plan(config_of(cfg, dbl), &pl)) return -2;
    if (in_frames > ((uint64_t)1 << 61)) return rows ? -2 : 0;
    if (rows == 0 || alacfb::out_frames_of(pl.base.W, pl.base.hop, pl.base.cfg.snip_edges, in_frames) == 0) return 0;
    Params p;
    if (!make_params(pl, in, in_stride, rows, in_frames, out, out_row_stride, out_inner_stride, pl.ws.data(), pl.fft.tw.data(),
                     pl.fft.pos.data(), pl.base.fbw.data(), pl.base.first.data(), pl.base.dct.data(), pl.base.lifter.data(), &p))
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
        p.fb.m.in = (const float*)copy;
        p.fft.m.in = (const float*)copy;
    }
    /* exactly the plan's LDS, on the heap: an index past it is the sanitizer's to see */
    float* lds = nullptr;
    if (posix_memalign((void**)&lds, 16, (size_t)pl.base.lds_floats * sizeof(float))) return -3;
    for (uint64_t row = 0; row < rows; row++)
        for (uint64_t tile = 0; tile < p.fb.m.tiles_per_row; tile++) {
            const Tile t = alacfb::make_tile(p.fb, row, tile);
            if (t.count == 0) continue;
            memset(lds, 0xA5, (size_t)pl.base.lds_floats * sizeof(float)); /* LDS holds whatever the last workgroup left */
            for_each_phase(p, t, [&](uint32_t phase, uint32_t arg) {
                for (uint32_t tid = 0; tid < kThreads; tid++) tile_phase(p, t, lds, phase, arg, tid);
            });
        }
    free(lds);
    if (region) munmap(region, region_len);
    return 0;
}

}  // extern "C"
