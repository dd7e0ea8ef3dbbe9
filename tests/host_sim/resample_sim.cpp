/*
 * resample_sim.cpp — TEST-ONLY host build of the resampler.
 *
 * Compiles saprobe-alac_amd/csrc/alac_resample.h (the text the gfx950 kernel of k_resample.hip is built from) with g++ and
 * runs it the way k_resample.hip launches it: for every tile of every row the staging phase for work items 0..255, the
 * barrier, the chains for work items 0..255, the barrier, and the store phase for work items 0..255. The CPU suite (-m "not
 * gpu") checks it against a numpy restatement, and the GPU suite holds the kernel to it bit for bit. It lives under tests/
 * and is never linked into libalacgpu.so.
 */
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/csrc/alac_resample.h"

using namespace alacrs;

extern "C" {

/* alacgpu_resampler_create + alacgpu_resampler_plan: info = {o, n, width, taps, tile_out}; h_out / first_out may be NULL.
 * -> 0, or -2 where the entries return ALACGPU_E_ARG. */
int resample_sim_plan(uint32_t orig, uint32_t new_, uint32_t W, double rolloff, uint32_t* info, float* h_out, uint64_t h_cap,
                      int32_t* first_out, uint64_t first_cap) {
    Plan pl;
    if (!info || !make_plan(orig, new_, W, rolloff, &pl)) return -2;
    if ((h_out && h_cap < pl.h.size()) || (first_out && first_cap < pl.first.size())) return -2;
    info[0] = pl.o;
    info[1] = pl.n;
    info[2] = pl.width;
    info[3] = pl.taps;
    info[4] = pl.tile_out;
    if (h_out) memcpy(h_out, pl.h.data(), pl.h.size() * sizeof(float));
    if (first_out) memcpy(first_out, pl.first.data(), pl.first.size() * sizeof(int32_t));
    return 0;
}

/* The arguments of alacgpu_resample_device with host pointers, the plan's arguments spelled out. -> 0, or -2 for what the
 * entries reject. guard != 0: the input, (rows - 1) * in_stride + in_frames elements, is copied so that it ENDS at an
 * inaccessible page, and the pass reads the copy: a read behind the last row's frames is fatal. */
int resample_sim_run(uint32_t orig, uint32_t new_, uint32_t W, double rolloff, const float* in, uint64_t in_stride, uint64_t rows,
                     uint64_t in_frames, float* out, uint64_t out_stride, int guard) {
    Plan pl;
    if (!make_plan(orig, new_, W, rolloff, &pl)) return -2;
    if (rows == 0 || in_frames == 0) return 0;
    Params p;
    if (!make_params(pl, in, in_stride, rows, in_frames, out, out_stride, pl.ht.data(), pl.first.data(), &p)) return -2;

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
        p.in = (const float*)copy;
    }
    alignas(16) static thread_local float stage[kStageFloats];
    alignas(16) static thread_local float outb[kOutFloats];
    for (uint64_t row = 0; row < rows; row++)
        for (uint64_t tile = 0; tile < p.tiles_per_row; tile++) {
            const Tile t = make_tile(p, row, tile);
            if (t.count == 0) continue;
            memset(stage, 0xA5, sizeof(stage)); /* LDS holds whatever the last workgroup left */
            memset(outb, 0xA5, sizeof(outb));
            for (uint32_t tid = 0; tid < kThreads; tid++) stage_tile(p, t, stage, tid);
            for (uint32_t tid = 0; tid < kThreads; tid++) compute_tile(p, t, stage, outb, tid);
            for (uint32_t tid = 0; tid < kThreads; tid++) store_tile(p, t, outb, tid);
        }
    if (region) munmap(region, region_len);
    return 0;
}

/* alacgpu_resample_out_frames; 0 when there is no plan or the product overflows */
uint64_t resample_sim_out_frames(uint32_t orig, uint32_t new_, uint64_t in_frames) {
    uint32_t a = orig, b = new_;
    while (b) {
        const uint32_t r = a % b;
        a = b;
        b = r;
    }
    uint64_t of = 0;
    if (!a || !new_ || !out_frames_of(orig / a, new_ / a, in_frames, &of)) return 0;
    return of;
}

/* the staging buffer, and what a tile of the plan's tile_out columns can need of it */
uint32_t resample_sim_stage_floats(void) { return kStageFloats; }
uint64_t resample_sim_stage_need(uint32_t orig, uint32_t new_, uint32_t W, double rolloff) {
    Plan pl;
    if (!make_plan(orig, new_, W, rolloff, &pl)) return 0;
    return stage_need(pl, pl.tile_out);
}

}  // extern "C"
