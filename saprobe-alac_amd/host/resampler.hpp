// resampler.hpp — C++ host-side RAII mirror of the resampler of include/alacgpu.h (alacgpu_resampler_*; the reference has no
// counterpart: it hands out PCM at the file's rate).
//
//   NewResampler(orig, new)               -> throws std::invalid_argument where no plan can be built
//   Resampler::OutFrames(T)               ceil(new * T / orig)
//   Resampler::ResampleDevice(...)        float32 rows on the device, asynchronous on Stream() unless sync
//   Resampler::Plan()                     the numbers and the host copies of the table the kernel uses
// Header-only; link with -lalacgpu. Every pass runs the HIP kernel: there is no CPU path.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/alacgpu.h"
#include "pass_handle.hpp"

namespace alac {

struct ResamplePlan {
    alacgpu_resample_info info{};
    std::vector<float> h;       // [n][taps]
    std::vector<int32_t> first; // [n]: the tap index of each phase's first kept tap
};

class Resampler {
public:
    Resampler(uint32_t orig_freq, uint32_t new_freq, int device = 0, uint32_t lowpass_filter_width = 6, double rolloff = 0.99) {
        alacgpu_resampler* h = nullptr;
        detail::check(alacgpu_resampler_create(device, orig_freq, new_freq, lowpass_filter_width, rolloff, &h));
        h_.reset(h);
    }

    uint64_t OutFrames(uint64_t in_frames) const { return alacgpu_resample_out_frames(h_.get(), in_frames); }

    // device pointers on the resampler's device, strides in elements: rows of in_frames float32 frames -> rows of
    // OutFrames(in_frames); exactly those columns of every output row are written
    void ResampleDevice(const float* d_in, size_t in_row_stride, size_t rows, size_t in_frames, float* d_out,
                        size_t out_row_stride, bool sync = false) {
        detail::check(alacgpu_resample_device(h_.get(), d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, sync ? 1 : 0));
    }

    ResamplePlan Plan() const {
        ResamplePlan p;
        detail::must(alacgpu_resampler_plan(h_.get(), &p.info, nullptr, 0, nullptr, 0));
        p.h.resize((size_t)p.info.n * p.info.taps);
        p.first.resize(p.info.n);
        detail::must(alacgpu_resampler_plan(h_.get(), &p.info, p.h.data(), p.h.size(), p.first.data(), p.first.size()));
        return p;
    }

    // milliseconds of the last pass: HIP events around its kernels
    float LastMs() {
        float ms = 0;
        detail::must(alacgpu_resampler_last_ms(h_.get(), &ms));
        return ms;
    }

    void* Stream() const { return alacgpu_resampler_stream(h_.get()); }
    void Synchronize() { detail::must(alacgpu_resampler_synchronize(h_.get())); }
    alacgpu_resampler* handle() const { return h_.get(); }

private:
    detail::Handle<alacgpu_resampler, alacgpu_resampler_destroy> h_;
};

inline std::unique_ptr<Resampler> NewResampler(uint32_t orig_freq, uint32_t new_freq, int device = 0,
                                               uint32_t lowpass_filter_width = 6, double rolloff = 0.99) {
    return std::make_unique<Resampler>(orig_freq, new_freq, device, lowpass_filter_width, rolloff);
}

}  // namespace alac
