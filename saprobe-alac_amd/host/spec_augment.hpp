// spec_augment.hpp — C++ host-side RAII mirror of the SpecAugment pass of include/alacgpu.h (alacgpu_specaug_*; the reference
// has no counterpart: it hands out PCM).
//
//   NewSpecAugment(config)              -> throws std::invalid_argument where no plan can be built
//   SpecAugConfig(bins, ...)            an alacgpu_specaug_config with the defaults (2 masks of up to 27 bins, 2 of up to 100
//                                       frames, no cap by the row's length, no warp, mask_value and pad_value 0)
//   SpecAugment::AugmentDevice(...)     float32 features on the device with per-row lengths -> the warped and masked features,
//                                       and the resolved draws; asynchronous on Stream() unless sync
//   SpecAugment::Plan()                 the parameters, the draws of a row and the tile's numbers
// Header-only; link with -lalacgpu. Every pass runs the HIP kernel: there is no CPU path.
#pragma once

#include <cmath>
#include <cstdint>
#include <memory>

#include "../../include/alacgpu.h"
#include "pass_handle.hpp"

namespace alac {

// time_ratio in [0, 1]: a time mask is at most that share of the row's valid frames; 1: time_width alone caps it
inline alacgpu_specaug_config SpecAugConfig(uint32_t bins, uint32_t freq_masks = 2, uint32_t freq_width = 27, uint32_t time_masks = 2,
                                            uint32_t time_width = 100, double time_ratio = 1.0, uint32_t warp = 0, float mask_value = 0.0f,
                                            float pad_value = 0.0f) {
    alacgpu_specaug_config c{};
    c.bins = bins;
    c.freq_masks = freq_masks;
    c.freq_width = freq_width;
    c.time_masks = time_masks;
    c.time_width = time_width;
    c.time_ratio_q16 = time_ratio >= 0.0 && time_ratio <= 1.0 ? (uint32_t)std::lround(time_ratio * 65536.0) : 0xFFFFFFFFu;  // refused
    c.warp = warp;
    c.mask_value = mask_value;
    c.pad_value = pad_value;
    return c;
}

class SpecAugment {
public:
    explicit SpecAugment(const alacgpu_specaug_config& config, int device = 0) {
        alacgpu_specaug* h = nullptr;
        detail::check(alacgpu_specaug_create(device, &config, &h));
        h_.reset(h);
    }

    // device pointers on the handle's device: rows x frames x bins elements of d_in -> the same elements of d_out, which may
    // not overlap d_in but, on a handle without a warp, may be d_in itself with the same strides. seed: the step's; row r's
    // identity is d_ids[r] (int64 per row) or, where d_ids is null, row_base + r. d_lengths and d_draws (int32 [rows][Plan().draws])
    // may be null; exactly the output's elements and the draws are written
    void AugmentDevice(const float* d_in, FeatureStrides in, size_t rows, size_t frames, const int32_t* d_lengths, uint64_t seed,
                       float* d_out, FeatureStrides out, uint64_t row_base = 0, const int64_t* d_ids = nullptr, int32_t* d_draws = nullptr,
                       bool sync = false) {
        detail::check(alacgpu_specaug_device(h_.get(), d_in, in.row, in.frame, in.bin, rows, frames, d_lengths, seed, row_base, d_ids,
                                             d_out, out.row, out.frame, out.bin, d_draws, sync ? 1 : 0));
    }

    alacgpu_specaug_info Plan() const {
        alacgpu_specaug_info info{};
        detail::must(alacgpu_specaug_plan(h_.get(), &info));
        return info;
    }

    // milliseconds of the last pass: HIP events around its kernel
    float LastMs() {
        float ms = 0;
        detail::must(alacgpu_specaug_last_ms(h_.get(), &ms));
        return ms;
    }

    void* Stream() const { return alacgpu_specaug_stream(h_.get()); }
    void Synchronize() { detail::must(alacgpu_specaug_synchronize(h_.get())); }
    alacgpu_specaug* handle() const { return h_.get(); }

private:
    detail::Handle<alacgpu_specaug, alacgpu_specaug_destroy> h_;
};

inline std::unique_ptr<SpecAugment> NewSpecAugment(const alacgpu_specaug_config& config, int device = 0) {
    return std::make_unique<SpecAugment>(config, device);
}

}  // namespace alac
