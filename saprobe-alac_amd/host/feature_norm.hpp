// feature_norm.hpp — C++ host-side RAII mirror of the feature normalisation pass of include/alacgpu.h (alacgpu_norm_*; the
// reference has no counterpart: it hands out PCM).
//
//   NewFeatureNorm(config, shift, scale)  -> throws std::invalid_argument where no plan can be built; shift / scale are empty
//                                            (none) or config.bins floats
//   NormConfig(bins, stat, ...)           an alacgpu_norm_config with the defaults (var_floor 1e-20, pad_value 0)
//   FeatureNorm::NormDevice(...)          float32 features on the device with per-row lengths -> normalised features, the
//                                         padding masked; asynchronous on Stream() unless sync
//   FeatureNorm::Plan()                   the numbers, the scratch block as it stands, and the host copies of shift and scale
// Header-only; link with -lalacgpu. Every pass runs the HIP kernels: there is no CPU path.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/alacgpu.h"
#include "pass_handle.hpp"

namespace alac {

inline alacgpu_norm_config NormConfig(uint32_t bins, uint32_t stat = ALACGPU_NORM_STAT_MEAN, float range = 0.0f,
                                      float pad_value = 0.0f, float var_floor = 1e-20f) {
    alacgpu_norm_config c{};
    c.bins = bins;
    c.stat = stat;
    c.var_floor = var_floor;
    c.range = range;
    c.pad_value = pad_value;
    return c;
}

struct NormPlan {
    alacgpu_norm_info info{};
    std::vector<float> shift;  // [bins], or empty
    std::vector<float> scale;  // [bins], or empty
};

using NormStrides = FeatureStrides;

class FeatureNorm {
public:
    explicit FeatureNorm(const alacgpu_norm_config& config, const std::vector<float>& shift = {}, const std::vector<float>& scale = {},
                         int device = 0) {
        if ((!shift.empty() && shift.size() != config.bins) || (!scale.empty() && scale.size() != config.bins))
            throw std::invalid_argument("shift and scale are empty or one float per bin");
        alacgpu_norm* h = nullptr;
        detail::check(alacgpu_norm_create(device, &config, shift.empty() ? nullptr : shift.data(), scale.empty() ? nullptr : scale.data(),
                                          &h));
        h_.reset(h);
    }

    uint64_t OutFrames(uint64_t in_frames) const { return alacgpu_norm_out_frames(h_.get(), in_frames); }

    // device pointers on the handle's device: rows x frames x bins elements of d_in -> the same elements of d_out (which may be
    // d_in with the same strides); d_lengths (int32 per row) and d_stats ([rows][2][bins]) may be null; exactly the output's
    // elements are written
    void NormDevice(const float* d_in, NormStrides in, size_t rows, size_t frames, const int32_t* d_lengths, float* d_out,
                    NormStrides out, float* d_stats = nullptr, bool sync = false) {
        detail::check(alacgpu_norm_device(h_.get(), d_in, in.row, in.frame, in.bin, rows, frames, d_lengths, d_out, out.row, out.frame,
                                          out.bin, d_stats, sync ? 1 : 0));
    }

    NormPlan Plan() const {
        NormPlan p;
        detail::must(alacgpu_norm_plan(h_.get(), &p.info, nullptr, 0, nullptr, 0));
        p.shift.resize(p.info.shift_entries);
        p.scale.resize(p.info.scale_entries);
        detail::must(alacgpu_norm_plan(h_.get(), &p.info, p.shift.data(), p.shift.size(), p.scale.data(), p.scale.size()));
        return p;
    }

    // milliseconds of the last pass: HIP events around its kernels
    float LastMs() {
        float ms = 0;
        detail::must(alacgpu_norm_last_ms(h_.get(), &ms));
        return ms;
    }

    void* Stream() const { return alacgpu_norm_stream(h_.get()); }
    void Synchronize() { detail::must(alacgpu_norm_synchronize(h_.get())); }
    alacgpu_norm* handle() const { return h_.get(); }

private:
    detail::Handle<alacgpu_norm, alacgpu_norm_destroy> h_;
};

inline std::unique_ptr<FeatureNorm> NewFeatureNorm(const alacgpu_norm_config& config, const std::vector<float>& shift = {},
                                                   const std::vector<float>& scale = {}, int device = 0) {
    return std::make_unique<FeatureNorm>(config, shift, scale, device);
}

}  // namespace alac
