// frame_stack.hpp — C++ host-side RAII mirror of the frame stacking pass of include/alacgpu.h (alacgpu_stack_*; the reference
// has no counterpart: it hands out PCM).
//
//   NewFrameStack(config)            -> throws std::invalid_argument where no plan can be built
//   StackConfig(bins, order, ...)    an alacgpu_stack_config with the defaults (window 2, no context, stride 1, pad_value 0)
//   LfrConfig(bins, m, n)            FunASR's apply_lfr(m, n): left (m - 1) / 2, right m - 1 - left, stride n
//   FrameStack::StackDevice(...)     float32 features on the device with per-row lengths -> deltas, context and subsampling with
//                                    lengths of their own; asynchronous on Stream() unless sync
//   FrameStack::Plan()               the tile's numbers and the host copies of the delta weights
// Header-only; link with -lalacgpu. Every pass runs the HIP kernel: there is no CPU path.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/alacgpu.h"
#include "pass_handle.hpp"

namespace alac {

inline alacgpu_stack_config StackConfig(uint32_t bins, uint32_t order = 0, uint32_t window = 2, uint32_t left = 0, uint32_t right = 0,
                                        uint32_t stride = 1, float pad_value = 0.0f) {
    alacgpu_stack_config c{};
    c.bins = bins;
    c.order = order;
    c.window = window;
    c.left = left;
    c.right = right;
    c.stride = stride;
    c.pad_value = pad_value;
    return c;
}

inline alacgpu_stack_config LfrConfig(uint32_t bins, uint32_t m = 7, uint32_t n = 6, float pad_value = 0.0f) {
    const uint32_t left = m ? (m - 1) / 2 : 0;
    return StackConfig(bins, 0, 2, left, m ? m - 1 - left : 0, n, pad_value);
}

struct StackPlan {
    alacgpu_stack_info info{};
    std::vector<float> w1;  // [2 window + 1], or empty
    std::vector<float> w2;  // [4 window + 1], or empty
};

using StackStrides = FeatureStrides;

class FrameStack {
public:
    explicit FrameStack(const alacgpu_stack_config& config, int device = 0) {
        alacgpu_stack* h = nullptr;
        detail::check(alacgpu_stack_create(device, &config, &h));
        h_.reset(h);
    }

    // ceil(in_frames / stride)
    uint64_t OutFrames(uint64_t in_frames) const { return alacgpu_stack_out_frames(h_.get(), in_frames); }

    // device pointers on the handle's device: rows x frames x bins elements of d_in -> rows x OutFrames(frames) x info.columns
    // elements of d_out, which may not overlap d_in; d_lengths and d_out_lengths (int32 per row) may be null; exactly the
    // output's elements and the out lengths are written
    void StackDevice(const float* d_in, StackStrides in, size_t rows, size_t frames, const int32_t* d_lengths, float* d_out,
                     StackStrides out, int32_t* d_out_lengths = nullptr, bool sync = false) {
        detail::check(alacgpu_stack_device(h_.get(), d_in, in.row, in.frame, in.bin, rows, frames, d_lengths, d_out, out.row, out.frame,
                                           out.bin, d_out_lengths, sync ? 1 : 0));
    }

    StackPlan Plan() const {
        StackPlan p;
        detail::must(alacgpu_stack_plan(h_.get(), &p.info, nullptr, 0));
        std::vector<float> w(p.info.w1_entries + p.info.w2_entries);
        detail::must(alacgpu_stack_plan(h_.get(), &p.info, w.data(), w.size()));
        p.w1.assign(w.begin(), w.begin() + p.info.w1_entries);
        p.w2.assign(w.begin() + p.info.w1_entries, w.end());
        return p;
    }

    // milliseconds of the last pass: HIP events around its kernel
    float LastMs() {
        float ms = 0;
        detail::must(alacgpu_stack_last_ms(h_.get(), &ms));
        return ms;
    }

    void* Stream() const { return alacgpu_stack_stream(h_.get()); }
    void Synchronize() { detail::must(alacgpu_stack_synchronize(h_.get())); }
    alacgpu_stack* handle() const { return h_.get(); }

private:
    detail::Handle<alacgpu_stack, alacgpu_stack_destroy> h_;
};

inline std::unique_ptr<FrameStack> NewFrameStack(const alacgpu_stack_config& config, int device = 0) {
    return std::make_unique<FrameStack>(config, device);
}

}  // namespace alac
