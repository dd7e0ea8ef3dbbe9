// pass_handle.hpp — what the RAII mirrors of the row passes share (resampler.hpp, mel_spectrogram.hpp, kaldi_features.hpp,
// feature_norm.hpp, frame_stack.hpp): how a return code becomes an exception and the owning pointer of a handle (alac::detail:
// no part of their interface), and the strides of a feature tensor, which the last two take. Header-only.
#pragma once

#include <memory>
#include <stdexcept>

#include "../../include/alacgpu.h"

namespace alac {
// the three element strides of a feature tensor: element (r, f, b) at base + r * row + f * frame + b * bin; frame or bin is 1
struct FeatureStrides {
    size_t row, frame, bin;
};
}  // namespace alac

namespace alac::detail {

// create and the device entry: what the caller passed and the library refused is std::invalid_argument
inline void check(int rc) {
    if (rc == ALACGPU_E_ARG) throw std::invalid_argument(alacgpu_last_error());
    if (rc != ALACGPU_E_OK) throw std::runtime_error(alacgpu_last_error());
}

// the other entries of a live handle (plan, last_ms, synchronize): every failure is std::runtime_error
inline void must(int rc) {
    if (rc != ALACGPU_E_OK) throw std::runtime_error(alacgpu_last_error());
}

template <auto Destroy>
struct Destroyer {
    template <typename H>
    void operator()(H* h) const {
        Destroy(h);
    }
};

// std::unique_ptr over a handle of the C interface and its alacgpu_*_destroy
template <typename H, auto Destroy>
using Handle = std::unique_ptr<H, Destroyer<Destroy>>;

}  // namespace alac::detail
