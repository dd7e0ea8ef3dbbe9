/*
 * alac_host.h — what the host code of libalacgpu.so shares (alacgpu.hip: the decoder's and the waveform pass's entries;
 * k_enc.hip: the encoder's): the error text behind alacgpu_last_error, the HIP-error macro, the grow-only buffers, the
 * pinned-pointer test and the configuration check. Host only and private to the library: no kernel header includes it,
 * and nothing in it is exported.
 */
#ifndef ALAC_HOST_H
#define ALAC_HOST_H
#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/alacgpu.h"

#pragma GCC visibility push(hidden)
namespace alack {

/* writes the thread-local text behind alacgpu_last_error (alacgpu.hip) */
void set_err(const char* fmt, ...);

#define HIP_TRY(expr)                                                                                \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            alack::set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return ALACGPU_E_HIP;                                                                    \
        }                                                                                            \
    } while (0)

/* a buffer that only grows, an eighth and 256 bytes beyond what is asked for; the old block goes before the new one comes */
template <bool Pinned>
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return ALACGPU_E_OK;
        release();
        size_t want = bytes + bytes / 8 + 256;
        if constexpr (Pinned) HIP_TRY(hipHostMalloc(&p, want, hipHostMallocDefault));
        else HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return ALACGPU_E_OK;
    }
    void release() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
};
using DevBuf = GrowBuf<false>;
using HostBuf = GrowBuf<true>; /* pinned staging */

inline bool is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); /* an ordinary (pageable) pointer: not an error */
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

inline int check_config(const alacgpu_config* cfg) {
    if (cfg->bit_depth != 16 && cfg->bit_depth != 20 && cfg->bit_depth != 24 && cfg->bit_depth != 32) { /* decoder.go:91-93 */
        set_err("invalid configuration: alac: unsupported bit depth: %d", (int)cfg->bit_depth);
        return ALACGPU_E_CONFIG;
    }
    if (cfg->num_channels < 1 || cfg->num_channels > 8) {
        set_err("invalid configuration: NumChannels %d outside 1..8", (int)cfg->num_channels);
        return ALACGPU_E_CONFIG;
    }
    if (cfg->frame_length == 0 || cfg->frame_length > (1u << 24)) {
        set_err("invalid configuration: FrameLength %u", cfg->frame_length);
        return ALACGPU_E_CONFIG;
    }
    return ALACGPU_E_OK;
}

} /* namespace alack */
#pragma GCC visibility pop
#endif
