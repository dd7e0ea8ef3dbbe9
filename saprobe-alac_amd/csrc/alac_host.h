/*
 * alac_host.h — what the host code of libalacgpu.so shares (alacgpu.hip: the decoder's and the waveform pass's entries;
 * k_enc.hip: the encoder's; k_resample.hip, k_mel.hip, k_melfft.hip, k_fbank.hip, k_fbankfft.hip, k_featnorm.hip,
 * k_stack.hip and k_specaug.hip: the row passes'): the error text behind alacgpu_last_error, the HIP-error macro, the grow-only
 * buffers, the pinned-pointer test, the configuration check, and the skeleton of a row pass: PassHandle and launch_tiles. Host
 * only and private to the library: no kernel header includes it, and nothing in it is exported.
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

/* the refusal of a NULL handle or result pointer */
inline int null_argument() {
    set_err("null argument");
    return ALACGPU_E_ARG;
}

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

/* What the handle of a row pass (resampler, spectrogram, Kaldi features) is besides its plan: a device, a stream of its own,
 * an event pair around the kernels of the last pass, and the plan's tables on the device. The handle struct
 * derives from it; create opens it and uploads the tables, destroy closes it. */
struct PassHandle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr; /* around the kernels of the last pass */
    bool timed = false;
    hipError_t err = hipSuccess; /* the first failure of open() or upload(); what follows one is skipped */
    std::vector<void*> blocks;   /* the tables, close() frees them */

    void open(int dev) {
        device = dev;
        err = hipSetDevice(dev);
        if (err == hipSuccess) err = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        if (err == hipSuccess) err = hipEventCreate(&ev0);
        if (err == hipSuccess) err = hipEventCreate(&ev1);
    }

    /* a table on the device; an empty one still gets a block, so that the kernel's arguments are never NULL */
    template <typename T>
    void upload(T** d, const std::vector<T>& v) {
        if (err == hipSuccess) err = hipMalloc((void**)d, (v.empty() ? 1 : v.size()) * sizeof(T));
        if (err != hipSuccess) return;
        blocks.push_back(*d);
        if (!v.empty()) err = hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }

    void close() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* b : blocks) (void)hipFree(b);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }

    int synchronize() {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamSynchronize(stream));
        return ALACGPU_E_OK;
    }

    /* `what` names the pass: "no <what> pass on this handle yet" */
    int last_ms(float* ms, const char* what) {
        if (!ms || !timed) {
            if (!ms) set_err("null argument");
            else set_err("no %s pass on this handle yet", what);
            return ALACGPU_E_ARG;
        }
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipEventSynchronize(ev1));
        HIP_TRY(hipEventElapsedTime(ms, ev0, ev1));
        return ALACGPU_E_OK;
    }

    /* one pass: launch(stream) -> hipError_t between the two events */
    template <typename F>
    int run(bool sync, F&& launch) {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipEventRecord(ev0, stream));
        HIP_TRY(launch(stream));
        HIP_TRY(hipEventRecord(ev1, stream));
        timed = true;
        if (sync) HIP_TRY(hipStreamSynchronize(stream));
        return ALACGPU_E_OK;
    }
};

/* A kernel(params, first_tile) over `tiles` workgroups of `threads`, in slices far below a dispatch's 2^32 work-items: 2^22
 * workgroups of 256 */
constexpr uint64_t kTilesPerLaunch = (uint64_t)1 << 22;

template <typename Params>
hipError_t launch_tiles(void (*kernel)(Params, uint64_t), uint64_t tiles, uint32_t threads, uint32_t lds_bytes, hipStream_t stream,
                        const Params& p) {
    for (uint64_t t0 = 0; t0 < tiles; t0 += kTilesPerLaunch) {
        const uint64_t m = tiles - t0 < kTilesPerLaunch ? tiles - t0 : kTilesPerLaunch;
        hipLaunchKernelGGL(kernel, dim3((unsigned)m), dim3(threads), lds_bytes, stream, p, t0);
    }
    return hipGetLastError();
}

} /* namespace alack */
#pragma GCC visibility pop
#endif
