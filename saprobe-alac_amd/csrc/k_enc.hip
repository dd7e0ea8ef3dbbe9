/*
 * k_enc.hip — the batch ALAC encoder: gfx950 kernels over csrc/alac_enc.h and the encoder entries of include/alacgpu.h
 * (one translation unit of libalacgpu.so; nothing here touches the decode kernels or their launches).
 *
 * One encode = these launches on the handle's stream:
 *   alac_enc_chains   one lane per channel chain of a packet (the U and V chains of a CPE apart, 64-lane workgroups so that
 *                     the waves spread over every CU): warm pass, predictor and Golomb writer into the chain's scratch
 *   alac_enc_layout   one lane per packet: escape per element, segment table and size; the workgroup's sum of sizes
 *   alac_enc_scan     one workgroup: exclusive scan of the workgroup sums (the scan across workgroups), total = offsets[n]
 *   alac_enc_offsets  one lane per packet: the scan inside the workgroup + its base = offsets[i]; largest packet
 *   alac_enc_pack     one wave per packet: every lane funnel-shifts the segments into one output dword at a time (byte
 *                     stores only at the packet's two unaligned ends, where the neighbours' bytes share the dword)
 * Everything is written with vector stores; the two counters of the cookie are global atomics.
 *
 * The waveform entries (alacgpu_pcm_from_waveform_device, alacgpu_encode_waveform_device) are host code here, beside the
 * handle they extend; their kernel is k_wavepack.hip's (alac_wavepack.h).
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "alac_enc.h"
#include "alac_host.h"
#include "alac_wavepack.h"

using namespace alacenc;
using namespace alack;

namespace {

constexpr int kScanThreads = 256;
constexpr uint64_t kChainsPerLaunch = (uint64_t)1 << 26;  /* alac_enc_chains: lanes per launch */
constexpr uint64_t kPacketsPerPack = (uint64_t)1 << 24;   /* alac_enc_pack: 64 lanes a packet, 2^30 per launch */
/* the one-lane-per-packet kernels and the single-workgroup scan take a batch in one launch: below 2^31 packets */
constexpr uint64_t kMaxPackets = ((uint64_t)1 << 31) - 1;

struct EncStats {
    unsigned long long total_bytes;
    unsigned int max_packet;
    unsigned int pad0;
};

/* ---- kernels ------------------------------------------------------------------------------------------------------- */
__global__ void __launch_bounds__(64) alac_enc_chains(Params p, const uint8_t* __restrict__ pcm, uint32_t* __restrict__ streams,
                                                      ChainResult* __restrict__ res, uint64_t first_chain) {
    const uint64_t t = first_chain + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.n_packets * p.nch) return;
    encode_chain(p, pcm, t / p.nch, (uint32_t)(t % p.nch), streams + t * p.chain_words, res + t);
}

/* block-wide inclusive scan of one uint64 per thread (kScanThreads threads) */
__device__ uint64_t block_scan(uint64_t v, uint64_t* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const uint64_t add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    return sh[t];
}

__global__ void __launch_bounds__(kScanThreads) alac_enc_layout(Params p, const ChainResult* __restrict__ res, Layout* __restrict__ lay,
                                                                uint64_t* __restrict__ block_sums) {
    __shared__ uint64_t sh[kScanThreads];
    const uint64_t pk = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    uint64_t bytes = 0;
    if (pk < p.n_packets) {
        build_layout(p, pk, res + pk * p.nch, pk * p.nch * p.chain_words, lay + pk);
        bytes = lay[pk].bytes;
    }
    const uint64_t sum = block_scan(bytes, sh);
    if (threadIdx.x == kScanThreads - 1) block_sums[blockIdx.x] = sum;
}

/* one workgroup: block_sums[b] -> exclusive prefix; offsets[n] = total */
__global__ void __launch_bounds__(kScanThreads) alac_enc_scan(uint64_t* __restrict__ block_sums, uint64_t nblocks, uint64_t* __restrict__ offsets,
                                                              uint64_t n, EncStats* __restrict__ stats) {
    __shared__ uint64_t sh[kScanThreads];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nblocks; base += kScanThreads) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < nblocks ? block_sums[i] : 0;
        const uint64_t inc = block_scan(v, sh);
        if (i < nblocks) block_sums[i] = carry + inc - v;
        carry += sh[kScanThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        offsets[n] = carry;
        atomicAdd(&stats->total_bytes, (unsigned long long)carry);
    }
}

__global__ void __launch_bounds__(kScanThreads) alac_enc_offsets(Params p, const Layout* __restrict__ lay, const uint64_t* __restrict__ block_base,
                                                                 uint64_t* __restrict__ offsets, EncStats* __restrict__ stats) {
    __shared__ uint64_t sh[kScanThreads];
    const uint64_t pk = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const uint32_t bytes = pk < p.n_packets ? lay[pk].bytes : 0u;
    const uint64_t inc = block_scan(bytes, sh);
    if (pk < p.n_packets) offsets[pk] = block_base[blockIdx.x] + inc - bytes;
    __syncthreads();
    /* the largest packet of the workgroup, then one atomic */
    sh[threadIdx.x] = bytes;
    __syncthreads();
    for (int d = kScanThreads / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d && sh[threadIdx.x + d] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0 && sh[0]) atomicMax(&stats->max_packet, (unsigned int)sh[0]);
}

__global__ void __launch_bounds__(256) alac_enc_pack(Params p, const Layout* __restrict__ lay, const uint32_t* __restrict__ streams,
                                                     const uint8_t* __restrict__ pcm, const uint64_t* __restrict__ offsets,
                                                     uint8_t* __restrict__ blob, uint64_t first_packet) {
    const uint64_t pk = first_packet + (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (pk >= p.n_packets) return;
    const Layout& L = lay[pk];
    /* dwords of the ABSOLUTE address space, so that the stores are aligned whatever d_blob's alignment */
    const uint64_t a0 = (uint64_t)(uintptr_t)blob + offsets[pk], a1 = a0 + L.bytes;
    uint32_t cursor = 0;
    for (uint64_t D = a0 / 4u + lane; D * 4u < a1; D += 64u) {
        const uint64_t a = D * 4u;
        const uint32_t v = window(p, L, streams, pcm, 8 * ((int64_t)a - (int64_t)a0), cursor);
        uint8_t* dst = (uint8_t*)(uintptr_t)a;
        if (a >= a0 && a + 4u <= a1) {
            *(uint32_t*)dst = __builtin_bswap32(v);
        } else {
            for (uint32_t k = 0; k < 4; k++)
                if (a + k >= a0 && a + k < a1) dst[k] = (uint8_t)(v >> (24u - 8u * k));
        }
    }
}

} /* namespace */

/* ---- host side (alac_host.h) ---------------------------------------------------------------------------------------- */
struct alacgpu_encoder {
    alacgpu_config cfg;
    int device;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    uint64_t frames_done = 0;
    EncStats* stats = nullptr;
    DevBuf res, streams, lay, sums;    /* the kernels' scratch */
    DevBuf d_pcm, d_blob, d_off;       /* alacgpu_encode's device copies */
    HostBuf h_in, h_out, h_off;        /* alacgpu_encode's staging */
    DevBuf wave_pcm;                   /* alacgpu_encode_waveform_device: the pack pass's PCM */
    hipEvent_t ev_w0 = nullptr, ev_w1 = nullptr; /* around the kernels of the last pack pass */
    bool wave_timed = false;
};

namespace {
void release(alacgpu_encoder* e) {
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (DevBuf* m : {&e->res, &e->streams, &e->lay, &e->sums, &e->d_pcm, &e->d_blob, &e->d_off, &e->wave_pcm}) m->release();
    for (HostBuf* m : {&e->h_in, &e->h_out, &e->h_off}) m->release();
    if (e->stats) (void)hipFree(e->stats);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->ev_w0) (void)hipEventDestroy(e->ev_w0);
    if (e->ev_w1) (void)hipEventDestroy(e->ev_w1);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}
} /* namespace */

extern "C" {

int alacgpu_encoder_create(const alacgpu_config* cfg, int device, alacgpu_encoder** out) {
    if (!cfg || !out) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    *out = nullptr;
    if (int rc = check_config(cfg)) return rc;
    HIP_TRY(hipSetDevice(device));
    alacgpu_encoder* e = new (std::nothrow) alacgpu_encoder();
    if (!e) {
        set_err("out of memory");
        return ALACGPU_E_ARG;
    }
    e->cfg = *cfg;
    e->device = device;
    hipError_t h = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (h == hipSuccess) h = hipEventCreate(&e->ev0);
    if (h == hipSuccess) h = hipEventCreate(&e->ev1);
    if (h == hipSuccess) h = hipEventCreate(&e->ev_w0);
    if (h == hipSuccess) h = hipEventCreate(&e->ev_w1);
    if (h == hipSuccess) h = hipMalloc((void**)&e->stats, sizeof(EncStats));
    if (h == hipSuccess) h = hipMemsetAsync(e->stats, 0, sizeof(EncStats), e->stream);
    if (h == hipSuccess) h = hipStreamSynchronize(e->stream);
    if (h != hipSuccess) {
        set_err("encoder creation failed: %s", hipGetErrorString(h));
        release(e);
        return ALACGPU_E_HIP;
    }
    *out = e;
    return ALACGPU_E_OK;
}

void alacgpu_encoder_destroy(alacgpu_encoder* e) {
    if (e) release(e);
}

uint64_t alacgpu_encode_max_bytes(const alacgpu_encoder* e, uint64_t total_frames) {
    return e ? max_bytes(e->cfg, total_frames) : 0;
}

int alacgpu_encode_device(alacgpu_encoder* e, const uint8_t* d_pcm, uint64_t total_frames, uint8_t* d_blob, uint64_t blob_cap,
                          uint64_t* d_offsets, int sync) {
    if (!e || !d_offsets || (total_frames && (!d_pcm || !d_blob))) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    if (blob_cap < max_bytes(e->cfg, total_frames)) {
        set_err("blob_cap below alacgpu_encode_max_bytes()");
        return ALACGPU_E_ARG;
    }
    const Params p = make_params(e->cfg, total_frames);
    if (p.n_packets > kMaxPackets) {
        set_err("more than 2^31 - 1 packets in one encode");
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    const uint64_t n = p.n_packets, chains = n * p.nch;
    const uint64_t blocks = (n + kScanThreads - 1) / kScanThreads;
    if (n) {
        if (int rc = e->res.ensure(chains * sizeof(ChainResult))) return rc;
        if (int rc = e->streams.ensure(chains * p.chain_words * sizeof(uint32_t))) return rc;
        if (int rc = e->lay.ensure(n * sizeof(Layout))) return rc;
        if (int rc = e->sums.ensure(blocks * sizeof(uint64_t))) return rc;
    }
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    if (n) {
        ChainResult* res = (ChainResult*)e->res.p;
        uint32_t* streams = (uint32_t*)e->streams.p;
        Layout* lay = (Layout*)e->lay.p;
        uint64_t* sums = (uint64_t*)e->sums.p;
        /* the two kernels with more than one work-item per packet go in slices, each far below a dispatch's 2^32 work-items */
        for (uint64_t c0 = 0; c0 < chains; c0 += kChainsPerLaunch) {
            const uint64_t m = chains - c0 < kChainsPerLaunch ? chains - c0 : kChainsPerLaunch;
            hipLaunchKernelGGL(alac_enc_chains, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, e->stream, p, d_pcm, streams, res, c0);
        }
        hipLaunchKernelGGL(alac_enc_layout, dim3((unsigned)blocks), dim3(kScanThreads), 0, e->stream, p, res, lay, sums);
        hipLaunchKernelGGL(alac_enc_scan, dim3(1), dim3(kScanThreads), 0, e->stream, sums, blocks, d_offsets, n, e->stats);
        hipLaunchKernelGGL(alac_enc_offsets, dim3((unsigned)blocks), dim3(kScanThreads), 0, e->stream, p, lay, sums, d_offsets,
                           e->stats);
        for (uint64_t p0 = 0; p0 < n; p0 += kPacketsPerPack) {
            const uint64_t m = n - p0 < kPacketsPerPack ? n - p0 : kPacketsPerPack;
            hipLaunchKernelGGL(alac_enc_pack, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, e->stream, p, lay, streams, d_pcm,
                               d_offsets, d_blob, p0);
        }
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, sizeof(uint64_t), e->stream));
    }
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    e->timed = true;
    e->frames_done += total_frames;
    if (sync) HIP_TRY(hipStreamSynchronize(e->stream));
    return ALACGPU_E_OK;
}

/* ---- waveforms in (alac_wavepack.h, k_wavepack.hip) ------------------------------------------------------------------- */
} /* extern "C" */

namespace {
/* what both waveform entries reject before any HIP call; -> the pass's parameters */
int wave_args(const alacgpu_encoder* e, const void* d_wave, int layout, int type, size_t channel_stride, size_t packet_stride,
              uint64_t total_frames, alacwp::Params* out) {
    if ((layout != ALACGPU_WAVE_STREAM && layout != ALACGPU_WAVE_PACKETS) || (type != ALACGPU_WAVE_FLOAT && type != ALACGPU_WAVE_INT)) {
        set_err("unknown waveform layout %d or type %d", layout, type);
        return ALACGPU_E_ARG;
    }
    if ((uintptr_t)d_wave & 3u) {
        set_err("d_wave is not 4-byte aligned");
        return ALACGPU_E_ARG;
    }
    const uint32_t fl = e->cfg.frame_length, nch = e->cfg.num_channels;
    if (layout == ALACGPU_WAVE_STREAM ? channel_stride < total_frames
                                      : (channel_stride < fl || packet_stride / nch < channel_stride)) {
        set_err("waveform strides below the tensor's extent");
        return ALACGPU_E_ARG;
    }
    if (alacwp::packets_of(total_frames, fl) > kMaxPackets) {
        set_err("more than 2^31 - 1 packets in one encode");
        return ALACGPU_E_ARG;
    }
    *out = alacwp::make_params(fl, e->cfg.bit_depth, nch, (uint32_t)layout, (uint32_t)type, total_frames);
    out->wave = (const uint8_t*)d_wave;
    out->channel_stride = channel_stride;
    out->packet_stride = packet_stride;
    return ALACGPU_E_OK;
}

/* the pass on the handle's stream between its own events */
int wave_pass(alacgpu_encoder* e, alacwp::Params p, uint8_t* d_pcm, uint64_t* d_clipped) {
    p.pcm = d_pcm;
    HIP_TRY(hipEventRecord(e->ev_w0, e->stream));
    HIP_TRY(wavepack_launch(e->stream, p, d_clipped, alacwp::kTilesPerLaunch));
    HIP_TRY(hipEventRecord(e->ev_w1, e->stream));
    e->wave_timed = true;
    return ALACGPU_E_OK;
}
} /* namespace */

extern "C" {

int alacgpu_pcm_from_waveform_device(alacgpu_encoder* e, const void* d_wave, int layout, int type, size_t channel_stride,
                                     size_t packet_stride, uint64_t total_frames, uint8_t* d_pcm, uint64_t* d_clipped, int sync) {
    if (!e || !d_wave || !d_pcm) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    alacwp::Params p;
    if (int rc = wave_args(e, d_wave, layout, type, channel_stride, packet_stride, total_frames, &p)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    if (int rc = wave_pass(e, p, d_pcm, d_clipped)) return rc;
    if (sync) HIP_TRY(hipStreamSynchronize(e->stream));
    return ALACGPU_E_OK;
}

int alacgpu_encode_waveform_device(alacgpu_encoder* e, const void* d_wave, int layout, int type, size_t channel_stride,
                                   size_t packet_stride, uint64_t total_frames, uint8_t* d_blob, uint64_t blob_cap,
                                   uint64_t* d_offsets, uint64_t* d_clipped, int sync) {
    if (!e || !d_wave || !d_blob || !d_offsets) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    alacwp::Params p;
    if (int rc = wave_args(e, d_wave, layout, type, channel_stride, packet_stride, total_frames, &p)) return rc;
    if (blob_cap < max_bytes(e->cfg, total_frames)) {
        set_err("blob_cap below alacgpu_encode_max_bytes()");
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    const uint64_t pcm_bytes = total_frames * p.bpf;
    if (int rc = e->wave_pcm.ensure(pcm_bytes ? pcm_bytes : 1)) return rc;
    if (int rc = wave_pass(e, p, (uint8_t*)e->wave_pcm.p, d_clipped)) return rc;
    return alacgpu_encode_device(e, (const uint8_t*)e->wave_pcm.p, total_frames, d_blob, blob_cap, d_offsets, sync);
}

int alacgpu_encoder_waveform_last_ms(alacgpu_encoder* e, float* ms) {
    if (!e || !ms || !e->wave_timed) {
        set_err(!e || !ms ? "null argument" : "no waveform pass on this handle yet");
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipEventSynchronize(e->ev_w1));
    HIP_TRY(hipEventElapsedTime(ms, e->ev_w0, e->ev_w1));
    return ALACGPU_E_OK;
}

int alacgpu_encode(alacgpu_encoder* e, const uint8_t* pcm, uint64_t total_frames, uint8_t* blob, uint64_t blob_cap,
                   uint64_t* offsets, uint64_t* blob_bytes_out) {
    if (!e || !offsets || (total_frames && (!pcm || !blob))) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    const uint64_t need = max_bytes(e->cfg, total_frames);
    if (blob_cap < need) {
        set_err("blob_cap below alacgpu_encode_max_bytes()");
        return ALACGPU_E_ARG;
    }
    const Params p = make_params(e->cfg, total_frames);
    if (p.n_packets > kMaxPackets) {
        set_err("more than 2^31 - 1 packets in one encode");
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    const uint64_t n = p.n_packets;
    const uint64_t pcm_bytes = total_frames * p.nch * p.bps;
    if (int rc = e->d_pcm.ensure(pcm_bytes ? pcm_bytes : 1)) return rc;
    if (int rc = e->d_blob.ensure(need ? need : 1)) return rc;
    if (int rc = e->d_off.ensure((n + 1) * sizeof(uint64_t))) return rc;
    if (int rc = e->h_off.ensure((n + 1) * sizeof(uint64_t))) return rc;
    if (pcm_bytes) {
        const void* src = pcm;
        if (!is_pinned(pcm)) {
            if (int rc = e->h_in.ensure(pcm_bytes)) return rc;
            memcpy(e->h_in.p, pcm, pcm_bytes);
            src = e->h_in.p;
        }
        HIP_TRY(hipMemcpyAsync(e->d_pcm.p, src, pcm_bytes, hipMemcpyHostToDevice, e->stream));
    }
    if (int rc = alacgpu_encode_device(e, (const uint8_t*)e->d_pcm.p, total_frames, (uint8_t*)e->d_blob.p, e->d_blob.cap,
                                       (uint64_t*)e->d_off.p, 0))
        return rc;
    HIP_TRY(hipMemcpyAsync(e->h_off.p, e->d_off.p, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const uint64_t total = ((const uint64_t*)e->h_off.p)[n];
    if (total) {
        if (is_pinned(blob)) {
            HIP_TRY(hipMemcpyAsync(blob, e->d_blob.p, total, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
        } else {
            if (int rc = e->h_out.ensure(total)) return rc;
            HIP_TRY(hipMemcpyAsync(e->h_out.p, e->d_blob.p, total, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            memcpy(blob, e->h_out.p, total);
        }
    }
    memcpy(offsets, e->h_off.p, (n + 1) * sizeof(uint64_t));
    if (blob_bytes_out) *blob_bytes_out = total;
    return ALACGPU_E_OK;
}

int alacgpu_encoder_cookie(alacgpu_encoder* e, uint8_t out[24]) {
    if (!e || !out) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    EncStats s;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(&s, e->stats, sizeof(s), hipMemcpyDeviceToHost));
    const uint64_t rate = e->frames_done ? (uint64_t)((double)s.total_bytes * 8.0 * e->cfg.sample_rate / (double)e->frames_done) : 0;
    cookie(e->cfg, s.max_packet, rate > 0xffffffffull ? 0xffffffffu : (uint32_t)rate, out);
    return ALACGPU_E_OK;
}

int alacgpu_encoder_last_kernel_ms(alacgpu_encoder* e, float* ms) {
    if (!e || !ms || !e->timed) {
        set_err(!e || !ms ? "null argument" : "no encode on this handle yet");
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipEventSynchronize(e->ev1));
    HIP_TRY(hipEventElapsedTime(ms, e->ev0, e->ev1));
    return ALACGPU_E_OK;
}

void* alacgpu_encoder_stream(alacgpu_encoder* e) { return e ? (void*)e->stream : nullptr; }

int alacgpu_encoder_synchronize(alacgpu_encoder* e) {
    if (!e) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return ALACGPU_E_OK;
}

} /* extern "C" */
