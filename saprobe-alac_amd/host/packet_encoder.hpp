// packet_encoder.hpp — C++ host-side RAII twin of packet_decoder.hpp for the batch encoder of include/alacgpu.h
// (alacgpu_encoder_*; the reference is decode-only, so there is no Go counterpart to mirror).
//
//   NewPacketEncoder(config)              -> throws ErrConfig for the configs NewPacketDecoder rejects
//   PacketEncoder::Encode(pcm, frames)    interleaved LE PCM (the decoder's output format) -> dense packets + offsets
//   PacketEncoder::EncodeDevice(...)      device-resident, asynchronous on Stream()
//   PacketEncoder::PcmFromWaveformDevice / EncodeWaveformDevice   planar float32 / int32 waveforms in, on the device
//   PacketEncoder::Cookie()               24-byte ALACSpecificConfig for the encoded stream
// Header-only; link with -lalacgpu. Every encode runs the HIP kernels: there is no CPU path.
#pragma once

#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <vector>

#include "../../include/alacgpu.h"
#include "packet_decoder.hpp"

namespace alac {

struct EncodedPackets {
    std::vector<uint8_t> blob;     // packets back to back
    std::vector<uint64_t> offsets; // n + 1 entries: packet i = blob[offsets[i], offsets[i + 1])
    size_t size() const { return offsets.empty() ? 0 : offsets.size() - 1; }
};

class PacketEncoder {
public:
    PacketEncoder(const PacketConfig& config, int device = 0) : frame_length_(config.frame_length) {
        alacgpu_encoder* h = nullptr;
        const int rc = alacgpu_encoder_create(&config, device, &h);
        if (rc == ALACGPU_E_CONFIG) throw ErrConfig(alacgpu_last_error());
        if (rc != ALACGPU_E_OK) throw std::runtime_error(alacgpu_last_error());
        h_.reset(h);
    }

    // a blob capacity that always suffices for `frames` frames
    uint64_t MaxBytes(uint64_t frames) const { return alacgpu_encode_max_bytes(h_.get(), frames); }

    // pcm: `frames` interleaved frames; blocking
    EncodedPackets Encode(const uint8_t* pcm, uint64_t frames) {
        EncodedPackets r;
        const uint64_t cap = MaxBytes(frames);
        r.blob.resize(cap ? cap : 1);
        r.offsets.resize((frames + frame_length_ - 1) / frame_length_ + 1);
        uint64_t got = 0;
        if (alacgpu_encode(h_.get(), pcm, frames, r.blob.data(), cap, r.offsets.data(), &got) != ALACGPU_E_OK)
            throw std::runtime_error(alacgpu_last_error());
        r.blob.resize(got);
        return r;
    }

    // device pointers on the encoder's device; d_offsets has n + 1 entries. Asynchronous on Stream() unless sync.
    void EncodeDevice(const uint8_t* d_pcm, uint64_t frames, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offsets,
                      bool sync = false) {
        if (alacgpu_encode_device(h_.get(), d_pcm, frames, d_blob, blob_cap, d_offsets, sync ? 1 : 0) != ALACGPU_E_OK)
            throw std::runtime_error(alacgpu_last_error());
    }

    // d_wave: a planar float32 (ALACGPU_WAVE_FLOAT) or int32 (ALACGPU_WAVE_INT) waveform on the device, strides in elements
    // (ALACGPU_WAVE_STREAM [channels][channel_stride] / ALACGPU_WAVE_PACKETS [n][channels] rows) -> `frames` interleaved
    // frames of the encoder's input format at d_pcm; d_clipped (one uint64, may be null): saturated and NaN samples
    void PcmFromWaveformDevice(const void* d_wave, int layout, int type, size_t channel_stride, size_t packet_stride,
                               uint64_t frames, uint8_t* d_pcm, uint64_t* d_clipped = nullptr, bool sync = false) {
        if (alacgpu_pcm_from_waveform_device(h_.get(), d_wave, layout, type, channel_stride, packet_stride, frames, d_pcm,
                                             d_clipped, sync ? 1 : 0) != ALACGPU_E_OK)
            throw std::runtime_error(alacgpu_last_error());
    }

    // the same pass into the handle's scratch, then EncodeDevice, with no host synchronisation in between
    void EncodeWaveformDevice(const void* d_wave, int layout, int type, size_t channel_stride, size_t packet_stride,
                              uint64_t frames, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offsets,
                              uint64_t* d_clipped = nullptr, bool sync = false) {
        if (alacgpu_encode_waveform_device(h_.get(), d_wave, layout, type, channel_stride, packet_stride, frames, d_blob,
                                           blob_cap, d_offsets, d_clipped, sync ? 1 : 0) != ALACGPU_E_OK)
            throw std::runtime_error(alacgpu_last_error());
    }

    // milliseconds of the last pack pass (LastKernelMs keeps timing the encode kernels only)
    float WaveformLastMs() {
        float ms = 0;
        if (alacgpu_encoder_waveform_last_ms(h_.get(), &ms) != ALACGPU_E_OK) throw std::runtime_error(alacgpu_last_error());
        return ms;
    }

    std::array<uint8_t, 24> Cookie() {
        std::array<uint8_t, 24> c{};
        if (alacgpu_encoder_cookie(h_.get(), c.data()) != ALACGPU_E_OK) throw std::runtime_error(alacgpu_last_error());
        return c;
    }

    float LastKernelMs() {
        float ms = 0;
        if (alacgpu_encoder_last_kernel_ms(h_.get(), &ms) != ALACGPU_E_OK) throw std::runtime_error(alacgpu_last_error());
        return ms;
    }

    void* Stream() const { return alacgpu_encoder_stream(h_.get()); }
    void Synchronize() {
        if (alacgpu_encoder_synchronize(h_.get()) != ALACGPU_E_OK) throw std::runtime_error(alacgpu_last_error());
    }
    alacgpu_encoder* handle() const { return h_.get(); }

private:
    uint32_t frame_length_;
    struct Del {
        void operator()(alacgpu_encoder* e) const { alacgpu_encoder_destroy(e); }
    };
    std::unique_ptr<alacgpu_encoder, Del> h_;
};

inline std::unique_ptr<PacketEncoder> NewPacketEncoder(const PacketConfig& config, int device = 0) {
    return std::make_unique<PacketEncoder>(config, device);
}

}  // namespace alac
