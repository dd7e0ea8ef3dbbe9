/*
 * lean_ends_san_main.cpp — TEST-ONLY stand-alone program over lean_ends_sim.cpp (the host build of the decode logic with
 * ALAC_LEAN_ENDS, alac_regular.h), to be built with -fsanitize=address,undefined and run on the CPU
 * (tests/test_lean_ends_host.py does both); links saprobe-alac_amd/synth/alac_synth.c.
 *
 * It encodes a handful of 16-bit packets (stereo and mono; music, near silence, noise), and decodes every prefix of each at
 * each of the four byte misalignments out of a heap block that is dword-aligned at both ends and no longer: the promise
 * RingRd's tail fetches rely on (aligned dwords that hold a packet byte can be read), with the sanitizer watching the block's
 * ends. The bytes around the packet inside the block are 0xff. Every result must equal the one of the same prefix decoded at
 * misalignment 0 with 64 zero bytes behind it, and the whole packets must give back their source PCM.
 */
#include <cstdio>

#include "lean_ends_sim.cpp"
#include "../../saprobe-alac_amd/synth/alac_synth.h"

namespace {

struct Result {
    std::vector<uint8_t> out;
    uint32_t frames;
    int32_t status;
    uint32_t cls;
};

Result decode(const alacgpu_config& cfg, const uint8_t* block, size_t block_bytes, uint64_t off, uint32_t size, size_t stride) {
    Result r{std::vector<uint8_t>(stride + 16, 0), 0, 0, 0};
    uint8_t* out = r.out.data();
    out += (16 - (reinterpret_cast<uintptr_t>(out) & 15u)) & 15u;
    if (lane_sim_decode_batch(&cfg, block, block_bytes, &off, &size, 1, out, stride, &r.frames, &r.status, 0, -1, &r.cls, 0) != 0) {
        printf("lane_sim_decode_batch failed\n");
        exit(2);
    }
    if (out != r.out.data()) memmove(r.out.data(), out, stride);
    r.out.resize(stride);
    return r;
}

}  // namespace

int main() {
    int bad = 0;
    size_t decodes = 0, regular = 0;
    for (int ch = 2; ch >= 1; --ch) {
        alacgpu_config cfg{};
        cfg.frame_length = 96;
        cfg.bit_depth = 16;
        cfg.num_channels = (uint8_t)ch;
        cfg.pb = 40;
        cfg.mb = 10;
        cfg.kb = 14;
        cfg.max_run = 255;
        const size_t bpf = (size_t)ch * 2u, stride = (96 * bpf + 15) / 16 * 16;
        const struct { int profile; uint32_t frames; uint8_t order; } kinds[] = {
            {ALAC_SYNTH_PROFILE_MUSIC, 96, 4}, {ALAC_SYNTH_PROFILE_QUIET, 96, 4}, {ALAC_SYNTH_PROFILE_NOISE, 40, 0},
            {ALAC_SYNTH_PROFILE_MUSIC, 89, 12}, {ALAC_SYNTH_PROFILE_QUIET, 41, 0}};
        for (size_t k = 0; k < sizeof(kinds) / sizeof(kinds[0]); ++k) {
            std::vector<int32_t> pcm((size_t)96 * ch);
            alac_synth_signal(&cfg, kinds[k].profile, 1000 + k, kinds[k].frames, pcm.data());
            alac_synth_elem e{};
            e.order_u = e.order_v = kinds[k].order;
            e.den_shift = 9;
            e.pb_factor = 4;
            e.mix_bits = 2;
            e.mix_res = (int8_t)(k % 2);
            e.never_escape = 1;
            std::vector<uint8_t> pkt(4096);
            const size_t len = alac_synth_encode_packet(&cfg, &e, pcm.data(), kinds[k].frames, 0, pkt.data(), pkt.size());
            if (len == 0) {
                printf("encoder failed for kind %zu\n", k);
                return 2;
            }
            std::vector<uint8_t> src(kinds[k].frames * bpf);
            alac_synth_pack_pcm(&cfg, pcm.data(), kinds[k].frames, src.data());
            for (size_t cut = 0; cut <= len; ++cut) {
                std::vector<uint8_t> padded(cut + 64, 0);
                memcpy(padded.data(), pkt.data(), cut);
                const Result want = decode(cfg, padded.data(), padded.size(), 0, (uint32_t)cut, stride);
                regular += want.cls < 2048u;
                if (cut == len && (want.status != 0 || want.frames != kinds[k].frames || memcmp(want.out.data(), src.data(), src.size()) != 0)) {
                    printf("%d ch kind %zu: the whole packet does not give back its source (status %#x, %u frames)\n", ch, k, want.status, want.frames);
                    ++bad;
                }
                for (size_t mis = 0; mis < 4; ++mis) {
                    const size_t bytes = (mis + cut + 3u) & ~(size_t)3u;
                    uint8_t* block = (uint8_t*)malloc(bytes ? bytes : 4u); /* 16-byte aligned: dword-aligned at both ends */
                    memset(block, 0xff, bytes ? bytes : 4u);
                    memcpy(block + mis, pkt.data(), cut);
                    const Result got = decode(cfg, block, bytes, mis, (uint32_t)cut, stride);
                    free(block);
                    ++decodes;
                    const size_t nb = want.frames * bpf;
                    if (got.status != want.status || got.frames != want.frames || memcmp(got.out.data(), want.out.data(), nb) != 0) {
                        if (bad < 10)
                            printf("%d ch kind %zu prefix %zu of %zu at misalignment %zu: status %#x / %#x, frames %u / %u\n", ch, k, cut, len,
                                   mis, got.status, want.status, got.frames, want.frames);
                        ++bad;
                    }
                }
            }
        }
    }
    printf("lean ends: %zu decodes, %zu prefixes on the lean path, %d differ, switch %u\n", decodes, regular, bad, lean_ends_sim_switch());
    return bad ? 1 : 0;
}
