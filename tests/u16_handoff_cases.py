"""Packet sets for the half-word U hand-off and the whole-chunk writer of 16-bit pairs (alac_duo.h): shared by
tests/test_gpu_u16_handoff.py (the kernels) and tests/test_u16_handoff_host.py (the same text built for the host).

Every generator returns a list of packets (bytes) of one 16-bit stereo configuration; what they should decode to comes
from the oracle. The sets are small (64-512 packets): the GPU tests run them with full wave slots (ALACGPU_PPW=64), so
that the lanes of one workgroup hold the mixture each set is about."""
import numpy as np

COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 4095, 4096)   # frames per packet; the writer's chunk is 8 steps, the tile row 2
MIXES = [(res, sh) for res in (0, 1, 2, -1) for sh in (0, 1, 2)]  # mixRes (int8: 255 is -1), mixBits


def _elem(synth, order, mix_res=1, mix_bits=2, **kw):
    return synth.default_elem(order=order, mix_res=mix_res, mix_bits=mix_bits, never_escape=1, **kw)


def antiphase_pcm(cfg, rng, frames, loud=True):
    """L near full scale (a slow sine that crosses both rails' neighbourhood, plus noise), R = -L - 1: v = L - R needs 17
    bits, and with mixRes 2 / mixBits 0 so does u."""
    top = 1 << 15
    t = np.arange(frames)
    amp = (top - 40) if loud else top // 64
    left = (amp * np.sin(t / 9.0 + rng.uniform(0, 6.28))).astype(np.int64) + rng.integers(-30, 31, size=frames)
    left = np.clip(left, -top, top - 1)
    right = np.clip(-left - 1, -top, top - 1)
    return np.ascontiguousarray(np.stack([left, right], axis=1), dtype=np.int32)


def antiphase_set(synth, cfg, order=4, per_mix=10, seed=7):
    """per_mix loud anti-phase packets for every (mixRes, mixBits) of MIXES and a few quiet ones, shuffled: one key, so the
    matrixed lanes and the mixRes 0 lanes share their workgroups."""
    rng = np.random.default_rng(seed)
    fl = cfg.frame_length
    out = []
    for res, sh in MIXES:
        for k in range(per_mix):
            out.append(synth.encode_packet(cfg, [_elem(synth, order, res, sh)], antiphase_pcm(cfg, rng, fl, loud=k != 0)))
    while len(out) % 64:
        out.append(synth.encode_packet(cfg, [_elem(synth, order)], antiphase_pcm(cfg, rng, fl, loud=False)))
    return [out[i] for i in rng.permutation(len(out))]


def u_samples(pcm_bytes, frames, mix_res, mix_bits):
    """The U channel the decoder reconstructs for a matrixed pair (matrix.go:40-41 inverted), as chanBits = 17 bit values."""
    s = np.frombuffer(pcm_bytes[:frames * 4], "<i2").astype(np.int64).reshape(-1, 2)
    v = s[:, 0] - s[:, 1]
    u = s[:, 1] + ((mix_res * v) >> mix_bits)
    return ((u + (1 << 16)) % (1 << 17)) - (1 << 16)


def mixed_matrix_set(synth, cfg, order=6, n=128, seed=11):
    """Lanes with mixRes 0 beside matrixed lanes, alternating: the key is the orders only."""
    rng = np.random.default_rng(seed)
    fl = cfg.frame_length
    return [synth.encode_packet(cfg, [_elem(synth, order, 0 if i % 3 == 0 else 1 + i % 2, i % 3)],
                                antiphase_pcm(cfg, rng, fl, loud=i % 5 != 0)) for i in range(n)]


def frame_count_set(synth, cfg, order=4, n=128, seed=13):
    """Short and full packets side by side: every count of COUNTS that fits the frame length, frame_length - 1 and the
    frame length itself, both matrixed and not."""
    rng = np.random.default_rng(seed)
    fl = cfg.frame_length
    counts = sorted({k for k in COUNTS + (fl - 1, fl) if 1 <= k <= fl})
    out = []
    for i in range(n):
        k = counts[(i // 2) % len(counts)] if i % 2 else fl
        out.append(synth.encode_packet(cfg, [_elem(synth, order, i % 3, 2)], antiphase_pcm(cfg, rng, fl, loud=i % 4 != 0)[:k]))
    return [out[i] for i in rng.permutation(len(out))]


def all_short_set(synth, cfg, order=4, n=64, seed=17):
    """No full packet at all: the workgroup's step count is the longest short packet's (an odd one: the lone last U store)."""
    rng = np.random.default_rng(seed)
    fl = cfg.frame_length
    counts = [k for k in (1, 2, 7, 8, 9, 15, 16, 17, 33, 41) if k < fl]
    return [synth.encode_packet(cfg, [_elem(synth, order, i % 2, 1)], antiphase_pcm(cfg, rng, fl)[:counts[i % len(counts)]])
            for i in range(n)]


def damaged_set(synth, cfg, order=4, n=64, seed=19):
    """Good packets and, among them, packets cut off inside V (the last quarter of their bytes gone)."""
    rng = np.random.default_rng(seed)
    fl = cfg.frame_length
    out = []
    for i in range(n):
        p = synth.encode_packet(cfg, [_elem(synth, order, 1, 2)], antiphase_pcm(cfg, rng, fl, loud=i % 2 == 0))
        if i % 9 == 4:
            p = p[:len(p) - len(p) // 4]
        out.append(p)
    return out
