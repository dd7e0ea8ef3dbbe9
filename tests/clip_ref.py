"""TEST HELPER for the clip gather (alacgpu_clips_device): the numpy restatement every comparison uses, the expected image
of a whole clips buffer, sentinel included, the host build of csrc/alac_clips.h (tests/host_sim/clip_sim.cpp), and the packet
lists and files the GPU tests decode.

The restatement imports nothing of the code under test. It starts from decoded slots (out[n, stride] uint8, frames, status
— the oracle's triple, or slots a test wrote by hand) and follows the definition in include/alacgpu.h with Python integers,
so that no descriptor wraps around: slot i is the frames [i * fl, (i + 1) * fl) of a grid; column t of clip j is grid frame
begin[j] + t, a sample when that does not overflow, its slot lies below min(limit[j], n) and its frame below the slot's f,
zero otherwise. Samples are unpacked and converted by tests/wave_ref.py. All comparisons are bit-exact."""
import ctypes
import os
import subprocess

import numpy as np

from tests import wave_ref as wr

ROOT = wr.ROOT
SIM_DIR = wr.SIM_DIR
SENTINEL = wr.SENTINEL


def ref_clips(out, frames, status, fl, depth, ch, wtype, begin, limit, L):
    """-> (clips uint32 [B, ch, L], valid uint32 [B], clip_status int32 [B])"""
    n = len(frames)
    f = [int(x) for x in wr.frames_used(frames, status, fl)] if n else []
    B = len(begin)
    clips = np.zeros((B, ch, L), np.uint32)
    valid = np.zeros(B, np.uint32)
    cstat = np.zeros(B, np.int32)
    cache = {}
    for j in range(B):
        b, lim = int(begin[j]), min(int(limit[j]), n)
        t = 0
        while t < L:
            g = b + t
            if g >= 1 << 64:
                break  # overflow: this column and all behind it
            i, r = divmod(g, fl)
            if i >= lim:
                break  # slots grow with t: nothing behind this column either
            take = min(fl - r, L - t, (1 << 64) - g)  # columns of this clip in slot i
            if status is not None and cstat[j] == 0 and int(status[i]) != 0:
                cstat[j] = status[i]
            have = max(0, min(f[i], r + take) - r)
            if have:
                if i not in cache:
                    cache[i] = wr.elements(wr.unpack(out[i], f[i], depth, ch), depth, wtype)
                clips[j, :, t:t + have] = cache[i][r:r + have].T
                valid[j] += have
            t += take
    return clips, valid, cstat


def expected_image(ref, elems, base, cs, ps):
    """The whole clips buffer (`elems` uint32 elements, the tensor starting at element `base`, rows cs apart, clips ps apart)
    as the gather must leave it when it was filled with SENTINEL before: the [B][ch] rows at their place, the sentinel
    everywhere else."""
    img = np.full(elems, SENTINEL, np.uint32)
    B, ch, L = ref.shape
    for j in range(B):
        for c in range(ch):
            o = base + j * ps + c * cs
            img[o:o + L] = ref[j, c]
    return img


def build_clip_sim():
    so = os.path.join(SIM_DIR, "libclip_sim.so")
    csrc = os.path.join(ROOT, "saprobe-alac_amd", "csrc")
    srcs = [os.path.join(SIM_DIR, "clip_sim.cpp"), os.path.join(csrc, "alac_clips.h"), os.path.join(csrc, "alac_waveform.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-fwrapv", "-fPIC", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-shared", "-o", so,
                               srcs[0]])
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.clip_sim_run.argtypes = [u32, u32, u32, vp, u64, vp, vp, u64, vp, vp, u64, u32, ctypes.c_int, vp, u64, u64, vp, vp, u64]
    for fn in (L.clip_sim_tile_cols, L.clip_sim_stage_need):
        fn.restype, fn.argtypes = u32, [u32, u32, u32]
    L.clip_sim_stage_bytes.restype = u32
    return L


# ---- packets and files for the GPU tests ---------------------------------------------------------------------------------
SHIFT = {16: 0, 20: 0, 24: 1, 32: 2}


def to_pkg_cfg(pkg, ocfg):
    return pkg.PacketConfig(FrameLength=ocfg.frame_length, BitDepth=ocfg.bit_depth, NumChannels=ocfg.num_channels,
                            PB=ocfg.pb, MB=ocfg.mb, KB=ocfg.kb, MaxRun=ocfg.max_run, SampleRate=ocfg.sample_rate)


def short_packet(synth, cfg, frames, seed, escape):
    ne = synth.num_elements(cfg.num_channels)
    kw = dict(force_escape=1) if escape else dict(never_escape=1, bytes_shifted=SHIFT[cfg.bit_depth])
    pcm = synth.signal(cfg, synth.PROFILE_MUSIC, seed, frames)
    return synth.encode_packet(cfg, [synth.default_elem(**kw) for _ in range(ne)], pcm)


def extreme_packet(synth, cfg):
    """One escaped packet whose samples are the depth's extremes in the PCM domain (a 20-bit sample comes out left-aligned in
    its three bytes), every channel starting at another one."""
    ex = np.array([-(1 << 19), (1 << 19) - 1, -1, 0, 1], np.int64) if cfg.bit_depth == 20 else wr.extremes(cfg.bit_depth)
    fl, ch = cfg.frame_length, cfg.num_channels
    pcm = np.stack([np.resize(np.roll(ex, c), fl) for c in range(ch)], axis=1).astype(np.int32)
    return synth.encode_packet(cfg, [synth.default_elem(force_escape=1) for _ in range(synth.num_elements(ch))], pcm)


def packet_list(synth, helpers, cfg, n, seed, damaged=0):
    """A synth batch with the extremes packet, short packets at the start, in the middle and at the end, and `damaged`
    mutated packets (helpers.mutate_packets: data errors the decoder reports as status) mixed in."""
    fl = cfg.frame_length
    b = synth.gen_batch(cfg, n, base_seed=seed, threads=8)
    rng = np.random.default_rng(seed)
    packets = [b.packet(i) for i in range(b.n)] + helpers.mutate_packets(b, rng, damaged)
    rng.shuffle(packets)
    packets.insert(len(packets) // 3, extreme_packet(synth, cfg))
    if fl > 1:
        for at, k, esc in ((0, 1, True), (len(packets) // 2, fl // 2 + 1, False), (len(packets) // 2, 3, True),
                           (len(packets), fl - 1, False), (len(packets), max(fl - 3, 1), True)):
            if 1 <= k < fl:
                packets.insert(at, short_packet(synth, cfg, k, seed + k, esc or fl < 16))
    return packets


class Batch:
    """Packets on the device and the oracle's decode of them."""

    def __init__(self, torch, oracle, helpers, cfg, packets):
        self.cfg, self.n = cfg, len(packets)
        blob, offs, sizes = helpers.pack_packets(packets)
        self.ref = oracle.decode_batch(cfg, blob, offs, sizes, threads=8)
        dev = torch.device("cuda:0")
        self.d_blob = torch.from_numpy(blob).to(dev)
        self.d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
        self.d_sz = torch.from_numpy(sizes.astype(np.int32)).to(dev)


def file_packets(oracle, synth, cfg, n, seed, last=None):
    """n full packets and a short last one, as an encoder writes a file (synth's batches have short packets of their own
    here and there: those are left out)."""
    b = synth.gen_batch(cfg, n + 8, base_seed=seed, threads=8)
    frames = oracle.decode_batch(cfg, b.blob, b.offsets, b.sizes, threads=8, want_output=False)[1]
    packets = [b.packet(i) for i in range(b.n) if frames[i] == cfg.frame_length][:n]
    assert len(packets) == n
    return packets + [short_packet(synth, cfg, last or cfg.frame_length // 3 + 1, seed, escape=False)]
