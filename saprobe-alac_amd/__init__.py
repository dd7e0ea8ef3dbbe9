"""saprobe-alac_amd — MI355X (gfx950) batch ALAC packet decoder.

Host-side mirror of the reference's packet layer (mycophonic/saprobe-alac, root package `alac`)
over the C ABI of include/alacgpu.h:

    reference (Go)                                   here
    ------------------------------------------------ ----------------------------------
    PacketConfig             config.go:27-38          PacketConfig
    PCMFormat                format.go:20-24          PCMFormat
    NewPacketDecoder         decoder.go:90            NewPacketDecoder / PacketDecoder(...)
    (*PacketDecoder).Format  decoder.go:112           PacketDecoder.Format()
    (*PacketDecoder).DecodePacket  decoder.go:117     PacketDecoder.DecodePacket(packet) -> bytes
    DecodePackets (new batch entry, north star)       PacketDecoder.DecodePackets(packets)
    ErrConfig / ErrDecode    errors.go:22-34          ErrConfig / ErrDecode (+ .sentinel)
    internal sentinels       internal/alac/errors.go  ErrBitstreamOverrun, ErrSampleOverrun, ...

The reference is Go; this image has no Go toolchain, so the host side above the C ABI is Python
(ctypes) for the tests/bench and C++ (host/packet_decoder.hpp) for native callers; INTEGRATION.md
shows the cgo binding. Every decode call runs the HIP kernels in csrc/: there is no CPU decode
path, and loading fails loudly when libalacgpu.so is missing.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_LIB = None

__all__ = [
    "PacketConfig", "PCMFormat", "PacketDecoder", "NewPacketDecoder", "PacketEncoder", "NewPacketEncoder", "ParseMagicCookie",
    "ErrConfig", "ErrDecode", "AlacError", "build", "lib", "lib_path", "trim", "load", "save",
    "load_clips", "Resampler", "NewResampler", "resample",
    "MelSpectrogram", "NewMelSpectrogram", "mel_spectrogram", "spectrogram", "whisper_log_mel",
    "KaldiFeatures", "NewKaldiFeatures", "kaldi_fbank", "kaldi_mfcc",
    "NormConfig", "FeatureNorm", "NewFeatureNorm", "normalize_features", "kaldi_frame_counts", "load_features",
    "StackConfig", "StackInfo", "FrameStack", "NewFrameStack", "stack_frames", "add_deltas", "lfr",
    "SpecAugConfig", "SpecAugInfo", "SpecAugment", "NewSpecAugment", "spec_augment",
    "WaveAugConfig", "WaveAugInfo", "WaveAugment", "NewWaveAugment", "augment_waveform",
]

PACKET_PAD = 0  # ALACGPU_PACKET_PAD: blobs are dense since 0.3.0
WAVE_STREAM, WAVE_PACKETS = 0, 1  # alacgpu_wave_layout
WAVE_FLOAT, WAVE_INT = 0, 1  # alacgpu_wave_type


def trim():
    """alacgpu_trim(): free what destroyed decoders left in the per-process handle pool (see PacketDecoder.close)."""
    lib().alacgpu_trim()


# ---- errors: errors.go:22-34 and internal/alac/errors.go:24-33 -------------------------------------
class AlacError(Exception):
    """Base of the package's errors; `sentinel` names the wrapped internal sentinel (errors.Is target)."""

    sentinel = None


class ErrConfig(AlacError):
    """errors.go:25 — invalid or unsupported configuration."""


class ErrDecode(AlacError):
    """errors.go:33 — failure during packet decoding; .status is the C ABI status word."""

    def __init__(self, msg, status=0, sentinel=None):
        super().__init__(msg)
        self.status = status
        self.sentinel = sentinel


class HipError(RuntimeError):
    """The HIP runtime or the extension failed (no reference counterpart)."""


ErrInvalidCookie = "alac: invalid magic cookie"
ErrUnsupportedVersion = "alac: unsupported compatible version"
ErrUnsupportedElement = "alac: unsupported element type (CCE/PCE)"
ErrInvalidHeader = "alac: invalid frame header"
ErrInvalidShift = "alac: invalid bytesShifted value"
ErrBitstreamOverrun = "alac: bitstream overrun"
ErrSampleOverrun = "alac: sample count exceeds buffer"
ErrBitDepth = "alac: unsupported bit depth"
ErrMalformed = "alac: malformed packet (the reference panics)"
ErrRange = "alac: packet outside the blob"

_CODE_SENTINEL = {1: ErrBitstreamOverrun, 2: ErrSampleOverrun, 3: ErrInvalidHeader, 4: ErrInvalidShift,
                  5: ErrUnsupportedElement, 6: ErrMalformed, 7: ErrRange}
_CTX = {0: None, 1: "SCE/LFE", 2: "CPE", 3: "DSE", 4: "FIL"}
_STAGE = {0: None, 1: "entropy decode", 2: "entropy decode U", 3: "entropy decode V"}


def status_error(status):
    """Rebuild the reference's error chain text from a status word (decoder.go:144-189,303,468,482)."""
    code, ctx, stage = status & 0xff, (status >> 8) & 0xf, (status >> 12) & 0x3
    parts = ["decode failed"]
    if _CTX.get(ctx):
        parts.append(_CTX[ctx])
    if _STAGE.get(stage):
        parts.append(_STAGE[stage])
    sentinel = _CODE_SENTINEL.get(code, "alac: unknown status %d" % code)
    parts.append(sentinel)
    return ErrDecode(": ".join(parts), status=status, sentinel=sentinel)


# ---- data contract ------------------------------------------------------------------------------------
class PacketConfig(ctypes.Structure):
    """PacketConfig (config.go:27-38) as the POD alacgpu_config."""

    _fields_ = [
        ("FrameLength", ctypes.c_uint32),
        ("BitDepth", ctypes.c_uint8),
        ("NumChannels", ctypes.c_uint8),
        ("PB", ctypes.c_uint8),
        ("MB", ctypes.c_uint8),
        ("KB", ctypes.c_uint8),
        ("_reserved0", ctypes.c_uint8),
        ("MaxRun", ctypes.c_uint16),
        ("MaxFrameBytes", ctypes.c_uint32),
        ("AvgBitRate", ctypes.c_uint32),
        ("SampleRate", ctypes.c_uint32),
    ]

    def __init__(self, FrameLength=4096, BitDepth=16, NumChannels=2, PB=40, MB=10, KB=14, MaxRun=255,
                 MaxFrameBytes=0, AvgBitRate=0, SampleRate=44100):
        super().__init__(FrameLength, BitDepth, NumChannels, PB, MB, KB, 0, MaxRun, MaxFrameBytes, AvgBitRate,
                         SampleRate)

    # C-side field names (alacgpu_config) as read-only aliases
    frame_length = property(lambda s: s.FrameLength)
    bit_depth = property(lambda s: s.BitDepth)
    num_channels = property(lambda s: s.NumChannels)
    pb = property(lambda s: s.PB)
    mb = property(lambda s: s.MB)
    kb = property(lambda s: s.KB)
    max_run = property(lambda s: s.MaxRun)
    max_frame_bytes = property(lambda s: s.MaxFrameBytes)
    avg_bit_rate = property(lambda s: s.AvgBitRate)
    sample_rate = property(lambda s: s.SampleRate)


class PCMFormat(ctypes.Structure):
    """PCMFormat (format.go:20-24)."""

    _fields_ = [("SampleRate", ctypes.c_int32), ("BitDepth", ctypes.c_int32), ("Channels", ctypes.c_int32)]

    def __repr__(self):
        return "PCMFormat(SampleRate=%d, BitDepth=%d, Channels=%d)" % (self.SampleRate, self.BitDepth, self.Channels)


def ParseMagicCookie(cookie):
    """ParseMagicCookie (config.go:47-81): 24-byte ALACSpecificConfig, optional 'frma'/'alac' wrappers."""
    data = bytes(cookie or b"")
    if len(data) >= 12 and data[4:8] == b"frma":
        data = data[12:]
    if len(data) >= 12 and data[4:8] == b"alac":
        data = data[12:]
    if len(data) < 24:
        e = ErrConfig("invalid configuration: " + ErrInvalidCookie)
        e.sentinel = ErrInvalidCookie
        raise e
    if data[4] > 0:
        e = ErrConfig("invalid configuration: %s: %d" % (ErrUnsupportedVersion, data[4]))
        e.sentinel = ErrUnsupportedVersion
        raise e
    be = lambda b: int.from_bytes(b, "big")  # noqa: E731
    return PacketConfig(FrameLength=be(data[0:4]), BitDepth=data[5], PB=data[6], MB=data[7], KB=data[8],
                        NumChannels=data[9], MaxRun=be(data[10:12]), MaxFrameBytes=be(data[12:16]),
                        AvgBitRate=be(data[16:20]), SampleRate=be(data[20:24]))


# ---- native library --------------------------------------------------------------------------------------
def lib_path():
    # ALACGPU_LIB: another build of the same library (kernel A/B experiments under profiles/)
    return os.environ.get("ALACGPU_LIB") or os.path.join(_CSRC, "libalacgpu.so")


def build(force=False):
    """Compile the translation units of csrc/ for gfx950 (hipcc cross-compiles without a GPU) and link libalacgpu.so."""
    so = lib_path()
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h", ".inc"))] + [
        os.path.join(_HERE, "..", "include", "alacgpu.h")]
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        jobs = str(max(1, min(6, os.cpu_count() or 1)))
        subprocess.check_call(["make", "-C", _CSRC, "-j", jobs, "libalacgpu.so"], stdout=subprocess.DEVNULL)
    return so


def csrc_sha256():
    """Fingerprint of the kernel sources (csrc/*.hip, *.h, *.inc): profiles/*/traffic.json is stamped with it."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(os.listdir(_CSRC)):
        if f.endswith((".hip", ".h", ".inc")):
            h.update(f.encode())
            h.update(open(os.path.join(_CSRC, f), "rb").read())
    return h.hexdigest()


class Dispatch(ctypes.Structure):
    """alacgpu_dispatch (include/alacgpu.h)."""

    _fields_ = [("packets_per_slot", ctypes.c_uint32), ("slots", ctypes.c_uint32), ("irregular_slots", ctypes.c_uint32),
                ("wide_slots", ctypes.c_uint32), ("narrow_slots", ctypes.c_uint32), ("keys", ctypes.c_uint32),
                ("gated", ctypes.c_uint32), ("lanes_per_packet", ctypes.c_uint32), ("narrow_kernel", ctypes.c_char * 32),
                ("wide_kernel", ctypes.c_char * 32), ("irregular_kernels", ctypes.c_char * 96), ("workgroups_per_cu", ctypes.c_uint32)]


_EXPORTS = {
    "alacgpu_create": (ctypes.c_int, [ctypes.POINTER(PacketConfig), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "alacgpu_destroy": (None, [ctypes.c_void_p]),
    "alacgpu_trim": (None, []),
    "alacgpu_host_alloc": (ctypes.c_void_p, [ctypes.c_size_t]),
    "alacgpu_host_free": (None, [ctypes.c_void_p]),
    "alacgpu_last_dispatch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "alacgpu_get_format": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(PCMFormat)]),
    "alacgpu_frame_bytes": (ctypes.c_size_t, [ctypes.c_void_p]),
    "alacgpu_decode_packet": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                             ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                             ctypes.POINTER(ctypes.c_int32)]),
    "alacgpu_decode_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_void_p]),
    "alacgpu_decode_batch_start": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                  ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                  ctypes.c_void_p]),
    "alacgpu_decode_batch_wait": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_decode_batch_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "alacgpu_reserve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t]),
    "alacgpu_last_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_timing_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_kernel_times": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.POINTER(ctypes.c_size_t)]),
    "alacgpu_pair_placement": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.POINTER(ctypes.c_size_t)]),
    "alacgpu_waveform_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                               ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]),
    "alacgpu_waveform_last_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_clips_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int]),
    "alacgpu_clips_last_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "alacgpu_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_encoder_create": (ctypes.c_int, [ctypes.POINTER(PacketConfig), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "alacgpu_encoder_destroy": (None, [ctypes.c_void_p]),
    "alacgpu_encode_max_bytes": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64]),
    "alacgpu_encode_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                             ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]),
    "alacgpu_pcm_from_waveform_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_int]),
    "alacgpu_encode_waveform_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_void_p,
                                                      ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "alacgpu_encoder_waveform_last_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "alacgpu_encoder_cookie": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "alacgpu_encoder_last_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_encoder_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "alacgpu_encoder_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_resampler_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double,
                                                ctypes.POINTER(ctypes.c_void_p)]),
    "alacgpu_resampler_destroy": (None, [ctypes.c_void_p]),
    "alacgpu_resampler_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "alacgpu_resampler_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_resampler_last_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_resample_out_frames": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64]),
    "alacgpu_resample_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                               ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]),
    "alacgpu_resampler_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                              ctypes.c_size_t]),
    "alacgpu_mel_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "alacgpu_mel_destroy": (None, [ctypes.c_void_p]),
    "alacgpu_mel_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "alacgpu_mel_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_mel_last_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_mel_out_frames": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64]),
    "alacgpu_mel_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                          ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]),
    "alacgpu_mel_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                        ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]),
    "alacgpu_mel_fft_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_size_t]),
    "alacgpu_fbank_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "alacgpu_fbank_create_transform": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]),
    "alacgpu_fbank_destroy": (None, [ctypes.c_void_p]),
    "alacgpu_fbank_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "alacgpu_fbank_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_fbank_last_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_fbank_out_frames": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64]),
    "alacgpu_fbank_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                            ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]),
    "alacgpu_fbank_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                          ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p, ctypes.c_size_t]),
    "alacgpu_fbank_fft_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                              ctypes.c_size_t]),
    "alacgpu_norm_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.POINTER(ctypes.c_void_p)]),
    "alacgpu_norm_destroy": (None, [ctypes.c_void_p]),
    "alacgpu_norm_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "alacgpu_norm_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_norm_last_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_norm_out_frames": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64]),
    "alacgpu_norm_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                           ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                           ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]),
    "alacgpu_norm_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                         ctypes.c_size_t]),
    "alacgpu_stack_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "alacgpu_stack_destroy": (None, [ctypes.c_void_p]),
    "alacgpu_stack_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "alacgpu_stack_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_stack_last_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_stack_out_frames": (ctypes.c_uint64, [ctypes.c_void_p, ctypes.c_uint64]),
    "alacgpu_stack_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                            ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]),
    "alacgpu_stack_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "alacgpu_specaug_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "alacgpu_specaug_destroy": (None, [ctypes.c_void_p]),
    "alacgpu_specaug_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "alacgpu_specaug_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_specaug_last_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_specaug_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.c_void_p, ctypes.c_int]),
    "alacgpu_specaug_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "alacgpu_waveaug_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "alacgpu_waveaug_destroy": (None, [ctypes.c_void_p]),
    "alacgpu_waveaug_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "alacgpu_waveaug_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "alacgpu_waveaug_last_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "alacgpu_waveaug_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "alacgpu_waveaug_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                            ctypes.c_size_t]),
    "alacgpu_last_error": (ctypes.c_char_p, []),
    "alacgpu_version": (ctypes.c_char_p, []),
}


def lib():
    """Load libalacgpu.so. Raises if the HIP extension has not been built: there is no fallback."""
    global _LIB
    if _LIB is None:
        so = lib_path()
        if not os.path.exists(so):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); this package has no CPU decode path" % so)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same SONAME as
        # /opt/rocm's). If torch is going to be used in this process it must be loaded FIRST so that
        # libalacgpu.so binds to the runtime torch initialises; loaded the other way round the process
        # ends up with two runtimes and torch.cuda.is_available() turns False. The library only needs
        # the stable hip_4.2 symbol set, so either runtime serves it.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(so)
        for name, (res, args) in _EXPORTS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _LIB = L
    return _LIB


def _check(rc):
    if rc == 0:
        return
    msg = (lib().alacgpu_last_error() or b"").decode("utf-8", "replace")
    if rc == -1:
        e = ErrConfig(msg or "invalid configuration")
        e.sentinel = ErrBitDepth if "bit depth" in msg else None
        raise e
    if rc == -2:
        raise ValueError(msg or "bad argument")
    raise HipError(msg or "HIP failure %d" % rc)


def bytes_per_sample(depth):
    """BytesPerSample (internal/alac/format.go:23-34)."""
    try:
        return {16: 2, 20: 3, 24: 3, 32: 4}[depth]
    except KeyError:
        raise ValueError("alac: BytesPerSample called with unsupported bit depth %d" % depth)


# ---- PacketDecoder (decoder.go:79-128) ------------------------------------------------------------------
class PacketDecoder:
    """Decodes ALAC packets into interleaved LE signed PCM on one MI355X (decoder.go:79).

    Like the reference's, a PacketDecoder is single-caller. It is bound to one HIP device and one
    stream; multi-GPU callers make one decoder per device (see parallel.py).
    """

    def __init__(self, config, device=0):
        self._h = ctypes.c_void_p()
        self._lib = lib()
        self.config = config
        _check(self._lib.alacgpu_create(ctypes.byref(config), device, ctypes.byref(self._h)))
        self.device = device
        self.frame_bytes = self._lib.alacgpu_frame_bytes(self._h)

    def close(self):
        """alacgpu_destroy: the handle's streams, events and small buffers go to a per-process pool for the next decoder on
        this device (at most 128 MB of device memory and 64 MB of pinned memory per pooled handle, four per device);
        trim() gives that back too."""
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.alacgpu_destroy(self._h)
            self._h = ctypes.c_void_p()

    @staticmethod
    def trim():
        """alacgpu_trim: free what destroyed handles left in the pool (every device)."""
        lib().alacgpu_trim()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def Format(self):
        """(*PacketDecoder).Format (decoder.go:112)."""
        f = PCMFormat()
        _check(self._lib.alacgpu_get_format(self._h, ctypes.byref(f)))
        return f

    def DecodePacket(self, packet):
        """(*PacketDecoder).DecodePacket (decoder.go:117): one packet -> PCM bytes; raises ErrDecode."""
        packet = bytes(packet)
        out = np.empty(max(self.frame_bytes, 1), dtype=np.uint8)
        n = ctypes.c_size_t()
        st = ctypes.c_int32()
        buf = np.frombuffer(packet, dtype=np.uint8) if packet else np.zeros(1, np.uint8)
        rc = self._lib.alacgpu_decode_packet(self._h, buf.ctypes.data, len(packet), out.ctypes.data, out.size,
                                             ctypes.byref(n), ctypes.byref(st))
        if rc == -4:
            raise status_error(st.value)
        _check(rc)
        return out[:n.value].tobytes()

    def DecodePackets(self, packets):
        """New batch entry: list of packets -> (list of PCM bytes or ErrDecode per packet)."""
        packets = [bytes(p) for p in packets]
        n = len(packets)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        if n:
            offsets[1:] = np.cumsum([len(p) for p in packets], dtype=np.uint64)
        blob = np.frombuffer(b"".join(packets) or b"\0", dtype=np.uint8)
        out, frames, status = self.decode_batch(blob, offsets)
        bpf = self.config.NumChannels * bytes_per_sample(self.config.BitDepth)
        res = []
        for i in range(n):
            res.append(status_error(int(status[i])) if status[i] else out[i, :int(frames[i]) * bpf].tobytes())
        return res

    def decode_batch(self, blob, offsets, out_stride=None):
        """alacgpu_decode_batch: host blob + offsets[n+1] -> (out[n, stride] uint8, frames, status). The offsets may
        come from an untrusted sample table: packets that leave the blob get ALACGPU_ERR_RANGE and are never read."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        stride = out_stride or self.frame_bytes
        # (empty, not zeros: the entry itself zeroes failing packets' slots and the bytes behind partial frames, and touching
        # 50 MB twice is a third of a long file's decode time)
        out = np.empty((max(n, 0), stride), dtype=np.uint8)
        frames = np.zeros(max(n, 0), dtype=np.uint32)
        status = np.zeros(max(n, 0), dtype=np.int32)
        if n > 0:
            _check(self._lib.alacgpu_decode_batch(self._h, blob.ctypes.data, blob.size, offsets.ctypes.data, n,
                                                  out.ctypes.data, stride, frames.ctypes.data, status.ctypes.data))
        return out, frames, status

    def decode_batch_start(self, blob, offsets, out_stride=None):
        """alacgpu_decode_batch_start: the same decode on a thread of the library's own (no Python thread, no GIL to fight
        for). -> a token for decode_batch_wait; nothing else may be called on this decoder until then."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        stride = out_stride or self.frame_bytes
        out = np.empty((max(n, 0), stride), dtype=np.uint8)
        frames = np.zeros(max(n, 0), dtype=np.uint32)
        status = np.zeros(max(n, 0), dtype=np.int32)
        if n > 0:
            _check(self._lib.alacgpu_decode_batch_start(self._h, blob.ctypes.data, blob.size, offsets.ctypes.data, n,
                                                        out.ctypes.data, stride, frames.ctypes.data, status.ctypes.data))
        return (blob, offsets, out, frames, status, n > 0)  # the token keeps every buffer alive

    def decode_batch_wait(self, token):
        """-> (out, frames, status) of the decode decode_batch_start began; raises what decode_batch would have."""
        if token[5]:
            _check(self._lib.alacgpu_decode_batch_wait(self._h))
        return token[2], token[3], token[4]

    def decode_batch_device(self, d_blob, blob_bytes, d_offsets, d_sizes, n, d_out, out_stride, d_frames, d_status,
                            sync=True):
        """alacgpu_decode_batch_device: raw device pointers (ints), e.g. torch tensors' data_ptr(); blob_bytes =
        readable bytes at d_blob (packets may lie densely); d_sizes may be None (offsets then has n+1 entries).
        The handle's stream does not order against torch's: synchronize the inputs first."""
        _check(self._lib.alacgpu_decode_batch_device(self._h, d_blob, blob_bytes, d_offsets, d_sizes, n, d_out,
                                                     out_stride, d_frames, d_status, 1 if sync else 0))

    def waveform_device(self, d_pcm, pcm_stride, d_frames, d_status, n, layout, wtype, d_wave, channel_stride,
                        packet_stride=0, d_starts=None, sync=True):
        """alacgpu_waveform_device: raw device pointers (ints). The PCM slots a device decode wrote (d_pcm / pcm_stride /
        d_frames, d_status or None) -> a planar float32 (WAVE_FLOAT) or int32 (WAVE_INT) waveform at d_wave, strides in
        elements: WAVE_STREAM [channels][channel_stride], the packets' frames back to back with failed packets left out;
        WAVE_PACKETS [n][channels] rows of FrameLength columns, zero behind a packet's frames. d_starts (n + 1 uint64, or
        None) gets the packets' first columns and the total. Runs on the handle's stream, behind a decode with sync=False."""
        _check(self._lib.alacgpu_waveform_device(self._h, d_pcm, pcm_stride, d_frames, d_status, n, layout, wtype, d_wave,
                                                 channel_stride, packet_stride, d_starts, 1 if sync else 0))

    def waveform_last_ms(self):
        """alacgpu_waveform_last_ms: HIP events around the kernels of the last waveform pass."""
        ms = ctypes.c_float()
        _check(self._lib.alacgpu_waveform_last_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def decode_waveform(self, blob, offsets, sizes=None, layout="stream", dtype=None):
        """Decode and convert on the device -> (wave, frames, status), torch tensors on the handle's device.

        blob: the packets' bytes, offsets: packet i's first byte (n entries with `sizes`, n + 1 without); numpy arrays or
        bytes are uploaded, CUDA tensors are used where they are. layout "stream": wave is [channels, total], the packets'
        frames back to back, failed packets (status != 0) left out; "packets": [n, channels, FrameLength], zero behind a
        packet's frames. dtype torch.float32 (samples x 2^-(w - 1), torchaudio's scale) or torch.int32 (the integers)."""
        return self._decode_waveform(blob, offsets, sizes, layout, dtype)

    def _upload(self, x, np_dtype, t_dtype):
        """A numpy array, bytes or a tensor -> a contiguous tensor of t_dtype on the handle's device (CUDA tensors of that
        type stay where they are)."""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(x, torch.Tensor):
            return x.to(device=dev, dtype=t_dtype).contiguous()
        if isinstance(x, (bytes, bytearray, memoryview)):
            x = np.frombuffer(x, dtype=np.uint8)
        a = np.ascontiguousarray(x, dtype=np_dtype)
        if t_dtype is not torch.uint8:
            a = a.view({8: np.int64, 4: np.int32}[a.itemsize])  # torch has no unsigned 32- / 64-bit tensors
        return torch.from_numpy(a.copy() if not a.flags.writeable else a).to(dev)

    def _upload_packets(self, blob, offsets, sizes):
        """The uploads decode_waveform and decode_clips share -> (d_blob, d_off, d_sz or None, n)."""
        import torch
        d_blob = self._upload(blob, np.uint8, torch.uint8)
        d_off = self._upload(offsets, np.uint64, torch.int64)
        d_sz = None if sizes is None else self._upload(sizes, np.uint32, torch.int32)
        n = d_off.numel() - (1 if d_sz is None else 0)
        if n < 0:
            raise ValueError("offsets without sizes needs n + 1 entries, at least one")
        if d_sz is not None and d_sz.numel() != n:
            raise ValueError("offsets and sizes differ in length")
        return d_blob, d_off, d_sz, n

    def _decode_waveform(self, blob, offsets, sizes, layout, dtype, into=None):
        """decode_waveform; into = (tensor [channels, capacity], column): "stream" writes there, from that column on,
        instead of allocating (load() fills one tensor window by window)."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.int32):
            raise ValueError("dtype must be torch.float32 or torch.int32")
        if layout not in ("stream", "packets"):
            raise ValueError("layout must be 'stream' or 'packets'")
        dev = torch.device("cuda", self.device)
        d_blob, d_off, d_sz, n = self._upload_packets(blob, offsets, sizes)
        fl, ch = int(self.config.FrameLength), int(self.config.NumChannels)
        stride = (self.frame_bytes + 15) // 16 * 16  # the decode's fast layout
        pcm = torch.empty((max(n, 1), stride), dtype=torch.uint8, device=dev)
        frames = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        col = 0
        if layout == "stream":
            if into is not None:
                wave, col = into
                if wave.dtype is not dtype or not wave.is_contiguous() or wave.shape[0] != ch or wave.shape[1] - col < n * fl:
                    raise ValueError("the waveform buffer does not take %d packets from column %d on" % (n, col))
            else:
                wave = torch.empty((ch, max(n * fl, 1)), dtype=dtype, device=dev)
            cs, ps = wave.shape[1], 0
        else:
            wave = torch.empty((n, ch, fl), dtype=dtype, device=dev)
            cs, ps = fl, ch * fl
        torch.cuda.synchronize(dev)  # the handle's stream does not order against torch's
        if n > 0:
            self.decode_batch_device(d_blob.data_ptr() if d_blob.numel() else None, d_blob.numel(), d_off.data_ptr(),
                                     None if d_sz is None else d_sz.data_ptr(), n, pcm.data_ptr(), stride, frames.data_ptr(),
                                     status.data_ptr(), sync=False)
        self.waveform_device(pcm.data_ptr(), stride, frames.data_ptr(), status.data_ptr(), n,
                             WAVE_STREAM if layout == "stream" else WAVE_PACKETS, WAVE_FLOAT if dtype is torch.float32 else WAVE_INT,
                             wave.data_ptr() + 4 * col, cs, ps, starts.data_ptr(), sync=True)
        if layout == "stream":
            wave = wave[:, col:col + int(starts[n].item())]
        return wave, frames[:n], status[:n]

    def clips_device(self, d_pcm, pcm_stride, d_frames, d_status, n, d_begin, d_limit, n_clips, clip_frames, wtype, d_clips,
                     channel_stride, clip_stride, d_valid=None, d_clip_status=None, sync=True):
        """alacgpu_clips_device: raw device pointers (ints). The PCM slots a device decode wrote (d_pcm / pcm_stride / d_frames,
        d_status or None) -> n_clips crops of clip_frames frames at d_clips, [n_clips][channels] rows, strides in elements,
        float32 (WAVE_FLOAT) or int32 (WAVE_INT). Slot i is the frames [i * FrameLength, (i + 1) * FrameLength) of a grid;
        d_begin[j] (uint64) is clip j's first grid frame, d_limit[j] (uint64) the first slot behind its source. Frames a clip
        does not find (a failed or short slot, the slots from d_limit[j] or n on) are zero; d_valid (uint32, or None) gets
        the count of those it found, d_clip_status (int32, or None) the status of the first failed slot it touches. Runs on
        the handle's stream, behind a decode with sync=False."""
        _check(self._lib.alacgpu_clips_device(self._h, d_pcm, pcm_stride, d_frames, d_status, n, d_begin, d_limit, n_clips,
                                              clip_frames, wtype, d_clips, channel_stride, clip_stride, d_valid, d_clip_status,
                                              1 if sync else 0))

    def clips_last_ms(self):
        """alacgpu_clips_last_ms: HIP events around the kernels of the last clip gather."""
        ms = ctypes.c_float()
        _check(self._lib.alacgpu_clips_last_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def decode_clips(self, blob, offsets, sizes=None, begin=(), limit=None, num_frames=1, dtype=None):
        """Decode and gather on the device -> (clips [B, channels, num_frames], valid [B], clip_status [B], frames, status),
        torch tensors on the handle's device.

        blob / offsets / sizes: the packets, as decode_waveform takes them. Packet i decodes into slot i, the frames
        [i * FrameLength, (i + 1) * FrameLength) of a grid over the batch. begin[j]: the first grid frame of clip j (any
        frame); limit[j]: the first slot that is not clip j's source any more (None: n for every clip). Frames a clip does
        not find are zero: valid (int32) counts the ones it found, clip_status is the status word of the first failed packet
        it touches, or 0. One decode and one gather, no host synchronisation in between."""
        return self._decode_clips(blob, offsets, sizes, begin, limit, num_frames, dtype)

    def _decode_clips(self, blob, offsets, sizes, begin, limit, num_frames, dtype, dest=None):
        """decode_clips; dest = (tensor, element, channel_stride, clip_stride): the clips go into that tensor's memory, clip
        0's channel 0 at that element of it, instead of into a new one (load() and load_clips() fill one tensor window by
        window), and None is returned for them."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.int32):
            raise ValueError("dtype must be torch.float32 or torch.int32")
        L = int(num_frames)
        if L < 1 or L > 0xFFFFFFFF:
            raise ValueError("num_frames must be 1 .. 2^32 - 1")
        dev = torch.device("cuda", self.device)
        d_blob, d_off, d_sz, n = self._upload_packets(blob, offsets, sizes)
        d_begin = self._upload(begin, np.uint64, torch.int64)
        B = d_begin.numel()
        d_limit = torch.full((B,), n, dtype=torch.int64, device=dev) if limit is None else self._upload(limit, np.uint64, torch.int64)
        if d_limit.numel() != B:
            raise ValueError("begin and limit differ in length")
        ch = int(self.config.NumChannels)
        stride = (self.frame_bytes + 15) // 16 * 16  # the decode's fast layout
        pcm = torch.empty((max(n, 1), stride), dtype=torch.uint8, device=dev)
        frames = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        if dest is None:
            clips = torch.empty((B, ch, L), dtype=dtype, device=dev)
            ptr, cs, ps = clips.data_ptr(), L, ch * L
        else:
            into, at, cs, ps = dest
            if into.dtype is not dtype or not into.is_contiguous() or cs < L or ps < ch * cs or at + (B - 1) * ps + (ch - 1) * cs + L > into.numel():
                raise ValueError("the clips buffer does not take %d clips of %d frames from element %d on" % (B, L, at))
            clips, ptr = None, into.data_ptr() + 4 * at
        valid = torch.zeros(B, dtype=torch.int32, device=dev)
        cstat = torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # the handle's stream does not order against torch's
        if n > 0:
            self.decode_batch_device(d_blob.data_ptr() if d_blob.numel() else None, d_blob.numel(), d_off.data_ptr(),
                                     None if d_sz is None else d_sz.data_ptr(), n, pcm.data_ptr(), stride, frames.data_ptr(),
                                     status.data_ptr(), sync=False)
        if B > 0:
            self.clips_device(pcm.data_ptr(), stride, frames.data_ptr(), status.data_ptr(), n, d_begin.data_ptr(), d_limit.data_ptr(),
                              B, L, WAVE_FLOAT if dtype is torch.float32 else WAVE_INT, ptr, cs, ps, valid.data_ptr(),
                              cstat.data_ptr(), sync=True)
        else:
            self.synchronize()
        return clips, valid, cstat, frames[:n], status[:n]

    def reserve(self, n_packets):
        _check(self._lib.alacgpu_reserve(self._h, n_packets))

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        _check(self._lib.alacgpu_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def timing_reset(self):
        _check(self._lib.alacgpu_timing_reset(self._h))

    def kernel_times_ms(self, max_n=64):
        """Durations (ms) of the most recent decode kernel launches, HIP events on the handle's stream."""
        ms = np.zeros(max_n, dtype=np.float32)
        got = ctypes.c_size_t()
        _check(self._lib.alacgpu_kernel_times(self._h, ms.ctypes.data, max_n, ctypes.byref(got)))
        return ms[:got.value].copy()

    def pair_placement(self, max_slots=1 << 16):
        """Diagnostics of the last device decode (include/alacgpu.h: alacgpu_pair_placement): an (n_slots, 4) uint32
        array, one row per wave slot of the launch plan — [tag, clock at start, clock at end, 0]; all zero for slots
        that no gated wave pair decoded."""
        raw = np.zeros((max_slots, 4), dtype=np.uint32)
        got = ctypes.c_size_t()
        _check(self._lib.alacgpu_pair_placement(self._h, raw.ctypes.data, raw.size, ctypes.byref(got)))
        return raw[:got.value].copy()

    def last_dispatch(self):
        """What the last device decode dispatched, read back from the plan the device built (include/alacgpu.h:
        alacgpu_last_dispatch) -> dict."""
        d = Dispatch()
        _check(self._lib.alacgpu_last_dispatch(self._h, ctypes.byref(d)))
        out = {k: int(getattr(d, k)) for k, _ in Dispatch._fields_[:8]}
        out.update({k: getattr(d, k).decode() for k in ("narrow_kernel", "wide_kernel", "irregular_kernels")})
        out["workgroups_per_cu"] = int(d.workgroups_per_cu)
        return out

    def synchronize(self):
        _check(self._lib.alacgpu_synchronize(self._h))


def NewPacketDecoder(config, device=0):
    """NewPacketDecoder (decoder.go:90): raises ErrConfig for bit depths outside {16,20,24,32}."""
    return PacketDecoder(config, device)


# ---- PacketEncoder (new: the reference is decode-only) ------------------------------------------------------------
class PacketEncoder:
    """Encodes interleaved LE PCM into ALAC packets on one MI355X (include/alacgpu.h: alacgpu_encoder_*).

    The input is the decoder's output format: [frames][channels] int16 (16-bit) / int32 (32-bit) arrays, or raw bytes (2 /
    3 / 3 / 4 bytes per sample at 16 / 20 / 24 / 32 bits; a 20-bit sample is left-aligned in 3 bytes and its low 4 bits
    are ignored). Packets of FrameLength frames, the last one possibly short; see alacgpu.h for the per-element policy.
    Single-caller, bound to one device and one stream."""

    def __init__(self, config, device=0):
        self._h = ctypes.c_void_p()
        self._lib = lib()
        self.config = config
        _check(self._lib.alacgpu_encoder_create(ctypes.byref(config), device, ctypes.byref(self._h)))
        self.device = device
        self.bytes_per_frame = config.NumChannels * bytes_per_sample(config.BitDepth)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.alacgpu_encoder_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _pcm_bytes(self, pcm):
        if isinstance(pcm, (bytes, bytearray, memoryview)):
            buf = np.frombuffer(bytes(pcm), dtype=np.uint8)
        else:
            arr = np.asarray(pcm)
            if arr.dtype == np.uint8 and arr.ndim == 1:
                buf = np.ascontiguousarray(arr)
            else:
                depth, ch = self.config.BitDepth, self.config.NumChannels
                if arr.ndim != 2 or arr.shape[1] != ch:
                    raise ValueError("pcm must be [frames][%d]" % ch)
                if depth == 16 and arr.dtype == np.int16:
                    buf = np.ascontiguousarray(arr, dtype="<i2").view(np.uint8).reshape(-1)
                elif depth == 32 and arr.dtype == np.int32:
                    buf = np.ascontiguousarray(arr, dtype="<i4").view(np.uint8).reshape(-1)
                elif depth in (20, 24) and arr.dtype == np.int32:
                    # an int32 array holds the samples in the PCM domain of the depth; 20-bit ones go left-aligned
                    v = arr.astype(np.int64).reshape(-1) << (4 if depth == 20 else 0)
                    b = (v & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]
                    buf = np.ascontiguousarray(b).reshape(-1)
                else:
                    raise ValueError("%s samples do not fit a %d-bit stream" % (arr.dtype, depth))
        if buf.size % self.bytes_per_frame:
            raise ValueError("pcm is not a whole number of frames")
        return buf

    def max_bytes(self, frames):
        """alacgpu_encode_max_bytes: a blob capacity that always suffices for `frames` frames."""
        return int(self._lib.alacgpu_encode_max_bytes(self._h, frames))

    def encode(self, pcm):
        """alacgpu_encode: PCM -> (blob np.uint8, offsets np.uint64[n + 1]); packet i is blob[offsets[i]:offsets[i + 1]]."""
        buf = self._pcm_bytes(pcm)
        frames = buf.size // self.bytes_per_frame
        fl = self.config.FrameLength
        n = (frames + fl - 1) // fl
        cap = self.max_bytes(frames)
        blob = np.empty(max(cap, 1), dtype=np.uint8)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        got = ctypes.c_uint64()
        _check(self._lib.alacgpu_encode(self._h, buf.ctypes.data if buf.size else None, frames, blob.ctypes.data, cap,
                                        offsets.ctypes.data, ctypes.byref(got)))
        return blob[:got.value].copy(), offsets

    def encode_device(self, d_pcm, total_frames, d_blob, blob_cap, d_offsets, sync=True):
        """alacgpu_encode_device: raw device pointers (ints), e.g. torch tensors' data_ptr(); d_offsets gets n + 1 uint64.
        The handle's stream does not order against torch's: synchronize the inputs first."""
        _check(self._lib.alacgpu_encode_device(self._h, d_pcm, total_frames, d_blob, blob_cap, d_offsets, 1 if sync else 0))

    def pcm_from_waveform_device(self, d_wave, layout, wtype, channel_stride, packet_stride, total_frames, d_pcm,
                                 d_clipped=None, sync=True):
        """alacgpu_pcm_from_waveform_device: raw device pointers (ints). A planar float32 (WAVE_FLOAT) or int32 (WAVE_INT)
        waveform at d_wave, strides in elements — WAVE_STREAM [channels][channel_stride], WAVE_PACKETS [n][channels] rows of
        FrameLength columns, the last clip possibly short — -> total_frames interleaved frames of the encoder's input
        format at d_pcm. d_clipped (one uint64, or None) gets the count of saturated and NaN samples. Runs on the handle's
        stream."""
        _check(self._lib.alacgpu_pcm_from_waveform_device(self._h, d_wave, layout, wtype, channel_stride, packet_stride,
                                                          total_frames, d_pcm, d_clipped, 1 if sync else 0))

    def encode_waveform_device(self, d_wave, layout, wtype, channel_stride, packet_stride, total_frames, d_blob, blob_cap,
                               d_offsets, d_clipped=None, sync=True):
        """alacgpu_encode_waveform_device: pcm_from_waveform_device into the handle's scratch, then encode_device, on the
        handle's stream with no host synchronisation in between."""
        _check(self._lib.alacgpu_encode_waveform_device(self._h, d_wave, layout, wtype, channel_stride, packet_stride,
                                                        total_frames, d_blob, blob_cap, d_offsets, d_clipped, 1 if sync else 0))

    def waveform_last_ms(self):
        """alacgpu_encoder_waveform_last_ms: HIP events around the kernels of the last pack pass."""
        ms = ctypes.c_float()
        _check(self._lib.alacgpu_encoder_waveform_last_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def encode_waveform(self, wave, layout="stream", frames=None):
        """Quantise, pack and encode on the device -> (blob, offsets, clipped).

        wave: a torch tensor on any device or a numpy array, float32 (samples in [-1, 1), torchaudio's scale) or int32 (the
        integers decode_waveform's int32 gives), [channels, T] for layout "stream" or [n, channels, FrameLength] for
        "packets"; the time axis must be contiguous, the other strides are taken as they are. frames: the frames to encode,
        default T or n * FrameLength. blob: uint8 CUDA tensor trimmed to offsets[n]; offsets: int64 CUDA tensor of n + 1
        entries; clipped: how many samples were saturated or NaN."""
        import torch
        if layout not in ("stream", "packets"):
            raise ValueError("layout must be 'stream' or 'packets'")
        if isinstance(wave, np.ndarray):
            if wave.dtype not in (np.float32, np.int32):
                raise ValueError("wave must be float32 or int32")
            if wave.ndim and wave.shape[-1] > 1 and wave.strides[-1] != wave.itemsize:
                raise ValueError("the time axis of wave must be contiguous")
            wave = torch.from_numpy(wave if wave.flags.writeable and all(s >= 0 for s in wave.strides) else wave.copy())
        if not isinstance(wave, torch.Tensor):
            raise ValueError("wave must be a torch tensor or a numpy array")
        if wave.dtype not in (torch.float32, torch.int32):
            raise ValueError("wave must be float32 or int32")
        fl, ch = int(self.config.FrameLength), int(self.config.NumChannels)
        if layout == "stream":
            if wave.dim() != 2 or wave.shape[0] != ch:
                raise ValueError("a 'stream' waveform is [%d, T]" % ch)
            room = int(wave.shape[1])
        else:
            if wave.dim() != 3 or wave.shape[1] != ch or wave.shape[2] != fl:
                raise ValueError("a 'packets' waveform is [n, %d, %d]" % (ch, fl))
            room = int(wave.shape[0]) * fl
        if wave.shape[-1] > 1 and wave.stride(-1) != 1:
            raise ValueError("the time axis of wave must be contiguous")
        frames = room if frames is None else int(frames)
        if frames < 0 or frames > room:
            raise ValueError("frames outside the waveform")
        dev = torch.device("cuda", self.device)
        wave = wave.to(dev)
        if wave.numel() == 0 or (wave.shape[-1] > 1 and wave.stride(-1) != 1):
            wave = wave.contiguous() if wave.numel() else torch.zeros(1, dtype=wave.dtype, device=dev)
        if layout == "stream":
            cs, ps = (int(wave.stride(0)) if ch > 1 and wave.numel() > 1 else max(room, 1)), 0
        else:
            cs = int(wave.stride(1)) if ch > 1 else fl
            ps = int(wave.stride(0)) if wave.shape[0] > 1 else ch * cs
        n = (frames + fl - 1) // fl
        cap = self.max_bytes(frames)
        blob = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        clipped = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)  # the handle's stream does not order against torch's
        self.encode_waveform_device(wave.data_ptr(), WAVE_STREAM if layout == "stream" else WAVE_PACKETS,
                                    WAVE_FLOAT if wave.dtype is torch.float32 else WAVE_INT, cs, ps, frames, blob.data_ptr(), cap,
                                    offsets.data_ptr(), clipped.data_ptr(), sync=True)
        return blob[:int(offsets[n].item())], offsets, int(clipped.item())

    def cookie(self):
        """alacgpu_encoder_cookie: 24-byte ALACSpecificConfig (ParseMagicCookie reads it) with the largest packet and the
        average bit rate of what this encoder has written."""
        out = (ctypes.c_uint8 * 24)()
        _check(self._lib.alacgpu_encoder_cookie(self._h, out))
        return bytes(out)

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        _check(self._lib.alacgpu_encoder_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def synchronize(self):
        _check(self._lib.alacgpu_encoder_synchronize(self._h))


def NewPacketEncoder(config, device=0):
    """A PacketEncoder (context manager); raises ErrConfig for the configs NewPacketDecoder rejects."""
    return PacketEncoder(config, device)


# ---- the float32 row passes (Resampler, MelSpectrogram, KaldiFeatures, FeatureNorm, FrameStack, SpecAugment, WaveAugment): what they share (§15a)
class _RowPass:
    """The handle of a row pass: _h (NULL once closed), _lib and device, and the entries every such handle has. A subclass names
    its C functions one by one (they are irregular: alacgpu_resampler_last_ms, but alacgpu_resample_out_frames), creates the
    handle with _create, and keeps its own device entry, plan() and __call__. A closed handle answers out_frames() with 0 and
    everything else with ValueError, on the host."""

    _CREATE = _DESTROY = _OUT_FRAMES = _LAST_MS = _SYNCHRONIZE = None

    def __init__(self):
        self._h = ctypes.c_void_p()
        self._lib = lib()

    def _create(self, device, *args):
        _check(getattr(self._lib, self._CREATE)(device, *args, ctypes.byref(self._h)))
        self.device = device

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            getattr(self._lib, self._DESTROY)(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def out_frames(self, in_frames):
        """The C entry's count of the frames (columns) a row of in_frames gives, by the formula in the class's docstring; 0
        where there is none."""
        return int(getattr(self._lib, self._OUT_FRAMES)(self._h, int(in_frames)))

    def last_ms(self):
        """HIP events around the kernels of the last pass; ValueError before the first pass that launched one."""
        ms = ctypes.c_float()
        _check(getattr(self._lib, self._LAST_MS)(self._h, ctypes.byref(ms)))
        return ms.value

    def synchronize(self):
        _check(getattr(self._lib, self._SYNCHRONIZE)(self._h))

    def _over_rows(self, waveform, shape, device_call):
        """The body of a __call__: waveform [..., T] made contiguous on the handle's device and flattened to rows, the output
        [rows] + shape allocated, torch synchronised and device_call(in pointer, rows, out pointer) run where there is an
        element to write -> the output as [...] + shape."""
        import torch
        dev = torch.device("cuda", self.device)
        T = int(waveform.shape[-1])
        rows = 1
        for d in waveform.shape[:-1]:
            rows *= int(d)
        x = waveform.to(dev).contiguous().reshape(rows, T)
        out = torch.empty((rows,) + shape, dtype=torch.float32, device=dev)
        if out.numel():
            torch.cuda.synchronize(dev)  # the handle's stream does not order against torch's
            device_call(x.data_ptr(), rows, out.data_ptr())
        return out.reshape(tuple(waveform.shape[:-1]) + shape)


def _fetch_plan(fn, handle, info, *tables_of):
    """The two calls of a plan export: the numbers into info, then the tables. Each of tables_of makes one zeroed numpy array
    from the filled info -> those arrays, filled."""
    _check(fn(handle, ctypes.byref(info), *(None, 0) * len(tables_of)))
    tables = [make(info) for make in tables_of]
    _check(fn(handle, ctypes.byref(info), *(a for t in tables for a in (t.ctypes.data, t.size))))
    return tables


def _float32_input(waveform):
    """ValueError unless waveform is a float32 torch tensor or numpy array [..., T]"""
    import torch
    if isinstance(waveform, np.ndarray):
        if waveform.dtype != np.float32:
            raise ValueError("waveform must be float32")
    elif not isinstance(waveform, torch.Tensor) or waveform.dtype is not torch.float32:
        raise ValueError("waveform must be a float32 torch tensor or numpy array")
    if waveform.ndim < 1:
        raise ValueError("waveform must be [..., T]")


def _on_device(waveform, device):
    """A checked input -> (a tensor, the device index): a numpy array wrapped, device None resolved to the tensor's own, cuda:0
    for what is on the host (the handle's __call__ uploads)"""
    import torch
    if isinstance(waveform, np.ndarray):
        waveform = torch.from_numpy(np.ascontiguousarray(waveform))
    if device is None:
        device = (waveform.device.index or 0) if waveform.is_cuda else 0
    return waveform, device


def _cached(cache, key, make):
    """cache[key], made by make() at its first use: one handle per (device, parameter set) and process"""
    if key not in cache:
        cache[key] = make()
    return cache[key]


# ---- the passes over feature tensors (FeatureNorm, FrameStack, SpecAugment): one strided view with per-row lengths (§16) ----
def _feature_strides(t, layout):
    """A tensor [rows, F, bins] (layout frames) or [rows, bins, F] (bins) -> its (row, frame, bin) strides, or None where
    neither inner stride is 1. The stride of an axis of one element is whatever torch keeps there: it is replaced."""
    rs, a, b = (int(s) for s in t.stride())
    fs, bs = (a, b) if layout == "frames" else (b, a)
    frames, bins = (t.shape[1], t.shape[2]) if layout == "frames" else (t.shape[2], t.shape[1])
    if frames == 1:
        fs = bins if bs == 1 else 1
    if bins == 1:
        bs = frames if fs == 1 else 1
    extent = (frames - 1) * fs + (bins - 1) * bs + 1
    if t.shape[0] == 1:
        rs = extent
    if (fs != 1 and bs != 1) or rs < extent:
        return None
    return rs, fs, bs


def _feature_rows(t, rows, layout):
    """[..., a, b] -> ([rows, a, b] without a copy, strides), or (None, None)"""
    try:
        v = t.view((rows,) + tuple(t.shape[-2:])) if t.ndim != 3 else t
    except RuntimeError:
        return None, None
    st = _feature_strides(v, layout) if v.numel() else (1, 1, 1)
    return (v, st) if st else (None, None)


def _feature_input(feats, layout, device):
    """What the one-call functions check before they pick a handle -> (bins, the device index: None resolved to the tensor's
    own, cuda:0 for what is on the host)"""
    import torch
    if not isinstance(feats, torch.Tensor) or feats.ndim < 2:
        raise ValueError("feats must be a float32 torch tensor [..., F, bins] or [..., bins, F]")
    if layout not in _FBANK_LAYOUTS:
        raise ValueError("layout is 'frames' or 'bins', not %r" % (layout,))
    if device is None:
        device = (feats.device.index or 0) if feats.is_cuda else 0
    return int(feats.shape[-1 if layout == "frames" else -2]), device


class _FeaturePass(_RowPass):
    """A row pass over float32 features [..., F, bins] or [..., bins, F] with per-row lengths; the subclass sets bins."""

    def _features(self, feats, layout):
        """What a __call__ checks behind its layouts -> (the handle's torch device, the leading dimensions, rows, frames)"""
        import torch
        if not self._h:
            raise ValueError("the handle is closed")
        if not isinstance(feats, torch.Tensor) or feats.dtype is not torch.float32 or feats.ndim < 2:
            raise ValueError("feats must be a float32 torch tensor [..., F, bins] or [..., bins, F]")
        if int(feats.shape[-1 if layout == "frames" else -2]) != self.bins:
            raise ValueError("feats has %d bins, the handle %d" % (feats.shape[-1 if layout == "frames" else -2], self.bins))
        lead = tuple(feats.shape[:-2])
        rows = int(np.prod(lead, dtype=np.int64))
        return torch.device("cuda", self.device), lead, rows, int(feats.shape[-2 if layout == "frames" else -1])

    @staticmethod
    def _lengths(lengths, rows, dev):
        """lengths (None, or one integer per row) -> None, or an int32 tensor [rows] on dev: lengths itself where it is one
        already. The caller holds the tensor until its device call, which is synchronous, has returned."""
        import torch
        if lengths is None:
            return None
        if not isinstance(lengths, torch.Tensor):
            lengths = torch.as_tensor(np.asarray(lengths))
        if lengths.numel() != rows or lengths.dtype.is_floating_point:
            raise ValueError("lengths holds one integer per row: %d, not %d" % (rows, lengths.numel()))
        info = torch.iinfo(torch.int32)
        ln = lengths if lengths.dtype is torch.int32 else lengths.clamp(info.min, info.max).to(torch.int32)
        return ln.to(dev).contiguous().reshape(rows)


# ---- Resampler (new: torchaudio.functional.resample's sinc_interp_hann on the device) ----------------------------------
class ResampleInfo(ctypes.Structure):
    """alacgpu_resample_info (include/alacgpu.h)."""

    _fields_ = [("o", ctypes.c_uint32), ("n", ctypes.c_uint32), ("width", ctypes.c_uint32), ("taps", ctypes.c_uint32),
                ("tile_out", ctypes.c_uint32)]


class Resampler(_RowPass):
    """float32 rows at orig_freq -> the same rows at new_freq on one MI355X (include/alacgpu.h: alacgpu_resampler_*):
    torchaudio's sinc_interp_hann, its table built once per handle. ValueError when no plan can be built (equal or zero
    rates, a width of 0, rolloff outside (0, 1], a ratio too steep for the kernel's staging buffer). Single-caller, bound to
    one device and one stream. out_frames(T) is alacgpu_resample_out_frames: ceil(new_freq * T / orig_freq)."""

    _CREATE, _DESTROY, _OUT_FRAMES = "alacgpu_resampler_create", "alacgpu_resampler_destroy", "alacgpu_resample_out_frames"
    _LAST_MS, _SYNCHRONIZE = "alacgpu_resampler_last_ms", "alacgpu_resampler_synchronize"

    def __init__(self, orig_freq, new_freq, device=0, lowpass_filter_width=6, rolloff=0.99):
        super().__init__()
        for v in (orig_freq, new_freq, lowpass_filter_width):
            if int(v) != v or not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError("the rates and the filter width are integers below 2^32")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self._create(device, self.orig_freq, self.new_freq, int(lowpass_filter_width), float(rolloff))

    def resample_device(self, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, sync=True):
        """alacgpu_resample_device: raw device pointers (ints), strides in elements. rows rows of in_frames float32 frames ->
        rows of out_frames(in_frames); exactly those columns of every output row are written. Runs on the handle's stream,
        which does not order against torch's: synchronize the input first."""
        _check(self._lib.alacgpu_resample_device(self._h, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride,
                                                 1 if sync else 0))

    def plan(self):
        """alacgpu_resampler_plan -> dict: o, n, width, taps, tile_out, and the host copies of the table the kernel uses, h
        [n, taps] float32 and first [n] int32 (the tap index of each phase's first kept tap)."""
        info = ResampleInfo()
        h, first = _fetch_plan(self._lib.alacgpu_resampler_plan, self._h, info, lambda i: np.zeros((i.n, i.taps), np.float32),
                               lambda i: np.zeros(i.n, np.int32))
        out = {k: int(getattr(info, k)) for k, _ in ResampleInfo._fields_}
        out.update(h=h, first=first)
        return out

    def __call__(self, waveform):
        """A float32 CUDA tensor [..., T] on the handle's device -> [..., out_frames(T)] (made contiguous, flattened to rows)."""
        T = int(waveform.shape[-1])
        frames = self.out_frames(T)
        if T and not frames:
            raise ValueError("%d frames are more than one pass takes" % T)
        return self._over_rows(waveform, (frames,),
                               lambda x, rows, out: self.resample_device(x, T, rows, T, out, frames, sync=True))


def NewResampler(orig_freq, new_freq, device=0, lowpass_filter_width=6, rolloff=0.99):
    """A Resampler (context manager); ValueError where no plan can be built."""
    return Resampler(orig_freq, new_freq, device, lowpass_filter_width, rolloff)


_RESAMPLERS = {}  # (device, orig, new, width, rolloff) -> Resampler: a plan is built once per process


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, device=None):
    """torchaudio.functional.resample(waveform, orig_freq, new_freq) with its default sinc_interp_hann, on the device: a
    float32 tensor [..., T] -> [..., ceil(new_freq * T / orig_freq)] on cuda:`device` (default: the tensor's own device, cuda:0
    for a CPU tensor or a numpy array, which are uploaded). Equal rates return the input as it is; another dtype raises
    ValueError. The filter table of a (device, rates, width, rolloff) is built once and kept."""
    _float32_input(waveform)
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq <= 0 or new_freq <= 0:
        raise ValueError("orig_freq and new_freq must be positive integers")
    if int(orig_freq) == int(new_freq):
        return waveform
    waveform, device = _on_device(waveform, device)
    key = (device, int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff))
    return _cached(_RESAMPLERS, key, lambda: Resampler(orig_freq, new_freq, device, lowpass_filter_width, rolloff))(waveform)


# ---- MelSpectrogram (new: torch.stft + |.|^2 + torchaudio's melscale_fbanks + log, one fused pass on the device) --------
class MelConfig(ctypes.Structure):
    """alacgpu_mel_config (include/alacgpu.h)."""

    _fields_ = [("sample_rate", ctypes.c_uint32), ("n_fft", ctypes.c_uint32), ("win_length", ctypes.c_uint32),
                ("hop_length", ctypes.c_uint32), ("f_min", ctypes.c_double), ("f_max", ctypes.c_double), ("n_mels", ctypes.c_uint32),
                ("center", ctypes.c_uint32), ("norm", ctypes.c_uint32), ("mel_scale", ctypes.c_uint32), ("log", ctypes.c_uint32),
                ("transform", ctypes.c_uint32), ("floor", ctypes.c_double)]


class MelInfo(ctypes.Structure):
    """alacgpu_mel_info (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_uint32) for k in ("n_fft", "win_length", "hop_length", "n_freqs", "n_mels", "taps", "bins",
                                               "tile_frames", "lds_bytes")]


class MelFftInfo(ctypes.Structure):
    """alacgpu_mel_fft_info (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_uint32) for k in ("transform", "tile_frames", "lds_bytes", "batch_frames", "pitch", "n_passes")] + [
        ("radix", ctypes.c_uint32 * 8), ("window_entries", ctypes.c_uint32), ("twiddle_entries", ctypes.c_uint32)]


_MEL_TRANSFORMS = {"direct": 0, "fft": 1}
_MEL_SCALES = {"htk": 1, "slaney": 2}
_MEL_LOGS = {None: 0, "ln": 1, "log10": 2, "db": 3}


def _mel_config(sample_rate, n_fft, win_length, hop_length, f_min, f_max, n_mels, center, norm, mel_scale, log, floor,
                transform="direct"):
    """The arguments of the Python entries -> MelConfig, defaults resolved; ValueError for what is no number of its kind or no
    name of an enum (what the numbers may be is the plan's to say)."""
    if not isinstance(transform, str) or transform not in _MEL_TRANSFORMS:
        raise ValueError("transform is 'direct' or 'fft', not %r" % (transform,))
    for v in (sample_rate, n_fft) + tuple(u for u in (win_length, hop_length, n_mels) if u is not None):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("sample_rate, n_fft, win_length, hop_length and n_mels are integers in [0, 2^32)")
    if norm not in (None, "slaney"):
        raise ValueError("norm is None or 'slaney', not %r" % (norm,))
    if log not in _MEL_LOGS:
        raise ValueError("log is None, 'ln', 'log10' or 'db', not %r" % (log,))
    if n_mels is not None and mel_scale not in _MEL_SCALES:
        raise ValueError("mel_scale is 'htk' or 'slaney', not %r" % (mel_scale,))
    if n_mels is not None and int(n_mels) == 0:
        raise ValueError("n_mels is at least 1 (None gives the power spectrogram itself)")
    win = int(n_fft) if win_length is None else int(win_length)
    hop = win // 2 if hop_length is None else int(hop_length)
    c = MelConfig()
    c.sample_rate, c.n_fft, c.win_length, c.hop_length = int(sample_rate), int(n_fft), win, hop
    c.f_min = float(f_min)
    c.f_max = float(int(sample_rate) / 2 if f_max is None else f_max)
    c.center = 1 if center else 0
    c.log, c.floor = _MEL_LOGS[log], float(floor)
    c.transform = _MEL_TRANSFORMS[transform]
    if n_mels is not None:
        c.n_mels, c.norm, c.mel_scale = int(n_mels), 1 if norm == "slaney" else 0, _MEL_SCALES[mel_scale]
    return c


class MelSpectrogram(_RowPass):
    """float32 rows -> their power spectrograms (n_mels None) or (log-)mel spectrograms on one MI355X (include/alacgpu.h:
    alacgpu_mel_*): periodic Hann window, reflect padding when centred, |X|^2, torchaudio's melscale_fbanks, s log(max(v,
    floor)); the tables are built once per handle. ValueError when no plan can be built. Single-caller, bound to one device
    and one stream. transform="fft" (keyword only; the default "direct" is the fmaf chains over the basis) computes the powers by
    a mixed-radix FFT: n_fft must be even with n_fft / 2 = 2^a 3^b 5^c, any other is a ValueError, never a fall-back; the result
    is fixed bit for bit as well, but it is not the direct transform's. out_frames(T) is alacgpu_mel_out_frames: 1 + (T - n_fft %
    2) / hop centred (T > n_fft / 2; torch.stft's count: it pads n_fft / 2 on each side), 1 + (T - n_fft) / hop otherwise; 0 where
    no frame exists."""

    _CREATE, _DESTROY, _OUT_FRAMES = "alacgpu_mel_create", "alacgpu_mel_destroy", "alacgpu_mel_out_frames"
    _LAST_MS, _SYNCHRONIZE = "alacgpu_mel_last_ms", "alacgpu_mel_synchronize"

    def __init__(self, sample_rate, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, n_mels=128, center=True,
                 norm=None, mel_scale="htk", log=None, floor=1e-10, device=0, *, transform="direct"):
        super().__init__()
        self.config = _mel_config(sample_rate, n_fft, win_length, hop_length, f_min, f_max, n_mels, center, norm, mel_scale, log, floor,
                                  transform)
        self.transform = transform
        self._create(device, ctypes.byref(self.config))
        self.bins = int(n_mels) if n_mels is not None else int(n_fft) // 2 + 1

    def mel_device(self, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, out_bin_stride, sync=True):
        """alacgpu_mel_device: raw device pointers (ints), strides in elements. rows rows of in_frames float32 samples ->
        [rows][bins][out_frames(in_frames)], element (r, b, f) at d_out + r * out_row_stride + b * out_bin_stride + f; exactly
        those elements are written. Runs on the handle's stream, which does not order against torch's: synchronize the input
        first."""
        _check(self._lib.alacgpu_mel_device(self._h, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, out_bin_stride,
                                            1 if sync else 0))

    def plan(self):
        """alacgpu_mel_plan -> dict: n_fft, win_length, hop_length, n_freqs, n_mels, taps, bins, tile_frames, lds_bytes, and the
        host copies of the tables the kernel uses: basis [2, n_freqs, n_fft] float32 (C, then S), fb [n_mels, taps] float32 (each
        filter's window) and first [n_mels] int32 (the bin of each window's first weight)."""
        info = MelInfo()
        basis, fb, first = _fetch_plan(
            self._lib.alacgpu_mel_plan, self._h, info,
            lambda i: np.zeros((2, i.n_freqs if self.config.transform == 0 else 0, i.n_fft), np.float32),
            lambda i: np.zeros((i.n_mels, i.taps), np.float32), lambda i: np.zeros(i.n_mels, np.int32))
        out = {k: int(getattr(info, k)) for k, _ in MelInfo._fields_}
        out.update(basis=basis, fb=fb, first=first)
        return out

    def fft_plan(self):
        """alacgpu_mel_fft_plan -> dict: transform (0 direct, 1 fft), tile_frames, lds_bytes, batch_frames, pitch, n_passes, radix
        (the passes' radices in order), and the tables window [n_fft] float32 and twiddle float32 (8 roots, each pass's twiddles,
        the split step's n_fft / 2 + 1 pairs). On a direct handle: transform 0, no passes, empty tables."""
        info = MelFftInfo()
        window, twiddle = _fetch_plan(self._lib.alacgpu_mel_fft_plan, self._h, info, lambda i: np.zeros(i.window_entries, np.float32),
                                      lambda i: np.zeros(i.twiddle_entries, np.float32))
        out = {k: int(getattr(info, k)) for k in ("transform", "tile_frames", "lds_bytes", "batch_frames", "pitch", "n_passes")}
        out.update(radix=[int(r) for r in info.radix[:info.n_passes]], window=window, twiddle=twiddle)
        return out

    def __call__(self, waveform):
        """A float32 tensor [..., T] -> [..., bins, out_frames(T)] on the handle's device (made contiguous, flattened to rows):
        1 + (T - n_fft % 2) / hop frames centred, as torch.stft has them. ValueError where T has no frame."""
        T = int(waveform.shape[-1])
        frames = self.out_frames(T)
        if not frames:
            raise ValueError("%d samples have no frame of n_fft %d" % (T, self.config.n_fft))
        return self._over_rows(waveform, (self.bins, frames),
                               lambda x, rows, out: self.mel_device(x, T, rows, T, out, self.bins * frames, frames, sync=True))


def NewMelSpectrogram(sample_rate, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, n_mels=128, center=True,
                      norm=None, mel_scale="htk", log=None, floor=1e-10, device=0, *, transform="direct"):
    """A MelSpectrogram (context manager); ValueError where no plan can be built."""
    return MelSpectrogram(sample_rate, n_fft, win_length, hop_length, f_min, f_max, n_mels, center, norm, mel_scale, log, floor, device,
                          transform=transform)


_MELS = {}  # (device, every field of the configuration) -> MelSpectrogram: a plan is built once per process


def mel_spectrogram(waveform, sample_rate, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, n_mels=128,
                    center=True, norm=None, mel_scale="htk", log=None, floor=1e-10, device=None, *, transform="direct"):
    """torchaudio.transforms.MelSpectrogram(sample_rate, n_fft, win_length, hop_length, f_min, f_max, n_mels=n_mels, center=center,
    norm=norm, mel_scale=mel_scale)(waveform) with power 2, the periodic Hann window and reflect padding, and optionally s
    log(max(., floor)) (log: None, "ln", "log10", "db"), in one pass on the device: a float32 tensor [..., T] (CUDA, CPU or
    numpy; the last two are uploaded) -> [..., n_mels, F] on cuda:`device` (default: the tensor's own device, cuda:0 for a CPU
    tensor or a numpy array). n_mels None gives the power spectrogram [..., n_fft / 2 + 1, F]. Another dtype, parameters without
    a plan or a T without a frame raise ValueError. The tables of a (device, parameter set) are built once and kept.
    transform="fft" takes the FFT in place of the direct transform (MelSpectrogram); the two have handles of their own."""
    _float32_input(waveform)
    c = _mel_config(sample_rate, n_fft, win_length, hop_length, f_min, f_max, n_mels, center, norm, mel_scale, log, floor, transform)
    waveform, device = _on_device(waveform, device)
    key = (device,) + tuple(getattr(c, k) for k, _ in MelConfig._fields_)
    return _cached(_MELS, key, lambda: MelSpectrogram(sample_rate, n_fft, win_length, hop_length, f_min, f_max, n_mels, center, norm,
                                                      mel_scale, log, floor, device, transform=transform))(waveform)


def spectrogram(waveform, sample_rate, n_fft=400, win_length=None, hop_length=None, center=True, log=None, floor=1e-10, device=None,
                *, transform="direct"):
    """mel_spectrogram without the mel stage: the power spectrogram [..., n_fft / 2 + 1, F] (torchaudio.transforms.Spectrogram
    with power 2), sample_rate only naming the handle."""
    return mel_spectrogram(waveform, sample_rate, n_fft, win_length, hop_length, n_mels=None, center=center, log=log, floor=floor,
                           device=device, transform=transform)


def whisper_post(logmel):
    """Whisper's post-processing of a log10 mel tensor [..., n_mels, F], in torch ops: drop the last frame, clamp below (the
    maximum over [n_mels, frames]) - 8, then (x + 4) / 4."""
    import torch
    x = logmel[..., :-1]
    top = x.amax(dim=(-2, -1), keepdim=True)
    x = torch.maximum(x, top - 8.0)
    return (x + 4.0) / 4.0


def whisper_log_mel(waveform, n_mels=80, device=None, *, transform="direct"):
    """Whisper's log_mel_spectrogram of 16 kHz audio [..., T] -> [..., n_mels, T / 160]: the pass at n_fft 400, hop 160 with the
    slaney scale and norm and log10 at floor 1e-10, then whisper_post."""
    return whisper_post(mel_spectrogram(waveform, 16000, 400, 400, 160, 0.0, 8000.0, n_mels, True, "slaney", "slaney", "log10",
                                        1e-10, device, transform=transform))


# ---- Kaldi features (new: torchaudio.compliance.kaldi.fbank / .mfcc, one fused pass on the device) ---------------------
class FbankConfig(ctypes.Structure):
    """alacgpu_fbank_config (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_uint32) for k in ("sample_rate", "frame_length", "frame_shift", "round_to_power_of_two", "num_mel_bins",
                                               "num_ceps", "snip_edges", "remove_dc_offset", "window_type", "use_log_fbank",
                                               "use_energy", "raw_energy", "htk_compat", "use_power", "log_energy", "layout")] + [
        (k, ctypes.c_double) for k in ("preemphasis_coefficient", "blackman_coeff", "low_freq", "high_freq", "energy_floor", "scale",
                                       "cepstral_lifter", "dither", "vtln_warp")]


class FbankInfo(ctypes.Structure):
    """alacgpu_fbank_info (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_uint32) for k in ("frame_length", "frame_shift", "n_fft", "n_freqs", "num_mel_bins", "taps", "num_ceps",
                                               "cols", "tile_frames", "lds_bytes")]


class FbankFftInfo(ctypes.Structure):
    """alacgpu_fbank_fft_info (include/alacgpu.h)."""

    _fields_ = MelFftInfo._fields_


_FBANK_TRANSFORMS = {"direct": 0, "fft": 1}
_FBANK_WINDOWS = {"hanning": 0, "hamming": 1, "povey": 2, "rectangular": 3, "blackman": 4}
_FBANK_LAYOUTS = {"frames": 0, "bins": 1}


def _fbank_transform(transform):
    """"direct" or "fft" -> ALACGPU_FBANK_TRANSFORM_*; ValueError for anything else"""
    if not isinstance(transform, str) or transform not in _FBANK_TRANSFORMS:
        raise ValueError("transform is 'direct' or 'fft', not %r" % (transform,))
    return _FBANK_TRANSFORMS[transform]


def _fbank_config(sample_rate, frame_length, frame_shift, num_mel_bins, num_ceps, round_to_power_of_two, snip_edges, remove_dc_offset,
                  window_type, use_log_fbank, use_energy, raw_energy, htk_compat, use_power, log_energy, layout,
                  preemphasis_coefficient, blackman_coeff, low_freq, high_freq, energy_floor, scale, cepstral_lifter, dither,
                  vtln_warp):
    """The arguments of the handle (lengths in samples) -> FbankConfig; ValueError for what is no number of its kind or no name
    of an enum (what the numbers may be is the plan's to say)."""
    for v in (sample_rate, frame_length, frame_shift, num_mel_bins, num_ceps):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError("sample_rate, frame_length, frame_shift, num_mel_bins and num_ceps are integers in [0, 2^32)")
    if window_type not in _FBANK_WINDOWS:
        raise ValueError("window_type is one of %s, not %r" % (", ".join(sorted(_FBANK_WINDOWS)), window_type))
    if layout not in _FBANK_LAYOUTS:
        raise ValueError("layout is 'frames' or 'bins', not %r" % (layout,))
    c = FbankConfig()
    c.sample_rate, c.frame_length, c.frame_shift = int(sample_rate), int(frame_length), int(frame_shift)
    c.num_mel_bins, c.num_ceps = int(num_mel_bins), int(num_ceps)
    c.round_to_power_of_two, c.snip_edges, c.remove_dc_offset = int(bool(round_to_power_of_two)), int(bool(snip_edges)), int(bool(remove_dc_offset))
    c.window_type, c.layout = _FBANK_WINDOWS[window_type], _FBANK_LAYOUTS[layout]
    c.use_log_fbank, c.use_energy, c.raw_energy = int(bool(use_log_fbank)), int(bool(use_energy)), int(bool(raw_energy))
    c.htk_compat, c.use_power, c.log_energy = int(bool(htk_compat)), int(bool(use_power)), int(bool(log_energy))
    c.preemphasis_coefficient, c.blackman_coeff = float(preemphasis_coefficient), float(blackman_coeff)
    c.low_freq, c.high_freq, c.energy_floor = float(low_freq), float(high_freq), float(energy_floor)
    c.scale, c.cepstral_lifter, c.dither, c.vtln_warp = float(scale), float(cepstral_lifter), float(dither), float(vtln_warp)
    return c


class KaldiFeatures(_RowPass):
    """float32 rows -> Kaldi's fbank (num_ceps 0) or MFCC features on one MI355X (include/alacgpu.h: alacgpu_fbank_*). Lengths
    are in samples here; kaldi_fbank / kaldi_mfcc take torchaudio's milliseconds. layout "frames" gives [..., F, cols], "bins"
    [..., cols, F]. log_energy=False keeps the energy column unlogged (for checks). MFCC with htk_compat and without use_energy
    ends in sqrt(2) C0 (plan()["dct"][0] is sqrt(2 / num_mel_bins) there). ValueError when no plan can be built:
    dither != 0, vtln_warp != 1, use_power False and use_energy without raw_energy among them, before any HIP call.
    transform="fft" (keyword only; the default "direct" is the fmaf chains over the folded basis) removes the mean, pre-emphasises
    and windows each frame in float32 and computes the powers by a mixed-radix FFT: the DFT size (the next power of two >=
    frame_length with round_to_power_of_two, else frame_length) must be even with its half 2^a 3^b 5^c, any other is a ValueError,
    never a fall-back; the result is fixed bit for bit as well, but only its energy column is the direct transform's.
    Single-caller, bound to one device and one stream. out_frames(T) is alacgpu_fbank_out_frames: 1 + (T - W) / h with snip_edges,
    (T + h / 2) / h without; 0 for T < W."""

    _CREATE, _DESTROY, _OUT_FRAMES = "alacgpu_fbank_create", "alacgpu_fbank_destroy", "alacgpu_fbank_out_frames"
    _LAST_MS, _SYNCHRONIZE = "alacgpu_fbank_last_ms", "alacgpu_fbank_synchronize"

    def __init__(self, sample_rate, frame_length, frame_shift, num_mel_bins=23, num_ceps=0, round_to_power_of_two=True,
                 snip_edges=True, remove_dc_offset=True, window_type="povey", use_log_fbank=True, use_energy=False, raw_energy=True,
                 htk_compat=False, use_power=True, log_energy=True, layout="frames", preemphasis_coefficient=0.97,
                 blackman_coeff=0.42, low_freq=20.0, high_freq=0.0, energy_floor=1.0, scale=1.0, cepstral_lifter=22.0, dither=0.0,
                 vtln_warp=1.0, device=0, *, transform="direct"):
        super().__init__()
        self.transform = transform
        self._transform = _fbank_transform(transform)
        self.config = _fbank_config(sample_rate, frame_length, frame_shift, num_mel_bins, num_ceps, round_to_power_of_two, snip_edges,
                                    remove_dc_offset, window_type, use_log_fbank, use_energy, raw_energy, htk_compat, use_power,
                                    log_energy, layout, preemphasis_coefficient, blackman_coeff, low_freq, high_freq, energy_floor,
                                    scale, cepstral_lifter, dither, vtln_warp)
        if self._transform:
            self._CREATE = "alacgpu_fbank_create_transform"
            self._create(device, ctypes.byref(self.config), self._transform)
        else:
            self._create(device, ctypes.byref(self.config))
        self.layout = layout
        self.cols = int(num_ceps) if int(num_ceps) else int(num_mel_bins) + int(bool(use_energy))

    def features_device(self, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, out_inner_stride, sync=True):
        """alacgpu_fbank_device: raw device pointers (ints), strides in elements. rows rows of in_frames float32 samples ->
        element (r, f, c) at d_out + r * out_row_stride + f * out_inner_stride + c (layout frames) or (r, c, f) at d_out + r *
        out_row_stride + c * out_inner_stride + f (layout bins); exactly those elements are written. Runs on the handle's
        stream, which does not order against torch's: synchronize the input first."""
        _check(self._lib.alacgpu_fbank_device(self._h, d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, out_inner_stride,
                                              1 if sync else 0))

    def plan(self):
        """alacgpu_fbank_plan -> dict: the numbers of alacgpu_fbank_info and the host copies of the tables the kernel uses: basis
        [2, n_freqs, frame_length] float32 (C, then S, folded), fb [num_mel_bins, taps], first [num_mel_bins] int32, dct
        [num_ceps, num_mel_bins] and lifter [num_ceps]. A handle with transform="fft" has no basis: [2, 0, frame_length]."""
        info = FbankInfo()
        basis, fb, first, dct, lifter = _fetch_plan(
            self._lib.alacgpu_fbank_plan, self._h, info,
            lambda i: np.zeros((2, 0 if self._transform else i.n_freqs, i.frame_length), np.float32),
            lambda i: np.zeros((i.num_mel_bins, i.taps), np.float32), lambda i: np.zeros(i.num_mel_bins, np.int32),
            lambda i: np.zeros((i.num_ceps, i.num_mel_bins), np.float32), lambda i: np.zeros(i.num_ceps, np.float32))
        out = {k: int(getattr(info, k)) for k, _ in FbankInfo._fields_}
        out.update(basis=basis, fb=fb, first=first, dct=dct, lifter=lifter)
        return out

    def fft_plan(self):
        """alacgpu_fbank_fft_plan -> dict: transform (0 direct, 1 fft), tile_frames, lds_bytes, batch_frames, pitch, n_passes, radix
        (the passes' radices in order), and the tables window [n_fft] float32 (scale * window, zeros from frame_length on) and
        twiddle float32 (laid out as MelSpectrogram.fft_plan's). On a direct handle: transform 0, no passes, empty tables."""
        info = FbankFftInfo()
        window, twiddle = _fetch_plan(self._lib.alacgpu_fbank_fft_plan, self._h, info, lambda i: np.zeros(i.window_entries, np.float32),
                                      lambda i: np.zeros(i.twiddle_entries, np.float32))
        out = {k: int(getattr(info, k)) for k in ("transform", "tile_frames", "lds_bytes", "batch_frames", "pitch", "n_passes")}
        out.update(radix=[int(r) for r in info.radix[:info.n_passes]], window=window, twiddle=twiddle)
        return out

    def __call__(self, waveform):
        """A float32 tensor [..., T] -> [..., F, cols] (layout frames) or [..., cols, F] (bins) on the handle's device (made
        contiguous, flattened to rows). ValueError where T has no frame (T < frame_length)."""
        T = int(waveform.shape[-1])
        frames = self.out_frames(T)
        if not frames:
            raise ValueError("%d samples have no frame of %d" % (T, self.config.frame_length))
        shape = (frames, self.cols) if self.layout == "frames" else (self.cols, frames)
        return self._over_rows(waveform, shape,
                               lambda x, rows, out: self.features_device(x, T, rows, T, out, self.cols * frames, shape[1], sync=True))


def NewKaldiFeatures(*args, **kw):
    """A KaldiFeatures (context manager); ValueError where no plan can be built."""
    return KaldiFeatures(*args, **kw)


_KALDIS = {}  # (device, every field of the configuration) -> KaldiFeatures: a plan is built once per process


def _kaldi(waveform, sample_frequency, frame_length, frame_shift, subtract_mean, device, transform, **kw):
    _float32_input(waveform)
    which = _fbank_transform(transform)
    # torchaudio's _get_waveform_and_window_properties: milliseconds -> samples
    W, h = int(sample_frequency * frame_length * 0.001), int(sample_frequency * frame_shift * 0.001)
    c = _fbank_config(sample_frequency, W, h, kw["num_mel_bins"], kw["num_ceps"], kw["round_to_power_of_two"], kw["snip_edges"],
                      kw["remove_dc_offset"], kw["window_type"], kw["use_log_fbank"], kw["use_energy"], kw["raw_energy"],
                      kw["htk_compat"], kw["use_power"], True, kw["layout"], kw["preemphasis_coefficient"], kw["blackman_coeff"],
                      kw["low_freq"], kw["high_freq"], kw["energy_floor"], kw["scale"], kw["cepstral_lifter"], kw["dither"],
                      kw["vtln_warp"])
    waveform, device = _on_device(waveform, device)
    key = (device, which) + tuple(getattr(c, k) for k, _ in FbankConfig._fields_)
    out = _cached(_KALDIS, key, lambda: KaldiFeatures(sample_frequency, W, h, device=device, transform=transform, **kw))(waveform)
    if subtract_mean:  # over the frames, as torchaudio's _subtract_column_mean: a torch op, as Whisper's post-processing is
        out = out - out.mean(dim=-2 if kw["layout"] == "frames" else -1, keepdim=True)
    return out


def kaldi_fbank(waveform, sample_frequency=16000, blackman_coeff=0.42, dither=0.0, energy_floor=1.0, frame_length=25.0,
                frame_shift=10.0, high_freq=0.0, htk_compat=False, low_freq=20.0, num_mel_bins=23, preemphasis_coefficient=0.97,
                raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True, snip_edges=True, subtract_mean=False,
                use_energy=False, use_log_fbank=True, use_power=True, vtln_warp=1.0, window_type="povey", scale=1.0,
                layout="frames", device=None, *, transform="direct"):
    """torchaudio.compliance.kaldi.fbank(waveform, ...) in one pass on the device, with torchaudio's keyword names and defaults
    (frame_length / frame_shift in milliseconds; sample_frequency an integer): a float32 tensor [..., T] (CUDA, CPU or numpy;
    the last two are uploaded) -> [..., F, num_mel_bins (+ 1 with use_energy)] on cuda:`device`, or [..., cols, F] with
    layout="bins". scale multiplies the waveform (32768 for recipes made for 16-bit sample values) at no cost. ValueError for
    dither != 0, vtln_warp != 1, use_power=False, use_energy without raw_energy, parameters without a plan, another dtype, or
    T below one frame (torchaudio returns frames there without snip_edges; this does not). The tables of a (device, parameter
    set) are built once and kept. transform="fft" takes the FFT in place of the direct transform (KaldiFeatures); the two have
    handles of their own."""
    return _kaldi(waveform, sample_frequency, frame_length, frame_shift, subtract_mean, device, transform, num_mel_bins=num_mel_bins,
                  num_ceps=0,
                  round_to_power_of_two=round_to_power_of_two, snip_edges=snip_edges, remove_dc_offset=remove_dc_offset,
                  window_type=window_type, use_log_fbank=use_log_fbank, use_energy=use_energy, raw_energy=raw_energy,
                  htk_compat=htk_compat, use_power=use_power, layout=layout, preemphasis_coefficient=preemphasis_coefficient,
                  blackman_coeff=blackman_coeff, low_freq=low_freq, high_freq=high_freq, energy_floor=energy_floor, scale=scale,
                  cepstral_lifter=0.0, dither=dither, vtln_warp=vtln_warp)


def kaldi_mfcc(waveform, sample_frequency=16000, blackman_coeff=0.42, cepstral_lifter=22.0, dither=0.0, energy_floor=1.0,
               frame_length=25.0, frame_shift=10.0, high_freq=0.0, htk_compat=False, low_freq=20.0, num_ceps=13, num_mel_bins=23,
               preemphasis_coefficient=0.97, raw_energy=True, remove_dc_offset=True, round_to_power_of_two=True, snip_edges=True,
               subtract_mean=False, use_energy=False, vtln_warp=1.0, window_type="povey", scale=1.0, layout="frames", device=None,
               *, transform="direct"):
    """torchaudio.compliance.kaldi.mfcc(waveform, ...) in one pass on the device: as kaldi_fbank, -> [..., F, num_ceps] (1 <=
    num_ceps <= num_mel_bins). Column 0 is C0, or the log energy with use_energy; htk_compat moves it to the end, and where
    it is C0 (no use_energy) it leaves there as sqrt(2) C0, as in Kaldi and torchaudio."""
    if isinstance(num_ceps, bool) or int(num_ceps) != num_ceps or int(num_ceps) < 1:
        raise ValueError("num_ceps is an integer in [1, num_mel_bins]")
    return _kaldi(waveform, sample_frequency, frame_length, frame_shift, subtract_mean, device, transform, num_mel_bins=num_mel_bins,
                  num_ceps=num_ceps, round_to_power_of_two=round_to_power_of_two, snip_edges=snip_edges,
                  remove_dc_offset=remove_dc_offset, window_type=window_type, use_log_fbank=True, use_energy=use_energy,
                  raw_energy=raw_energy, htk_compat=htk_compat, use_power=True, layout=layout,
                  preemphasis_coefficient=preemphasis_coefficient, blackman_coeff=blackman_coeff, low_freq=low_freq,
                  high_freq=high_freq, energy_floor=energy_floor, scale=scale, cepstral_lifter=cepstral_lifter, dither=dither,
                  vtln_warp=vtln_warp)


# ---- FeatureNorm (new: CMVN, max-clamp, affine and masked padding behind the feature passes, per-row lengths) -----------
class NormConfig(ctypes.Structure):
    """alacgpu_norm_config (include/alacgpu.h)."""

    _fields_ = [("bins", ctypes.c_uint32), ("stat", ctypes.c_uint32), ("var_floor", ctypes.c_float), ("range", ctypes.c_float),
                ("pad_value", ctypes.c_float)]


class NormInfo(ctypes.Structure):
    """alacgpu_norm_info (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_uint32) for k in ("bins", "stat", "tile_frames", "lds_bytes", "shift_entries", "scale_entries")] + [
        ("scratch_bytes", ctypes.c_uint64), ("scratch_address", ctypes.c_uint64)]


_NORM_STATS = {None: 0, "none": 0, "mean": 1, "mean_var": 2, "max": 3}


def _norm_table(v, bins, name):
    """shift / scale: None, a number (every bin's) or bins numbers -> None or a float32 array [bins]"""
    if v is None:
        return None
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    a = np.asarray(v, dtype=np.float32)
    if a.ndim == 0:
        a = np.full(bins, a, np.float32)
    if a.shape != (bins,):
        raise ValueError("%s is a number or %d numbers" % (name, bins))
    return np.ascontiguousarray(a)


class FeatureNorm(_FeaturePass):
    """float32 features with per-row lengths -> normalised features with the padding masked, on one MI355X (include/alacgpu.h:
    alacgpu_norm_*). Per row over its first n = clamp(lengths, 0, frames) frames: stat "mean" subtracts each bin's mean,
    "mean_var" also multiplies by 1 / sqrt(max(variance, var_floor)) (Kaldi's apply-cmvn --norm-vars), "max" clamps below (the
    row's maximum over bins and frames) - range, "none" / None does nothing; then (x - shift) * scale where given (a number or
    bins numbers each: global CMVN, or Whisper's shift -4, scale 0.25); then pad_value in every frame from n on, whatever the
    input holds there. The sums run in a fixed order, so the result is the same bits for every batch size and for
    both layouts. ValueError, before any HIP call, for bins outside [1, 4096], an unknown stat, var_floor <= 0, or "max" without
    a range >= 0. Single-caller, bound to one device and one stream. out_frames(F) is F."""

    _CREATE, _DESTROY, _OUT_FRAMES = "alacgpu_norm_create", "alacgpu_norm_destroy", "alacgpu_norm_out_frames"
    _LAST_MS, _SYNCHRONIZE = "alacgpu_norm_last_ms", "alacgpu_norm_synchronize"

    def __init__(self, bins, stat="mean", shift=None, scale=None, var_floor=1e-20, range=None, pad_value=0.0, device=0):
        super().__init__()
        if isinstance(bins, bool) or int(bins) != bins or not 0 <= int(bins) <= 0xFFFFFFFF:
            raise ValueError("bins is an integer in [1, 4096]")
        if not (stat is None or isinstance(stat, str)) or stat not in _NORM_STATS:
            raise ValueError("stat is 'none', 'mean', 'mean_var' or 'max', not %r" % (stat,))
        if _NORM_STATS[stat] == 3 and range is None:
            raise ValueError("stat 'max' needs a range >= 0")
        self.bins, self.stat = int(bins), stat or "none"
        self.config = NormConfig(self.bins, _NORM_STATS[stat], float(var_floor), 0.0 if range is None else float(range), float(pad_value))
        self.shift, self.scale = _norm_table(shift, self.bins, "shift"), _norm_table(scale, self.bins, "scale")
        self._create(device, ctypes.byref(self.config), None if self.shift is None else self.shift.ctypes.data,
                     None if self.scale is None else self.scale.ctypes.data)

    def norm_device(self, d_in, in_strides, rows, frames, d_lengths, d_out, out_strides, d_stats=0, sync=True):
        """alacgpu_norm_device: raw device pointers (ints; d_lengths and d_stats may be 0), in_strides / out_strides the (row,
        frame, bin) strides in elements, one of the two inner ones 1. Exactly the rows x frames x bins elements of the output
        are written; d_out may be d_in with the same strides. Runs on the handle's stream, which does not order against
        torch's: synchronize the input first."""
        _check(self._lib.alacgpu_norm_device(self._h, d_in, *[int(s) for s in in_strides], rows, frames, d_lengths or None, d_out,
                                             *[int(s) for s in out_strides], d_stats or None, 1 if sync else 0))

    def plan(self):
        """alacgpu_norm_plan -> dict: bins, stat, tile_frames (the frames of a chunk of the sums), lds_bytes, scratch_bytes and
        scratch_address (the handle's block for the chunks' partial results as it stands: a second pass of a shape changes
        neither), and shift / scale as float32 [bins], or None."""
        info = NormInfo()
        shift, scale = _fetch_plan(self._lib.alacgpu_norm_plan, self._h, info, lambda i: np.zeros(i.shift_entries, np.float32),
                                   lambda i: np.zeros(i.scale_entries, np.float32))
        out = {k: int(getattr(info, k)) for k in ("bins", "stat", "tile_frames", "lds_bytes", "scratch_bytes", "scratch_address")}
        out.update(shift=shift if info.shift_entries else None, scale=scale if info.scale_entries else None)
        return out

    def __call__(self, feats, lengths=None, layout="frames", out=None, return_stats=False):
        """A float32 tensor [..., F, bins] (layout "frames", the Kaldi pass's default) or [..., bins, F] ("bins": its other
        layout and the spectrogram pass's) -> the normalised tensor of the same shape on the handle's device. It works on the
        tensor's own strides, views such as logmel[..., :-1] included, where one inner stride is 1 and the leading dimensions
        flatten without a copy; anything else is made contiguous first. lengths: None (every frame is valid) or one integer
        per row of the leading dimensions, the count of its valid FRAMES (kaldi_frame_counts); int32 on the device as
        load_clips returns them is used in place. out: None for a new contiguous tensor, or a float32 tensor of feats' shape on
        the device, feats itself for in place. return_stats: also the statistics [..., 2, bins] (alacgpu_norm_device).
        ValueError for another dtype, a last-but-one / last dimension that is not bins, or lengths of another count."""
        import torch
        if layout not in _FBANK_LAYOUTS:
            raise ValueError("layout is 'frames' or 'bins', not %r" % (layout,))
        dev, lead, rows, frames = self._features(feats, layout)
        same = out is feats
        if same and feats.device != dev:
            raise ValueError("in place needs feats on the handle's device")
        if out is not None and not same:
            if not isinstance(out, torch.Tensor) or out.dtype is not torch.float32 or out.shape != feats.shape or out.device != dev:
                raise ValueError("out must be a float32 tensor of feats' shape on the handle's device")
        x = feats.to(dev)
        xv, xs = _feature_rows(x, rows, layout)
        if xv is None:
            if same:
                raise ValueError("in place needs a tensor whose rows flatten without a copy and whose frame or bin stride is 1")
            xv, xs = _feature_rows(x.contiguous(), rows, layout)
        if same:
            result, ov, os_ = feats, xv, xs
        else:
            result = torch.empty(feats.shape, dtype=torch.float32, device=dev) if out is None else out
            ov, os_ = _feature_rows(result, rows, layout)
            if ov is None:
                raise ValueError("out needs rows that flatten without a copy and a frame or bin stride of 1")
        ln = self._lengths(lengths, rows, dev)
        stats = torch.empty((rows, 2, self.bins), dtype=torch.float32, device=dev) if return_stats else None
        if rows and frames:
            torch.cuda.synchronize(dev)  # the handle's stream does not order against torch's
            self.norm_device(xv.data_ptr(), xs, rows, frames, 0 if ln is None else ln.data_ptr(), ov.data_ptr(), os_,
                             stats.data_ptr() if return_stats else 0, sync=True)
        elif return_stats:
            stats.zero_()
        return (result, stats.reshape(lead + (2, self.bins))) if return_stats else result


def NewFeatureNorm(bins, stat="mean", shift=None, scale=None, var_floor=1e-20, range=None, pad_value=0.0, device=0):
    """A FeatureNorm (context manager); ValueError where no plan can be built."""
    return FeatureNorm(bins, stat, shift, scale, var_floor, range, pad_value, device)


_NORMS = {}  # (device, bins, stat, var_floor, range, pad_value, the bytes of shift and of scale) -> FeatureNorm


def normalize_features(feats, lengths=None, stat="mean", layout="frames", shift=None, scale=None, var_floor=1e-20, range=None,
                       pad_value=0.0, out=None, return_stats=False, device=None):
    """FeatureNorm(bins, stat, ...)(feats, lengths, layout, out, return_stats) with the handle of a (device, parameter set) made
    once and kept: feats a float32 tensor [..., F, bins] (layout "frames") or [..., bins, F] ("bins") on cuda:`device` (default:
    the tensor's own, cuda:0 for a CPU tensor, which is uploaded). shift / scale enter the key by their bytes."""
    bins, device = _feature_input(feats, layout, device)
    sh, sc = _norm_table(shift, bins, "shift"), _norm_table(scale, bins, "scale")
    if not (stat is None or isinstance(stat, str)):
        raise ValueError("stat is 'none', 'mean', 'mean_var' or 'max', not %r" % (stat,))
    key = (device, bins, stat or "none", float(var_floor), None if range is None else float(range), float(pad_value),
           None if sh is None else sh.tobytes(), None if sc is None else sc.tobytes())
    norm = _cached(_NORMS, key, lambda: FeatureNorm(bins, stat, sh, sc, var_floor, range, pad_value, device))
    return norm(feats, lengths, layout, out, return_stats)


def kaldi_frame_counts(lengths, frame_length, frame_shift, snip_edges=True):
    """Per-row sample counts (a tensor of integers, as load_clips' lengths) -> the int32 tensor of the frames that Kaldi's
    framing gives a row of that many samples, frame_length / frame_shift in samples: KaldiFeatures.out_frames for every value:
    1 + (T - W) // h with snip_edges, (T + h // 2) // h without, 0 for T < W. With snip_edges the first out_frames(T) frames of a
    row that is zero-padded behind its T samples are the frames of the row cut to T, bit for bit: frame f reads the samples
    [f h, f h + W) only. Without snip_edges that holds for every frame but the last few, which read up to W / 2 - h / 2 samples
    behind T: they see the padding's zeros where Kaldi would reflect. And a lengths of load_clips is a count, not a prefix, where
    a short packet lies in front of a file's last: the samples it counts are then not the row's first."""
    import torch
    W, h = int(frame_length), int(frame_shift)
    if W < 1 or h < 1:
        raise ValueError("frame_length and frame_shift are positive sample counts")
    if not isinstance(lengths, torch.Tensor):
        lengths = torch.as_tensor(np.asarray(lengths))
    if lengths.dtype.is_floating_point:
        raise ValueError("lengths holds integers")
    T = lengths.to(torch.int64)
    n = 1 + torch.div(T - W, h, rounding_mode="floor") if snip_edges else torch.div(T + h // 2, h, rounding_mode="floor")
    return torch.where(T >= W, n, torch.zeros_like(n)).to(torch.int32)


# ---- FrameStack (new: deltas, context splicing and subsampling behind the normalisation, per-row lengths) ----------------
class StackConfig(ctypes.Structure):
    """alacgpu_stack_config (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_uint32) for k in ("bins", "order", "window", "left", "right", "stride")] + [("pad_value", ctypes.c_float)]


class StackInfo(ctypes.Structure):
    """alacgpu_stack_info (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_uint32) for k in ("bins", "order", "window", "left", "right", "stride", "columns", "tile_out", "tile_in",
                                               "tile_bins", "lds_bytes", "w1_entries", "w2_entries")]


def _stack_int(v, name, lo, hi):
    if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError("%s is an integer in [%d, %d], not %r" % (name, lo, hi, v))
    return int(v)


class FrameStack(_FeaturePass):
    """float32 features with per-row lengths -> their deltas, spliced context and subsampling in one pass on one MI355X, with
    lengths of their own (include/alacgpu.h: alacgpu_stack_*). Per row over its first n = clamp(lengths, 0, frames)
    frames: d_0 = x, d_k = the delta features of order k <= order with Kaldi's weights (the ramp -window .. window over sum j^2,
    convolved k times), every frame index clamped to [0, n - 1]: the row's own first and last valid frame are replicated, never
    the padding behind them. Output frame g < m = ceil(n / stride) holds, for c = 0 .. left + right, the d_0 .. d_order of frame
    clamp(g * stride + c - left, 0, n - 1), bins each: (left + right + 1) * (order + 1) * bins columns; the frames from m on are
    pad_value. Order 1 is torchaudio.functional.compute_deltas(mode="replicate") with win_length = 2 * window + 1; order 2 is
    Kaldi's add-deltas, with one clamp on x, and not compute_deltas applied twice (which clamps the deltas at the edges again).
    order 0 is splice-feats, the stride alone subsample-feats, left (m - 1) // 2, right m - 1 - left, stride n FunASR's
    apply_lfr(m, n). Each delta is one chain of float32 fused multiply-adds in tap order, so the bits depend on the row's own data
    and n only: not on the batch, nor on either layout. ValueError, before any HIP call, for bins outside [1, 4096], order outside
    [0, 2], window outside [1, 8] with an order above 0, left or right outside [0, 16], stride outside [1, 64], or more than 4096
    columns. Single-caller, bound to one device and one stream. out_frames(F) is ceil(F / stride)."""

    _CREATE, _DESTROY, _OUT_FRAMES = "alacgpu_stack_create", "alacgpu_stack_destroy", "alacgpu_stack_out_frames"
    _LAST_MS, _SYNCHRONIZE = "alacgpu_stack_last_ms", "alacgpu_stack_synchronize"

    def __init__(self, bins, order=0, window=2, left=0, right=0, stride=1, pad_value=0.0, device=0):
        super().__init__()
        self.bins, self.order = _stack_int(bins, "bins", 1, 4096), _stack_int(order, "order", 0, 2)
        self.window = _stack_int(window, "window", 1, 8) if self.order else 0
        self.left, self.right = _stack_int(left, "left", 0, 16), _stack_int(right, "right", 0, 16)
        self.stride = _stack_int(stride, "stride", 1, 64)
        self.columns = (self.left + self.right + 1) * (self.order + 1) * self.bins
        self.config = StackConfig(self.bins, self.order, self.window, self.left, self.right, self.stride, float(pad_value))
        self._create(device, ctypes.byref(self.config))

    def stack_device(self, d_in, in_strides, rows, frames, d_lengths, d_out, out_strides, d_out_lengths=0, sync=True):
        """alacgpu_stack_device: raw device pointers (ints; d_lengths and d_out_lengths may be 0), in_strides / out_strides the
        (row, frame, bin) strides in elements, one of the two inner ones 1 in each. Exactly the rows x out_frames(frames) x columns
        elements of the output and the rows out lengths are written; the output may not overlap the input. Runs on the handle's
        stream, which does not order against torch's: synchronize the input first."""
        _check(self._lib.alacgpu_stack_device(self._h, d_in, *[int(s) for s in in_strides], rows, frames, d_lengths or None, d_out,
                                              *[int(s) for s in out_strides], d_out_lengths or None, 1 if sync else 0))

    def plan(self):
        """alacgpu_stack_plan -> dict: the parameters, columns, tile_out (the output frames of a tile), tile_in (the input frames it
        stages at most), tile_bins, lds_bytes, and w1 / w2: the delta weights as float32 [2 window + 1] / [4 window + 1], or
        None above the order."""
        info = StackInfo()
        (w,) = _fetch_plan(self._lib.alacgpu_stack_plan, self._h, info, lambda i: np.zeros(i.w1_entries + i.w2_entries, np.float32))
        out = {k: int(getattr(info, k)) for k, _ in StackInfo._fields_ if not k.endswith("_entries")}
        out.update(w1=w[:info.w1_entries] if info.w1_entries else None, w2=w[info.w1_entries:] if info.w2_entries else None)
        return out

    def __call__(self, feats, lengths=None, layout="frames", out=None, out_layout=None):
        """A float32 tensor [..., F, bins] (layout "frames") or [..., bins, F] ("bins") -> (y, out_lengths): y [..., G, columns]
        (out_layout "frames") or [..., columns, G] ("bins"; default: layout) with G = out_frames(F), new and contiguous or `out`,
        and out_lengths int32 [...] on the device, ceil(n / stride) per row. feats is used on its own strides, views such as
        feats[..., :-1] included, under FeatureNorm's rule: one inner stride is 1 and the leading dimensions flatten without a
        copy; anything else is made contiguous first. lengths: None (every frame is valid) or one integer per row, the count of
        its valid frames. out: a float32 tensor of y's shape on the device that shares no memory with feats. ValueError for
        another dtype, a bins dimension that is not the handle's, or lengths of another count."""
        import torch
        out_layout = layout if out_layout is None else out_layout
        if layout not in _FBANK_LAYOUTS or out_layout not in _FBANK_LAYOUTS:
            raise ValueError("layout and out_layout are 'frames' or 'bins', not %r / %r" % (layout, out_layout))
        dev, lead, rows, frames = self._features(feats, layout)
        G = -(-frames // self.stride)
        oshape = lead + ((G, self.columns) if out_layout == "frames" else (self.columns, G))
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype is not torch.float32 or tuple(out.shape) != oshape or
                                out.device != dev):
            raise ValueError("out must be a float32 tensor of shape %r on the handle's device" % (oshape,))
        x = feats.to(dev)
        xv, xs = _feature_rows(x, rows, layout)
        if xv is None:
            xv, xs = _feature_rows(x.contiguous(), rows, layout)
        y = torch.empty(oshape, dtype=torch.float32, device=dev) if out is None else out
        yv, ys = _feature_rows(y, rows, out_layout)
        if yv is None:
            raise ValueError("out needs rows that flatten without a copy and a frame or bin stride of 1")
        ln = self._lengths(lengths, rows, dev)
        out_len = torch.zeros(rows, dtype=torch.int32, device=dev)
        if rows and frames:
            torch.cuda.synchronize(dev)  # the handle's stream does not order against torch's
            self.stack_device(xv.data_ptr(), xs, rows, frames, 0 if ln is None else ln.data_ptr(), yv.data_ptr(), ys,
                              out_len.data_ptr(), sync=True)
        return y, out_len.reshape(lead)


def NewFrameStack(bins, order=0, window=2, left=0, right=0, stride=1, pad_value=0.0, device=0):
    """A FrameStack (context manager); ValueError where no plan can be built."""
    return FrameStack(bins, order, window, left, right, stride, pad_value, device)


_STACKS = {}  # (device, bins, order, window, left, right, stride, pad_value) -> FrameStack


def stack_frames(feats, lengths=None, order=0, window=2, left=0, right=0, stride=1, layout="frames", pad_value=0.0, out=None,
                 out_layout=None, device=None):
    """FrameStack(bins, order, ...)(feats, lengths, layout, out, out_layout) -> (y, out_lengths) with the handle of a (device,
    parameter set) made once and kept: feats a float32 tensor [..., F, bins] (layout "frames") or [..., bins, F] ("bins") on
    cuda:`device` (default: the tensor's own, cuda:0 for a CPU tensor, which is uploaded)."""
    bins, device = _feature_input(feats, layout, device)
    order = _stack_int(order, "order", 0, 2)
    key = (device, bins, order, _stack_int(window, "window", 1, 8) if order else 0, _stack_int(left, "left", 0, 16),
           _stack_int(right, "right", 0, 16), _stack_int(stride, "stride", 1, 64), np.float32(pad_value).tobytes())
    st = _cached(_STACKS, key, lambda: FrameStack(bins, order, window, left, right, stride, pad_value, device))
    return st(feats, lengths, layout, out, out_layout)


def add_deltas(feats, lengths=None, order=2, window=2, layout="frames", **kw):
    """Kaldi's add-deltas: stack_frames(feats, lengths, order=order, window=window, layout=layout, ...) -> (y with (order + 1) *
    bins columns: the features, their deltas and delta-deltas; out_lengths = the lengths). 13 MFCCs give the usual 39."""
    return stack_frames(feats, lengths, order=order, window=window, layout=layout, **kw)


def lfr(feats, lengths=None, m=7, n=6, layout="frames", **kw):
    """FunASR's low-frame-rate stacking apply_lfr(m, n) per row: m frames stacked every n frames, the first frame replicated
    (m - 1) // 2 times in front and the row's own last valid frame behind: stack_frames with left (m - 1) // 2, right m - 1 -
    left, stride n -> (y with m * bins columns, out_lengths = ceil(lengths / n)). 80 bins at 7 / 6 give Paraformer's 560."""
    m = _stack_int(m, "m", 1, 33)
    left = (m - 1) // 2
    return stack_frames(feats, lengths, left=left, right=m - 1 - left, stride=n, layout=layout, **kw)


# ---- SpecAugment (new: time warp, frequency and time masks inside each row's own frames, between normalisation and stacking) ----
class SpecAugConfig(ctypes.Structure):
    """alacgpu_specaug_config (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_uint32) for k in ("bins", "freq_masks", "freq_width", "time_masks", "time_width", "time_ratio_q16",
                                               "warp")] + [("mask_value", ctypes.c_float), ("pad_value", ctypes.c_float)]


class SpecAugInfo(ctypes.Structure):
    """alacgpu_specaug_info (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_uint32) for k in ("bins", "freq_masks", "freq_width", "time_masks", "time_width", "time_ratio_q16", "warp",
                                               "draws", "tile_out", "lds_bytes")] + [("mask_value", ctypes.c_float),
                                                                                     ("pad_value", ctypes.c_float)]


def _specaug_ratio(time_ratio):
    """time_ratio in [0, 1] -> round(time_ratio * 65536)"""
    if isinstance(time_ratio, bool) or not isinstance(time_ratio, (int, float)) or not 0.0 <= time_ratio <= 1.0:
        raise ValueError("time_ratio is a number in [0, 1], not %r" % (time_ratio,))
    return int(round(time_ratio * 65536))


def _specaug_u64(v, name):
    if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < 1 << 64:
        raise ValueError("%s is an integer in [0, 2^64), not %r" % (name, v))
    return int(v)


class SpecAugment(_FeaturePass):
    """float32 features with per-row lengths -> SpecAugment on one MI355X (include/alacgpu.h: alacgpu_specaug_*).
    Per row over its first n = clamp(lengths, 0, frames) frames: a time warp (warp > 0 and n > 2 warp: a centre c in [warp, n - warp)
    moves to w in [c - warp + 1, c + warp]; the frames before and behind it are resampled linearly, each segment on its own, as
    ESPnet's time_warp does with bicubic weights), then freq_masks frequency masks of a width drawn from [0, freq_width] and
    time_masks time masks of a width drawn from [0, min(time_width, time_ratio * n)], all drawn inside the row's own n frames; an
    element under any mask is mask_value, every frame from n on pad_value, whatever the input holds there. The random words are
    Philox4x32-10 keyed by `seed` at a counter made of the row's identity (ids[r], or row_base + r), so an utterance's
    augmentation depends on (seed, identity, n) only: not on its place in the batch, nor on the rows around it. The draws are
    integer arithmetic and the warp one subtraction and one fused multiply-add per element, so the bits are the same for both
    layouts. ValueError, before any HIP call, for bins outside [1, 4096], freq_masks outside [0, 8], freq_width outside [0, bins],
    time_masks outside [0, 16], time_width outside [0, 65535], time_ratio outside [0, 1] or warp outside [0, 256]. Single-caller,
    bound to one device and one stream. out_frames(F) is F."""

    _CREATE, _DESTROY = "alacgpu_specaug_create", "alacgpu_specaug_destroy"
    _LAST_MS, _SYNCHRONIZE = "alacgpu_specaug_last_ms", "alacgpu_specaug_synchronize"

    def __init__(self, bins, freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=1.0, warp=0, mask_value=0.0,
                 pad_value=0.0, device=0):
        super().__init__()
        self.bins = _stack_int(bins, "bins", 1, 4096)
        self.freq_masks, self.freq_width = _stack_int(freq_masks, "freq_masks", 0, 8), _stack_int(freq_width, "freq_width", 0, self.bins)
        self.time_masks, self.time_width = _stack_int(time_masks, "time_masks", 0, 16), _stack_int(time_width, "time_width", 0, 65535)
        self.time_ratio_q16, self.warp = _specaug_ratio(time_ratio), _stack_int(warp, "warp", 0, 256)
        self.draws = 2 + 2 * self.freq_masks + 2 * self.time_masks
        self.config = SpecAugConfig(self.bins, self.freq_masks, self.freq_width, self.time_masks, self.time_width, self.time_ratio_q16,
                                    self.warp, float(mask_value), float(pad_value))
        self._create(device, ctypes.byref(self.config))

    def out_frames(self, in_frames):
        """in_frames itself: the pass keeps every frame; 0 on a closed handle."""
        return int(in_frames) if self._h else 0

    def specaug_device(self, d_in, in_strides, rows, frames, d_lengths, seed, d_out, out_strides, row_base=0, d_ids=0, d_draws=0,
                       sync=True):
        """alacgpu_specaug_device: raw device pointers (ints; d_lengths, d_ids and d_draws may be 0), in_strides / out_strides the
        (row, frame, bin) strides in elements, one of the two inner ones 1 in each. Exactly the rows x frames x bins elements of
        the output and the rows x draws int32 of d_draws are written; the output may not overlap the input, but on a handle
        without a warp it may be the input itself with the same strides. Runs on the handle's stream, which does not order
        against torch's: synchronize the input first."""
        _check(self._lib.alacgpu_specaug_device(self._h, d_in, *[int(s) for s in in_strides], rows, frames, d_lengths or None,
                                                _specaug_u64(seed, "seed"), _specaug_u64(row_base, "row_base"), d_ids or None, d_out,
                                                *[int(s) for s in out_strides], d_draws or None, 1 if sync else 0))

    def plan(self):
        """alacgpu_specaug_plan -> dict: the parameters, draws (the random words and resolved draws of a row), tile_out (the
        output frames of a tile, a function of bins alone) and lds_bytes."""
        info = SpecAugInfo()
        _check(self._lib.alacgpu_specaug_plan(self._h, ctypes.byref(info)))
        return {k: (float if k.endswith("_value") else int)(getattr(info, k)) for k, _ in SpecAugInfo._fields_}

    def __call__(self, feats, lengths=None, seed=0, ids=None, row_base=0, layout="frames", out=None, out_layout=None,
                 return_draws=False):
        """A float32 tensor [..., F, bins] (layout "frames") or [..., bins, F] ("bins") -> the augmented tensor [..., F, bins]
        (out_layout "frames") or [..., bins, F] ("bins"; default: layout), new and contiguous or `out`. feats is used on its own
        strides, views such as feats[..., :-1] included, under FeatureNorm's rule; anything else is made contiguous first.
        lengths: None (every frame is valid) or one integer per row, the count of its valid frames. seed: the step's, a uint64.
        ids: None, or one int64 per row, the utterance's identity; without it row r of the flattened leading dimensions is
        row_base + r. out: a float32 tensor of the result's shape on the device that shares no memory with feats, or, on a handle
        without a warp and with out_layout the layout, feats itself for in place. return_draws: also the resolved draws, int32
        [..., draws]: c, w, then (start, width) per mask, frequency masks first: what a caller needs to mask targets alike.
        ValueError for another dtype, a bins dimension that is not the handle's, lengths or ids of another count."""
        import torch
        out_layout = layout if out_layout is None else out_layout
        if layout not in _FBANK_LAYOUTS or out_layout not in _FBANK_LAYOUTS:
            raise ValueError("layout and out_layout are 'frames' or 'bins', not %r / %r" % (layout, out_layout))
        seed, row_base = _specaug_u64(seed, "seed"), _specaug_u64(row_base, "row_base")
        dev, lead, rows, frames = self._features(feats, layout)
        oshape = lead + ((frames, self.bins) if out_layout == "frames" else (self.bins, frames))
        same = out is feats
        if same and (self.warp or out_layout != layout or feats.device != dev):
            raise ValueError("in place needs a handle without a warp, one layout and feats on the handle's device")
        if out is not None and not same and (not isinstance(out, torch.Tensor) or out.dtype is not torch.float32 or
                                             tuple(out.shape) != oshape or out.device != dev):
            raise ValueError("out must be a float32 tensor of shape %r on the handle's device" % (oshape,))
        x = feats.to(dev)
        xv, xs = _feature_rows(x, rows, layout)
        if xv is None:
            if same:
                raise ValueError("in place needs a tensor whose rows flatten without a copy and whose frame or bin stride is 1")
            xv, xs = _feature_rows(x.contiguous(), rows, layout)
        if same:
            y, yv, ys = feats, xv, xs
        else:
            y = torch.empty(oshape, dtype=torch.float32, device=dev) if out is None else out
            yv, ys = _feature_rows(y, rows, out_layout)
            if yv is None:
                raise ValueError("out needs rows that flatten without a copy and a frame or bin stride of 1")
        ln = self._lengths(lengths, rows, dev)
        idv = None
        if ids is not None:
            idv = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
            if idv.numel() != rows or idv.dtype.is_floating_point or idv.dtype is torch.bool:
                raise ValueError("ids holds one integer per row: %d, not %d" % (rows, idv.numel()))
            idv = idv.to(dev, torch.int64).contiguous().reshape(rows)
        draws = torch.zeros((rows, self.draws), dtype=torch.int32, device=dev) if return_draws else None
        if rows and frames:
            torch.cuda.synchronize(dev)  # the handle's stream does not order against torch's
            self.specaug_device(xv.data_ptr(), xs, rows, frames, 0 if ln is None else ln.data_ptr(), seed, yv.data_ptr(), ys, row_base,
                                0 if idv is None else idv.data_ptr(), draws.data_ptr() if return_draws else 0, sync=True)
        return (y, draws.reshape(lead + (self.draws,))) if return_draws else y


def NewSpecAugment(bins, freq_masks=2, freq_width=27, time_masks=2, time_width=100, time_ratio=1.0, warp=0, mask_value=0.0,
                   pad_value=0.0, device=0):
    """A SpecAugment (context manager); ValueError where no plan can be built."""
    return SpecAugment(bins, freq_masks, freq_width, time_masks, time_width, time_ratio, warp, mask_value, pad_value, device)


_SPECAUGS = {}  # (device, bins, freq_masks, freq_width, time_masks, time_width, time_ratio_q16, warp, mask_value, pad_value) -> SpecAugment
_NO_SEED = object()


def spec_augment(feats, lengths=None, seed=_NO_SEED, ids=None, row_base=0, freq_masks=2, freq_width=27, time_masks=2, time_width=100,
                 time_ratio=1.0, warp=0, mask_value=0.0, pad_value=0.0, layout="frames", out=None, out_layout=None, return_draws=False,
                 device=None):
    """SpecAugment(bins, freq_masks, ...)(feats, lengths, seed, ids, row_base, layout, out, out_layout, return_draws) with the
    handle of a (device, parameter set) made once and kept: feats a float32 tensor [..., F, bins] (layout "frames") or [..., bins,
    F] ("bins") on cuda:`device` (default: the tensor's own, cuda:0 for a CPU tensor, which is uploaded). seed is required: a
    default would give every training step the same masks."""
    if seed is _NO_SEED:
        raise ValueError("spec_augment needs a seed: the step's, so that no two steps draw the same masks")
    bins, device = _feature_input(feats, layout, device)
    bins = _stack_int(bins, "bins", 1, 4096)
    key = (device, bins, _stack_int(freq_masks, "freq_masks", 0, 8), _stack_int(freq_width, "freq_width", 0, bins),
           _stack_int(time_masks, "time_masks", 0, 16), _stack_int(time_width, "time_width", 0, 65535), _specaug_ratio(time_ratio),
           _stack_int(warp, "warp", 0, 256), np.float32(mask_value).tobytes(), np.float32(pad_value).tobytes())
    sa = _cached(_SPECAUGS, key, lambda: SpecAugment(bins, freq_masks, freq_width, time_masks, time_width, time_ratio, warp, mask_value,
                                                     pad_value, device))
    return sa(feats, lengths, seed, ids, row_base, layout, out, out_layout, return_draws)


# ---- WaveAugment (new: gain, noise from a bank at an SNR and dither per row, between load_clips and the feature pass) ----
class WaveAugConfig(ctypes.Structure):
    """alacgpu_waveaug_config (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_int32) for k in ("snr_lo_q8", "snr_hi_q8", "gain_lo_q8", "gain_hi_q8")] + [
        ("noise_prob_q16", ctypes.c_uint32), ("dither", ctypes.c_float), ("clamp", ctypes.c_uint32), ("pad_value", ctypes.c_float)]


class WaveAugInfo(ctypes.Structure):
    """alacgpu_waveaug_info (include/alacgpu.h)."""

    _fields_ = [(k, ctypes.c_int32) for k in ("snr_lo_q8", "snr_hi_q8", "gain_lo_q8", "gain_hi_q8")] + [
        (k, ctypes.c_uint32) for k in ("noise_prob_q16", "clamp", "tile", "draws", "snr_entries", "gain_entries", "lds_bytes")] + [
        ("dither", ctypes.c_float), ("pad_value", ctypes.c_float), ("reserved", ctypes.c_uint32),
        ("scratch_bytes", ctypes.c_uint64), ("scratch_address", ctypes.c_uint64)]


def _waveaug_range(db, name):
    """(lo, hi) in dB -> (round(lo * 256), round(hi * 256)), each within +-64 dB, in order and at most 64 dB apart"""
    try:
        lo, hi = db
        lo, hi = int(round(float(lo) * 256)), int(round(float(hi) * 256))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s is (lo, hi) in dB, not %r" % (name, db))
    if not (-16384 <= lo <= hi <= 16384 and hi - lo <= 16384):
        raise ValueError("%s is (lo, hi) within [-64, 64] dB, lo <= hi <= lo + 64, not %r" % (name, db))
    return lo, hi


def _waveaug_config(snr, gain, noise_prob, dither, clamp, pad_value):
    """The keywords -> the fields of a WaveAugConfig; ValueError for what alacgpu_waveaug_create refuses"""
    if isinstance(noise_prob, bool) or not isinstance(noise_prob, (int, float)) or not 0.0 <= noise_prob <= 1.0:
        raise ValueError("noise_prob is a number in [0, 1], not %r" % (noise_prob,))
    if isinstance(dither, bool) or not isinstance(dither, (int, float)) or not 0.0 <= dither < float("inf"):
        raise ValueError("dither is a finite number >= 0, not %r" % (dither,))
    if not isinstance(clamp, (bool, int)) or clamp not in (0, 1):
        raise ValueError("clamp is True or False, not %r" % (clamp,))
    return (*_waveaug_range(snr, "snr"), *_waveaug_range(gain, "gain"), int(round(noise_prob * 65536)), float(np.float32(dither)),
            int(clamp), float(np.float32(pad_value)))


def _wave_rows(t, rows):
    """[..., T] -> ([rows, T] without a copy, the row stride in elements), or (None, None) where the rows do not flatten or the
    samples are not contiguous"""
    T = int(t.shape[-1])
    try:
        v = t.view(rows, T) if t.ndim != 2 else t
    except RuntimeError:
        return None, None
    if not v.numel():
        return v, max(T, 1)
    rs = T if rows == 1 else int(v.stride(0))
    if (T > 1 and v.stride(1) != 1) or rs < T:
        return None, None
    return v, rs


class WaveAugment(_RowPass):
    """float32 waveforms [..., T] with per-row lengths -> gain, noise at an SNR, dither, clamp and padding on one MI355X
    (include/alacgpu.h: alacgpu_waveaug_*). Per row over its first n = clamp(lengths, 0, T) samples: y = a x + b z +
    dither g, where a is a gain drawn from `gain` (dB, in steps of 1 / 256 dB), z the samples of a clip k of the noise bank from a
    drawn offset on, looping, b = sqrt(Ex / En) 10^(-snr / 20) a with the SNR drawn from `snr` and both energies taken over the
    row's own n samples, in a share noise_prob of the rows, and g an approximately normal variate per sample (Irwin-Hall of
    eight 16-bit words, unit variance, cut at 4.9 sigma; added to the waveform once, not per frame as Kaldi does). Every sample
    from n on is pad_value, whatever the input holds there. The random words are Philox4x32-10 keyed by `seed` at a counter made
    of the row's identity (ids[r], or row_base + r) and a stream number apart from SpecAugment's, so an utterance's augmentation
    depends on (seed, identity, n) and the bank only: not on its place in the batch, nor on the rows around it. With gain (0, 0),
    no noise, no dither and no clamp a sample is 1.0 * x: its own bits, but a signalling NaN comes out quiet. ValueError, before
    any HIP call, for a range outside [-64, 64] dB, out of order or more than 64 dB wide, noise_prob outside [0, 1], a dither
    that is negative or not finite. Single-caller, bound to one device and one stream. out_frames(T) is T."""

    _CREATE, _DESTROY = "alacgpu_waveaug_create", "alacgpu_waveaug_destroy"
    _LAST_MS, _SYNCHRONIZE = "alacgpu_waveaug_last_ms", "alacgpu_waveaug_synchronize"

    def __init__(self, snr=(5, 20), gain=(0, 0), noise_prob=1.0, dither=0.0, clamp=False, pad_value=0.0, device=0):
        super().__init__()
        self.config = WaveAugConfig(*_waveaug_config(snr, gain, noise_prob, dither, clamp, pad_value))
        self._create(device, ctypes.byref(self.config))

    def out_frames(self, in_frames):
        """in_frames itself: the pass keeps every sample; 0 on a closed handle."""
        return int(in_frames) if self._h else 0

    def waveaug_device(self, d_in, in_row_stride, rows, samples, d_lengths, seed, d_out, out_row_stride, d_noise=0, noise_row_stride=0,
                       noise_rows=0, noise_samples=0, d_noise_lengths=0, row_base=0, d_ids=0, d_draws=0, d_stats=0, sync=True):
        """alacgpu_waveaug_device: raw device pointers (ints; d_lengths, d_noise, d_noise_lengths, d_ids, d_draws and d_stats may be
        0), strides in elements. Exactly the rows x samples elements of the output, the rows x 5 int32 of d_draws and the rows x
        4 floats of d_stats are written; the output may be the input itself with the same stride and may not overlap it
        otherwise, nor the bank. Runs on the handle's stream, which does not order against torch's: synchronize the input first."""
        _check(self._lib.alacgpu_waveaug_device(self._h, d_in, int(in_row_stride), rows, samples, d_lengths or None, d_noise or None,
                                                int(noise_row_stride), noise_rows, noise_samples, d_noise_lengths or None,
                                                _specaug_u64(seed, "seed"), _specaug_u64(row_base, "row_base"), d_ids or None, d_out,
                                                int(out_row_stride), d_draws or None, d_stats or None, 1 if sync else 0))

    def plan(self):
        """alacgpu_waveaug_plan -> dict: the parameters, tile (the samples of a chunk of the energy sums), draws (5), lds_bytes,
        the scratch block as it stands, and the two tables snr_amp and gain_amp (float32 numpy arrays)."""
        info = WaveAugInfo()
        snr, gain = _fetch_plan(self._lib.alacgpu_waveaug_plan, self._h, info, lambda i: np.zeros(i.snr_entries, np.float32),
                                lambda i: np.zeros(i.gain_entries, np.float32))
        out = {k: (float if k in ("dither", "pad_value") else int)(getattr(info, k)) for k, _ in WaveAugInfo._fields_ if k != "reserved"}
        out.update(snr_amp=snr, gain_amp=gain)
        return out

    def __call__(self, clips, lengths=None, seed=0, noise=None, noise_lengths=None, ids=None, row_base=0, out=None, return_draws=False,
                 return_stats=False):
        """A float32 tensor or numpy array [..., T] -> the augmented tensor [..., T] on the handle's device, new and contiguous or
        `out`. A tensor whose leading dimensions flatten without a copy and whose samples are contiguous is used on its own row
        stride (clips[:, 0] of load_clips' [B, channels, L] included); anything else is made contiguous first. lengths: None
        (every sample is valid) or one integer per row. seed: the step's, a uint64. noise: None, or a float32 bank [N, Tn] with
        noise_lengths (None, or one integer per clip). ids: None, or one int64 per row, the utterance's identity; without it row
        r of the flattened leading dimensions is row_base + r. out: a float32 tensor of clips' shape on the device, which may be
        clips itself (in place) and may not share memory with it otherwise, nor with the bank. return_draws: also int32 [..., 5]:
        applied, k, o, the SNR and the gain in 1 / 256 dB. return_stats: also float32 [..., 4]: Ex, En, a, b."""
        import torch
        if not self._h:
            raise ValueError("the handle is closed")
        _float32_input(clips)
        seed, row_base = _specaug_u64(seed, "seed"), _specaug_u64(row_base, "row_base")
        dev = torch.device("cuda", self.device)
        same = out is clips
        if same and (not isinstance(clips, torch.Tensor) or clips.device != dev):
            raise ValueError("in place needs a tensor on the handle's device")
        x = (torch.from_numpy(np.ascontiguousarray(clips)) if isinstance(clips, np.ndarray) else clips).to(dev)
        lead, T = tuple(x.shape[:-1]), int(x.shape[-1])
        rows = int(np.prod(lead, dtype=np.int64))
        if out is not None and not same and (not isinstance(out, torch.Tensor) or out.dtype is not torch.float32 or
                                             tuple(out.shape) != tuple(x.shape) or out.device != dev):
            raise ValueError("out must be a float32 tensor of shape %r on the handle's device" % (tuple(x.shape),))
        xv, xs = _wave_rows(x, rows)
        if xv is None:
            if same:
                raise ValueError("in place needs a tensor whose rows flatten without a copy and whose samples are contiguous")
            xv, xs = _wave_rows(x.contiguous(), rows)
        if same:
            y, yv, ys = clips, xv, xs
        else:
            y = torch.empty(tuple(x.shape), dtype=torch.float32, device=dev) if out is None else out
            yv, ys = _wave_rows(y, rows)
            if yv is None:
                raise ValueError("out needs rows that flatten without a copy and contiguous samples")
        ln = _FeaturePass._lengths(lengths, rows, dev)
        nz, nzs, nl = None, 0, None
        if noise is not None:
            _float32_input(noise)
            nz = (torch.from_numpy(np.ascontiguousarray(noise)) if isinstance(noise, np.ndarray) else noise).to(dev)
            if nz.ndim != 2:
                raise ValueError("noise is a float32 bank [N, Tn]")
            nv, nzs = _wave_rows(nz, int(nz.shape[0]))
            if nv is None:
                nz = nz.contiguous()
                nv, nzs = _wave_rows(nz, int(nz.shape[0]))
            nl = _FeaturePass._lengths(noise_lengths, int(nz.shape[0]), dev)
        elif noise_lengths is not None:
            raise ValueError("noise_lengths without a noise bank")
        idv = None
        if ids is not None:
            idv = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
            if idv.numel() != rows or idv.dtype.is_floating_point or idv.dtype is torch.bool:
                raise ValueError("ids holds one integer per row: %d, not %d" % (rows, idv.numel()))
            idv = idv.to(dev, torch.int64).contiguous().reshape(rows)
        draws = torch.zeros((rows, 5), dtype=torch.int32, device=dev) if return_draws else None
        stats = torch.zeros((rows, 4), dtype=torch.float32, device=dev) if return_stats else None
        if rows and T:
            torch.cuda.synchronize(dev)  # the handle's stream does not order against torch's
            has_bank = nz is not None and nz.numel() > 0
            self.waveaug_device(xv.data_ptr(), xs, rows, T, 0 if ln is None else ln.data_ptr(), seed, yv.data_ptr(), ys,
                                nz.data_ptr() if has_bank else 0, nzs, int(nz.shape[0]) if has_bank else 0,
                                int(nz.shape[1]) if has_bank else 0, 0 if nl is None or not has_bank else nl.data_ptr(), row_base,
                                0 if idv is None else idv.data_ptr(), draws.data_ptr() if return_draws else 0,
                                stats.data_ptr() if return_stats else 0, sync=True)
        res = (y,) + ((draws.reshape(lead + (5,)),) if return_draws else ()) + ((stats.reshape(lead + (4,)),) if return_stats else ())
        return res if len(res) > 1 else y


def NewWaveAugment(snr=(5, 20), gain=(0, 0), noise_prob=1.0, dither=0.0, clamp=False, pad_value=0.0, device=0):
    """A WaveAugment (context manager); ValueError where no plan can be built."""
    return WaveAugment(snr, gain, noise_prob, dither, clamp, pad_value, device)


_WAVEAUGS = {}  # (device, the eight fields of the configuration) -> WaveAugment


def augment_waveform(clips, lengths=None, seed=_NO_SEED, noise=None, noise_lengths=None, snr=(5, 20), noise_prob=1.0, gain=(0, 0),
                     dither=0.0, clamp=False, pad_value=0.0, ids=None, row_base=0, out=None, return_draws=False, return_stats=False,
                     device=None):
    """WaveAugment(snr, gain, ...)(clips, lengths, seed, noise, noise_lengths, ids, row_base, out, return_draws, return_stats) with
    the handle of a (device, parameter set) made once and kept: clips a float32 tensor [..., T] on cuda:`device` (default: the
    tensor's own, cuda:0 for a CPU tensor or a numpy array, which is uploaded). seed is required: a default would give every
    training step the same noise."""
    if seed is _NO_SEED:
        raise ValueError("augment_waveform needs a seed: the step's, so that no two steps draw the same noise")
    _float32_input(clips)
    _, device = _on_device(clips, device)
    fields = _waveaug_config(snr, gain, noise_prob, dither, clamp, pad_value)
    key = (device,) + fields[:5] + (np.float32(fields[5]).tobytes(), fields[6], np.float32(fields[7]).tobytes())
    wa = _cached(_WAVEAUGS, key, lambda: WaveAugment(snr, gain, noise_prob, dither, clamp, pad_value, device))
    return wa(clips, lengths, seed, noise, noise_lengths, ids, row_base, out, return_draws, return_stats)


def load_features(sources, frame_offsets, num_frames, sample_rate=16000, kind="fbank", norm="mean", channel=0, transform="direct",
                  device=0, deltas=0, delta_window=2, context=(0, 0), subsample=1, augment=None, wave_augment=None, **kaldi_kwargs):
    """Files to normalised features in one call: load_clips(sources, frame_offsets, num_frames, sample_rate=sample_rate) -> the
    channel `channel` -> kaldi_fbank (kind "fbank") or kaldi_mfcc ("mfcc") with kaldi_kwargs (torchaudio's names; frames layout)
    -> kaldi_frame_counts of load_clips' lengths -> FeatureNorm(stat=norm: "mean", "mean_var" or None, which only masks).
    -> (feats [B, F, D], frame_lengths int32 [B], sample_rate): row j's first frame_lengths[j] frames are normalised over
    themselves, the frames behind them are 0. Nothing but that composition; its two limits are kaldi_frame_counts'.
    With deltas (0..2, delta_window frames each side), context (left, right) or subsample other than their defaults, stack_frames
    runs behind the normalisation, which is Kaldi's order: feats is [B, ceil(F / subsample), (left + right + 1) * (deltas + 1) * D]
    and frame_lengths its out_lengths. With the defaults that pass is not run.
    augment: None, or a dict of spec_augment's keywords that must hold `seed` (and may hold ids, row_base, the mask and warp
    parameters, mask_value): SpecAugment runs between the normalisation and the stacking, so its masks fall on the
    features' own bins and frames, and behind norm "mean" a mask_value of 0 is the row's mean. With None nothing runs.
    wave_augment: None, or a dict of augment_waveform's keywords that must hold `seed` (and may hold noise, noise_lengths, snr,
    noise_prob, gain, dither, clamp, ids, row_base): the waveform augmentation runs on the chosen channel over load_clips'
    lengths, in front of the feature pass, with a pad_value of 0, which the feature pass relies on. With None nothing runs."""
    try:
        left, right = context
    except (TypeError, ValueError):
        raise ValueError("context is (left, right), not %r" % (context,))
    if augment is not None:
        if not isinstance(augment, dict) or "seed" not in augment:
            raise ValueError("augment is a dict of spec_augment's keywords that holds 'seed'")
        for k in ("feats", "lengths", "layout", "out", "out_layout", "return_draws", "device", "pad_value"):
            if k in augment:
                raise ValueError("%s is not a key of augment" % k)
    if wave_augment is not None:
        if not isinstance(wave_augment, dict) or "seed" not in wave_augment:
            raise ValueError("wave_augment is a dict of augment_waveform's keywords that holds 'seed'")
        for k in ("clips", "lengths", "out", "return_draws", "return_stats", "device", "pad_value"):
            if k in wave_augment:
                raise ValueError("%s is not a key of wave_augment" % k)
    stacked = (_stack_int(deltas, "deltas", 0, 2), _stack_int(left, "context left", 0, 16), _stack_int(right, "context right", 0, 16),
               _stack_int(subsample, "subsample", 1, 64)) != (0, 0, 0, 1)
    if kind not in ("fbank", "mfcc"):
        raise ValueError("kind is 'fbank' or 'mfcc', not %r" % (kind,))
    if not (norm is None or isinstance(norm, str)) or norm not in (None, "mean", "mean_var"):
        raise ValueError("norm is 'mean', 'mean_var' or None, not %r" % (norm,))
    for k in ("layout", "subtract_mean", "sample_frequency", "device"):
        if k in kaldi_kwargs:
            raise ValueError("%s is not an argument of load_features" % k)
    clips, lengths, rate = load_clips(sources, frame_offsets, num_frames, device=device, sample_rate=sample_rate)
    if not 0 <= int(channel) < clips.shape[1]:
        raise ValueError("channel %d of %d" % (channel, clips.shape[1]))
    wave = clips[:, int(channel)]
    if wave_augment is not None:
        wave = augment_waveform(wave, lengths, device=device, **wave_augment)
    feats = (kaldi_fbank if kind == "fbank" else kaldi_mfcc)(wave, sample_frequency=rate, device=device, transform=transform,
                                                            **kaldi_kwargs)
    W = int(rate * kaldi_kwargs.get("frame_length", 25.0) * 0.001)
    h = int(rate * kaldi_kwargs.get("frame_shift", 10.0) * 0.001)
    counts = kaldi_frame_counts(lengths, W, h, kaldi_kwargs.get("snip_edges", True))
    feats = normalize_features(feats, counts, stat=norm, out=feats, device=device)
    if augment is not None:
        feats = spec_augment(feats, counts, device=device, **augment)
    if stacked:
        feats, counts = stack_frames(feats, counts, order=deltas, window=delta_window, left=left, right=right, stride=subsample,
                                     device=device)
    return feats, counts, rate


def NewDecoder(source, device=0, window=1024):
    """NewDecoder (decode.go:50-76): streaming façade over the batch path, see stream.py."""
    from . import stream
    return stream.NewDecoder(source, device=device, window=window)


def load(source, device=0, dtype=None, frame_offset=0, num_frames=-1, sample_rate=None):
    """An ALAC M4A/MP4 file -> (waveform [channels, frames], sample_rate), the call shape of torchaudio.load: a planar
    torch tensor on cuda:`device`, float32 in [-1, 1) (dtype=torch.int32: the integer samples). source: a path, a binary file
    object, or the file's bytes. The track is found and configured as NewDecoder does it (ErrNoTrack / ErrConfig); the packets
    are decoded and converted on the device in windows of 48 MB of PCM into one tensor, and the first packet that fails
    raises the ErrDecode that Read raises when it gets there.
    frame_offset / num_frames, as in torchaudio.load: the frames [frame_offset, frame_offset + num_frames) of the file, fewer
    when it ends before (none, [channels, 0], when it ends at or before frame_offset); num_frames = -1: up to the end. Only
    the packets that cover those frames are decoded — packets are independent — and the frames are cut out of them on the
    device (PacketDecoder.decode_clips); a failed packet outside the range is not noticed.
    sample_rate: the rate wanted. Where the file's differs, what the call gives without it is resampled on the device
    (resample(): torchaudio's sinc_interp_hann) and sample_rate is the rate returned; frame_offset and num_frames stay in the
    file's own frames, as in torchaudio.load. float32 only: with dtype=torch.int32 it raises ValueError."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    if sample_rate is None:
        return _load_file(source, device, dtype, frame_offset, num_frames)
    if dtype is not torch.float32:
        raise ValueError("sample_rate needs float32 samples: only those are resampled")
    if int(sample_rate) != sample_rate or sample_rate <= 0:
        raise ValueError("sample_rate must be a positive integer")
    wave, rate = _load_file(source, device, dtype, frame_offset, num_frames)
    return resample(wave, rate, int(sample_rate), device=device), int(sample_rate)


def _load_file(source, device, dtype, frame_offset, num_frames):
    """load() at the file's own rate."""
    import torch
    from . import stream
    frame_offset, num_frames = int(frame_offset), int(num_frames)
    if frame_offset < 0 or num_frames < -1:
        raise ValueError("frame_offset must be >= 0 and num_frames >= -1")
    if frame_offset or num_frames != -1:
        return _load_range(source, device, dtype, frame_offset, num_frames)
    _, view, track, cfg = stream.open_track(source)
    raw = np.frombuffer(view, dtype=np.uint8)
    offs, sizes = track.offsets.astype(np.int64), track.sizes.astype(np.int64)
    n, fl, ch = len(sizes), int(cfg.FrameLength), int(cfg.NumChannels)
    lost = np.nonzero(offs + sizes > raw.size)[0]
    n_ok = int(lost[0]) if len(lost) else n
    dev = torch.device("cuda", device)
    with NewPacketDecoder(cfg, device) as dec:
        window = stream.window_packets(dec.frame_bytes)
        dec.reserve(min(window, max(1, n_ok)))
        wave = torch.empty((ch, max(n_ok * fl, 1)), dtype=dtype, device=dev)
        total = 0
        for w0 in range(0, n_ok, window):
            w1 = min(w0 + window, n_ok)
            lo, hi = int(offs[w0:w1].min()), int((offs[w0:w1] + sizes[w0:w1]).max())
            part, _, status = dec._decode_waveform(raw[lo:hi], offs[w0:w1] - lo, sizes[w0:w1], "stream", dtype, into=(wave, total))
            bad = torch.nonzero(status)
            if bad.numel():
                k = int(bad[0].item())
                e = status_error(int(status[k].item()))
                raise ErrDecode("decoding packet %d: %s" % (w0 + k, e), status=e.status, sentinel=e.sentinel)
            total += part.shape[1]
    if n_ok < n:
        raise AlacError("reading sample %d: unexpected EOF" % n_ok)
    return wave[:, :total], int(cfg.SampleRate)


def _load_range(source, device, dtype, frame_offset, num_frames):
    """load() of the frames [frame_offset, frame_offset + num_frames): the covering packets in windows, one clip per window
    gathered straight into the result. Frame k of the file is taken to be frame k % FrameLength of packet k // FrameLength,
    which holds when every packet but the file's last is full, as encoders write them; a covering packet in front of the
    last that turns out short raises AlacError (the full load() closes such a gap up, so the frames behind it have other
    numbers there)."""
    import torch
    from . import stream
    if dtype not in (torch.float32, torch.int32):
        raise ValueError("dtype must be torch.float32 or torch.int32")
    _, view, track, cfg = stream.open_track(source)
    raw = np.frombuffer(view, dtype=np.uint8)
    offs, sizes = track.offsets.astype(np.int64), track.sizes.astype(np.int64)
    n, fl, ch = len(sizes), int(cfg.FrameLength), int(cfg.NumChannels)
    lost = np.nonzero(offs + sizes > raw.size)[0]
    n_ok = int(lost[0]) if len(lost) else n
    stop = n * fl if num_frames < 0 else min(n * fl, frame_offset + num_frames)  # the last frame the packets could hold, + 1
    p0, p1 = frame_offset // fl, -(-stop // fl)
    dev = torch.device("cuda", device)
    if p0 >= p1 or stop <= frame_offset:
        return torch.empty((ch, 0), dtype=dtype, device=dev), int(cfg.SampleRate)
    p1_ok = min(p1, n_ok)
    cap = stop - frame_offset
    wave = torch.empty((ch, cap), dtype=dtype, device=dev)
    total = 0
    with NewPacketDecoder(cfg, device) as dec:
        window = stream.window_packets(dec.frame_bytes)
        dec.reserve(min(window, max(1, p1_ok - p0)))
        col = 0
        for w0 in range(p0, p1_ok, window):
            w1 = min(w0 + window, p1_ok)
            first = max(frame_offset, w0 * fl)
            L = min(stop, w1 * fl) - first
            lo, hi = int(offs[w0:w1].min()), int((offs[w0:w1] + sizes[w0:w1]).max())
            _, valid, _, frames, status = dec._decode_clips(raw[lo:hi], offs[w0:w1] - lo, sizes[w0:w1], [first - w0 * fl], None, L,
                                                            dtype, dest=(wave, col, cap, ch * cap))
            bad = torch.nonzero(status)
            if bad.numel():
                k = int(bad[0].item())
                e = status_error(int(status[k].item()))
                raise ErrDecode("decoding packet %d: %s" % (w0 + k, e), status=e.status, sentinel=e.sentinel)
            short = torch.nonzero(frames[:min(w1, n - 1) - w0] != fl)
            if short.numel():
                k = int(short[0].item())
                raise AlacError("packet %d holds %d of %d frames and is not the file's last: frame offsets behind it are not "
                                "packet arithmetic" % (w0 + k, int(frames[k].item()), fl))
            total = col + int(valid[0].item())  # the file's last packet may be short
            col += L
    if p1_ok < p1:
        raise AlacError("reading sample %d: unexpected EOF" % n_ok)
    return wave[:, :total], int(cfg.SampleRate)


def _clip_batch(tracks, starts, first, count, fl):
    """One decode's worth of load_clips: for clip j the byte range of its covering packets — count[j] packets from first[j]
    on of tracks[j] = (file bytes, packet offsets, packet sizes, config) — appended to one host blob, the packets' offsets and
    sizes in it, and the clip's descriptors on the grid of slots -> (blob, offsets, sizes, begin, limit). Every covering
    packet must lie inside its file's bytes (load_clips checks that first): a range that left them would be cut short here
    and the packet's bytes would run into the next clip's."""
    parts, p_offs, p_sizes, begin, limit, at, slot = [], [], [], [], [], 0, 0
    for j, (raw, offs, sizes, _) in enumerate(tracks):
        begin.append(slot * fl + starts[j] % fl)
        if count[j]:
            o, z = offs[first[j]:first[j] + count[j]], sizes[first[j]:first[j] + count[j]]
            lo, hi = int(o.min()), int((o + z).max())
            if lo < 0 or hi > raw.size:
                raise AlacError("clip %d: its packets leave the file's %d bytes" % (j, raw.size))
            piece = raw[lo:hi]
            parts.append(piece)
            p_offs.append(o - lo + at)
            p_sizes.append(z)
            at += piece.size
            slot += count[j]
        limit.append(slot)
    blob = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    offsets = np.concatenate(p_offs) if p_offs else np.zeros(0, np.int64)
    sz = np.concatenate(p_sizes) if p_sizes else np.zeros(0, np.int64)
    return blob, offsets, sz, begin, limit


def load_clips(sources, frame_offsets, num_frames, device=0, dtype=None, sample_rate=None):
    """Fixed-length crops of many ALAC M4A/MP4 files as one batch -> (clips [B, channels, num_frames], lengths [B], sample_rate):
    clip j is the frames [frame_offsets[j], frame_offsets[j] + num_frames) of sources[j], a planar torch tensor on
    cuda:`device`, float32 in [-1, 1) or int32 as load() gives them. Frames behind a file's end are zero, and lengths
    (int32, on the device) says how many of a clip's frames are the file's. sources: paths, binary file objects or the files'
    bytes; the same object or an equal path may repeat and is opened and parsed once. All tracks must agree in FrameLength,
    BitDepth, NumChannels, PB / MB / KB / MaxRun and SampleRate (ErrConfig names the first source that differs).
    Only the packets that cover a clip are read, and all of them go through one upload, one decode and one gather
    (batches above a window of 48 MB of PCM are split between clips); a failed packet raises ErrDecode with the clip and
    the packet's index in its file, and a covering packet that lies outside its file's bytes (a truncated file) raises
    load()'s "unexpected EOF" with the clip in front, before anything is decoded. As in load(frame_offset, num_frames),
    frame k of a file is frame k % FrameLength of packet k // FrameLength; a short packet in front of a file's last leaves
    zeros in the clips that cover it, and their lengths count the samples, not a prefix.
    sample_rate = R: the clips at that rate, from sources whose SampleRate may differ (every other field must still agree).
    frame_offsets[j] stays in source j's own frames; num_frames = L counts frames at R. The sources are grouped by their rate
    r, and each group takes one decode, one gather of Ls = ceil(L * r / R) source frames per clip (L where r = R) and one
    resample() (torchaudio's sinc_interp_hann), of whose ceil(Ls * R / r) >= L columns the first L are kept; lengths[j] =
    min(L, ceil(valid * R / r)) for the valid source frames of clip j. The filter sees zeros in front of a clip's first frame and
    behind its last, not the file's neighbouring frames: exactly what cropping and then resampling gives with torchaudio.
    float32 only (dtype=torch.int32 raises ValueError); returns (clips, lengths, R)."""
    import torch
    from . import stream
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.int32):
        raise ValueError("dtype must be torch.float32 or torch.int32")
    if sample_rate is not None:
        if dtype is not torch.float32:
            raise ValueError("sample_rate needs float32 samples: only those are resampled")
        if int(sample_rate) != sample_rate or sample_rate <= 0:
            raise ValueError("sample_rate must be a positive integer")
    sources = list(sources)
    starts = [int(a) for a in frame_offsets]
    L = int(num_frames)
    if not sources or len(starts) != len(sources):
        raise ValueError("sources and frame_offsets must have the same length, at least 1")
    if L < 1 or any(a < 0 for a in starts):
        raise ValueError("num_frames must be >= 1 and every frame offset >= 0")
    opened, tracks = {}, []
    for src in sources:
        key = ("path", os.fspath(src)) if isinstance(src, (str, os.PathLike)) else ("object", id(src))
        if key not in opened:
            _, view, track, cfg = stream.open_track(src)
            opened[key] = (np.frombuffer(view, dtype=np.uint8), track.offsets.astype(np.int64), track.sizes.astype(np.int64), cfg)
        tracks.append(opened[key])
    cfg = tracks[0][3]
    same = ("FrameLength", "BitDepth", "NumChannels", "PB", "MB", "KB", "MaxRun") + (("SampleRate",) if sample_rate is None else ())
    for j, t in enumerate(tracks):
        for name in same:
            if getattr(t[3], name) != getattr(cfg, name):
                raise ErrConfig("source %d: %s %d differs from the first source's %d" % (j, name, getattr(t[3], name), getattr(cfg, name)))
    ids = list(range(len(sources)))
    if sample_rate is None:
        clips, lengths = _gather_clips(tracks, starts, ids, L, device, dtype)
        return clips, lengths, int(cfg.SampleRate)
    R = int(sample_rate)
    dev = torch.device("cuda", device)
    clips = torch.empty((len(sources), int(cfg.NumChannels), L), dtype=dtype, device=dev)
    lengths = torch.empty(len(sources), dtype=torch.int32, device=dev)
    for r in sorted({int(t[3].SampleRate) for t in tracks}):
        if r <= 0:
            raise ErrConfig("a source's SampleRate is 0")
        own = [j for j in ids if int(tracks[j][3].SampleRate) == r]
        Ls = L if r == R else -(-L * r // R)
        part, valid = _gather_clips([tracks[j] for j in own], [starts[j] for j in own], own, Ls, device, dtype)
        at = torch.tensor(own, dtype=torch.int64, device=dev)
        if r == R:
            clips[at], lengths[at] = part, valid
        else:
            clips[at] = resample(part, r, R, device=device)[:, :, :L]
            lengths[at] = torch.clamp((valid.to(torch.int64) * R + (r - 1)) // r, max=L).to(torch.int32)
    return clips, lengths, R


def _gather_clips(tracks, starts, ids, L, device, dtype):
    """load_clips for sources of one configuration (tracks[0]'s): clip k, known to the caller as clip ids[k], is L frames of
    tracks[k] from starts[k] on -> (clips [B, channels, L], lengths [B])."""
    import torch
    from . import stream
    cfg = tracks[0][3]
    fl, ch, B = int(cfg.FrameLength), int(cfg.NumChannels), len(tracks)
    # the covering packets of clip j: [first[j], first[j] + count[j]) of its file
    first = [a // fl for a in starts]
    count = [max(0, min(-(-(a + L) // fl), len(t[2])) - p) for a, p, t in zip(starts, first, tracks)]
    for j, (raw, offs, sizes, _) in enumerate(tracks):
        cover = slice(first[j], first[j] + count[j])
        lost = np.nonzero(offs[cover] + sizes[cover] > raw.size)[0]
        if len(lost):
            raise AlacError("clip %d: reading sample %d: unexpected EOF" % (ids[j], first[j] + int(lost[0])))
    dev = torch.device("cuda", device)
    clips = torch.empty((B, ch, L), dtype=dtype, device=dev)
    lengths = torch.empty(B, dtype=torch.int32, device=dev)
    with NewPacketDecoder(cfg, device) as dec:
        window = stream.window_packets(dec.frame_bytes)
        groups, j0, held = [], 0, 0  # batches of whole clips, each at most a window of packets (or one clip)
        for j in range(B):
            if j > j0 and held + count[j] > window:
                groups.append((j0, j))
                j0, held = j, 0
            held += count[j]
        groups.append((j0, B))
        dec.reserve(max(1, max(sum(count[a:b]) for a, b in groups)))
        for a, b in groups:
            blob, offsets, sz, begin, limit = _clip_batch(tracks[a:b], starts[a:b], first[a:b], count[a:b], fl)
            _, valid, cstat, _, status = dec._decode_clips(blob, offsets, sz, begin, limit, L, dtype,
                                                           dest=(clips, a * ch * L, L, ch * L))
            bad = torch.nonzero(cstat)
            if bad.numel():
                k = int(bad[0].item())
                s0 = limit[k] - count[a + k]
                i = int(torch.nonzero(status[s0:limit[k]])[0].item())
                e = status_error(int(status[s0 + i].item()))
                raise ErrDecode("clip %d: decoding packet %d: %s" % (ids[a + k], first[a + k] + i, e), status=e.status, sentinel=e.sentinel)
            lengths[a:b] = valid
    return clips, lengths


def save(dest, wave, sample_rate, bits_per_sample=16, frame_length=4096, device=0, _window=None, **_container):
    """A waveform [channels, frames] -> an ALAC M4A file, the call shape of torchaudio.save. dest: a path or a binary file
    object. wave: a torch tensor on any device or a numpy array, float32 in [-1, 1) or int32 (the integers load(dtype=
    torch.int32) gives). Returns how many samples were saturated or NaN. The waveform is quantised, packed and encoded on
    cuda:`device` in packet-aligned windows of 48 MB of PCM on one encoder handle (packets are independent, so the file equals a
    one-shot encode); the cookie is taken after the last window, so that its largest packet and bit rate cover the file."""
    import torch
    from . import mp4, stream
    if isinstance(wave, np.ndarray):
        if wave.ndim != 2:
            raise ValueError("wave must be [channels, frames]")
        ch, total = int(wave.shape[0]), int(wave.shape[1])
    elif isinstance(wave, torch.Tensor):
        if wave.dim() != 2:
            raise ValueError("wave must be [channels, frames]")
        ch, total = int(wave.shape[0]), int(wave.shape[1])
    else:
        raise ValueError("wave must be a torch tensor or a numpy array")
    cfg = PacketConfig(FrameLength=frame_length, BitDepth=bits_per_sample, NumChannels=ch, SampleRate=sample_rate)
    blobs, sizes, clipped = [], [], 0
    with NewPacketEncoder(cfg, device) as enc:
        window = _window or stream.window_packets(frame_length * enc.bytes_per_frame)
        for f0 in range(0, total, window * frame_length):
            f1 = min(f0 + window * frame_length, total)
            blob, offs, c = enc.encode_waveform(wave[:, f0:f1], "stream")
            blobs.append(blob.cpu().numpy())
            sizes.append(np.diff(offs.cpu().numpy()))
            clipped += c
        cookie = enc.cookie()
    offsets = np.zeros(1 + sum(len(s) for s in sizes), np.uint64)
    if len(offsets) > 1:
        offsets[1:] = np.cumsum(np.concatenate(sizes))
    data = mp4.write_m4a(cookie, np.concatenate(blobs) if blobs else np.zeros(0, np.uint8), offsets, total, sample_rate, ch,
                         bits_per_sample, **_container)
    if hasattr(dest, "write"):
        dest.write(data)
    else:
        with open(os.fspath(dest), "wb") as f:
            f.write(data)
    return clipped


def FindALACTrack(data):
    """internal/mp4 FindALACTrack (mp4.go:233-298) on a file in memory -> mp4.Track (cookie, offsets, sizes)."""
    from . import mp4
    return mp4.find_alac_track(data)
