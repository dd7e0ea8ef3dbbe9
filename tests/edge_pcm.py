"""Deterministic edge-case PCM for the encoder and decoder tests (a plain helper module, not a conftest).

Every generator is `f(synth, cfg, total_frames, seed=0)` -> int32 [frames][channels] in the PCM domain of cfg.bit_depth, the
format of test_encoder_host.make_pcm, so that synth.pack_pcm packs it. Signals that are laid out per packet (the clicks and
the run ladder) restart at every multiple of cfg.frame_length, because every packet is encoded on its own.

The spacings of RUN_LADDER are in the residual domain: the encoder's predictor smears a lone click over the next few
residuals (CLICK_TAIL of them; pinned by the trace checks of test_encoder_edges.py), so a gap of D frames between two clicks
leaves D - CLICK_TAIL zero residuals behind the first one."""
import numpy as np

SHIFT = {16: 0, 20: 0, 24: 1, 32: 2}

# residuals from a click up to the start of the zero run behind it (the click's code, two more codes and the short runs of
# the predictor's response; measured with oracle.goref's trace on the encoder's packets)
CLICK_TAIL = 10
MAX_RUN = 65535  # the longest zero run one run code carries (golomb.go:243)
RUN_ESC_M3 = 27  # a run code with m = 3 (k 2, the run behind a click) is escaped from 9 * 3 on
RUN_ESC_M255 = 2295  # ... and with m = 255 (k 8, the run behind a full run, where the mean is 0) from 9 * 255 on

# frame length of the run ladder: long enough for 131 071 zero residuals behind a click and the click that ends them
LADDER_FL = 131090
# click positions of the ladder's packets (packet p takes LADDER[p % 7]). Zero residuals behind a click at c, up to the next
# click at c + D: D - CLICK_TAIL. A stretch of L >= 65 535 is one full run, one code (mean 0, zmode 0) and a run of
# L - 65 536 with m = 255; behind the last click the run reaches the chain's last sample.
LADDER = [
    (0, 65544, 65580, 65617),  # 65 534 (one short of the cap), then runs of 26 and 27 (a run code either side of its escape)
    (0, 65545),  # 65 535: a full run ended by a click, no code between them
    (0, 65546),  # 65 536: a full run, a code, an empty run
    (0, 65536 + 10 + RUN_ESC_M255 - 1),  # a full run, a code, 2 294 with m = 255 (the last run code that is not escaped)
    (0, 65536 + 10 + RUN_ESC_M255),  # ... and 2 295 (the first escaped one)
    (0, 131080),  # 131 070: a full run, a code, 65 534
    (0, 131081),  # 131 071: two full runs in one chain with a code between them
]
# the zero-run lengths (in the trace's run codes) the ladder promises: packet -> runs that must occur in that order
LADDER_RUNS = [
    [65534, 26, 27],
    [65535],
    [65535, 0],
    [65535, RUN_ESC_M255 - 1],
    [65535, RUN_ESC_M255],
    [65535, 65534],
    [65535, 65535],
]


def _top(depth):
    return 1 << (depth - 1)


def _click(depth):
    """the smallest value that reaches the chain: one above the shift bytes"""
    return 1 << (8 * SHIFT[depth])


def _zeros(cfg, total):
    return np.zeros((total, cfg.num_channels), np.int64)


def _done(pcm):
    return np.ascontiguousarray(pcm, dtype=np.int64).astype(np.int32)


def silence(synth, cfg, total, seed=0):
    """digital silence: at frame_length 65 536 one run of exactly 65 535 that ends on the chain's last sample"""
    return _done(_zeros(cfg, total))


def _per_packet(cfg, total, positions_of):
    pcm = _zeros(cfg, total)
    fl = cfg.frame_length
    for p in range(-(-total // fl)):
        m = min(fl, total - p * fl)
        for c in positions_of(p, m):
            if 0 <= c < m:
                pcm[p * fl + c, 0] = _click(cfg.bit_depth)
    return pcm


def click_first(synth, cfg, total, seed=0):
    """one click on channel 0 at every packet's first frame: the run behind it is cut off by the chain's end"""
    return _done(_per_packet(cfg, total, lambda p, m: [0]))


def click_last(synth, cfg, total, seed=0):
    """one click on channel 0 at every packet's last frame: the run in front of it ends one sample early, and no run is
    entered behind it (i + 1 < n)"""
    return _done(_per_packet(cfg, total, lambda p, m: [m - 1]))


def run_ladder(synth, cfg, total, seed=0):
    """the clicks of LADDER on every channel (a stereo pair has the ladder in its U chain and silence in its V chain)"""
    pcm = _per_packet(cfg, total, lambda p, m: LADDER[p % len(LADDER)])
    pcm[:, 1:] = pcm[:, :1]
    return _done(pcm)


def dual_mono(synth, cfg, total, seed=0):
    """L == R == ... == a MUSIC signal: mono content stored as stereo, a difference chain with no non-zero residual"""
    mono = synth.signal(synth_cfg(synth, cfg, 1), synth.PROFILE_MUSIC, 1000 + seed, total) if total else np.zeros((0, 1))
    return _done(np.repeat(np.asarray(mono, np.int64).reshape(-1, 1), cfg.num_channels, axis=1))


def synth_cfg(synth, cfg, channels):
    from oracle import oracle
    return oracle.make_config(max(cfg.frame_length, 1), cfg.bit_depth, channels)


def dc_max(synth, cfg, total, seed=0):
    """every sample at positive full scale"""
    return _done(_zeros(cfg, total) + (_top(cfg.bit_depth) - 1))


def dc_min(synth, cfg, total, seed=0):
    """every sample at negative full scale"""
    return _done(_zeros(cfg, total) - _top(cfg.bit_depth))


def nyquist_full(synth, cfg, total, seed=0):
    """+full / -full scale from frame to frame (channel c starts with the sign of c)"""
    t = np.arange(total)[:, None] + np.arange(cfg.num_channels)[None, :]
    top = _top(cfg.bit_depth)
    return _done(np.where(t % 2 == 0, top - 1, -top))


def antiphase_full(synth, cfg, total, seed=0):
    """pairs (0, 1), (2, 3), ... in anti-phase at full scale, R = -L - 1: a full-scale sine in even packets, L = max / R = min
    constants in odd ones. The difference chain V = L - R of a pair then needs chanBits = depth - 8 * shift + 1 bits."""
    top = _top(cfg.bit_depth)
    fl = max(cfg.frame_length, 1)
    t = np.arange(total)
    s = np.floor((top - 0.5) * np.sin(2 * np.pi * t / 37.3 + 0.1 * seed)).astype(np.int64)
    s = np.clip(s, -top, top - 1)
    even = (t // fl) % 2 == 0
    left = np.where(even, s, top - 1)
    pcm = _zeros(cfg, total)
    for c in range(cfg.num_channels):
        pcm[:, c] = left if c % 2 == 0 else -left - 1
    return _done(pcm)


def bursts(synth, cfg, total, seed=0):
    """silence broken by bursts of 1..12 frames of full-scale noise every 97..600 frames: escape codes right after a zero
    run (zmode 1) and residuals above 0xffff where the chain is wider than 16 bits (the mean clamp)"""
    rng = np.random.default_rng(4242 + seed)
    top = _top(cfg.bit_depth)
    pcm = _zeros(cfg, total)
    pos = int(rng.integers(20, 200))
    while pos < total:
        n = int(rng.integers(1, 13))
        pcm[pos:pos + n] = rng.integers(-top, top, size=(min(n, total - pos), cfg.num_channels))
        pos += n + int(rng.integers(97, 601))
    return _done(pcm)


def low_byte_only(synth, cfg, total, seed=0):
    """samples within +-2^(8 * shift - 1): the chains above the shift bytes hold only 0 and -1 and the shift block carries
    everything (at 16 / 20 bits, without shift bytes, the samples are 0 and -1)"""
    rng = np.random.default_rng(99 + seed)
    half = 1 << max(8 * SHIFT[cfg.bit_depth] - 1, 0)
    lo = -half if SHIFT[cfg.bit_depth] else -1
    hi = half if SHIFT[cfg.bit_depth] else 1
    return _done(rng.integers(lo, hi, size=(total, cfg.num_channels)))


SIGNALS = {f.__name__: f for f in (silence, click_first, click_last, run_ladder, dual_mono, dc_max, dc_min, nyquist_full,
                                   antiphase_full, bursts, low_byte_only)}


def make(name, synth, cfg, total, seed=0):
    return SIGNALS[name](synth, cfg, total, seed)
