"""Packet sets for the chunk pipeline of the wave workgroups (alac_duo.h: the queue's buffer numbering, the lags of the
predictor and writer roles, the tails, and the int16-wrap countdown): shared by tests/test_gpu_chunk_pipeline.py (the
kernels) and tests/test_chunk_pipeline_host.py (the same text built for the host, tests/host_sim/lane_sim.cpp).

Every generator returns a list of packets (bytes) of one configuration; what they should decode to comes from the oracle."""
import numpy as np

# frames per packet: every residue of the step count modulo the writer's chunk (8 steps) on both sides of one, two, three
# and four chunks; a slot whose longest packet has 1..7 frames holds no whole chunk at all
COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33)
ORDERS = (0, 4, 5, 6, 8, 12, 16, 31)
WRAP_STARTS = (1, 7, 8, 9, 16, 40)  # steps a coefficient starts away from the int16 limit it is driven to


def _bs(depth):
    return {16: 0, 20: 0, 24: 1, 32: 2}[depth]


def quiet_pcm(cfg, rng, frames):
    """A slow sine plus noise in every channel, with the low (shifted) bytes of the 24- and 32-bit depths random."""
    depth, ch = cfg.bit_depth, cfg.num_channels
    bs = _bs(depth)
    top = 1 << (depth - 8 * bs - 1)
    t = np.arange(frames)[:, None]
    hi = (top // 3 * np.sin(t / 7.0 + rng.uniform(0, 6.28, size=(1, ch)))).astype(np.int64) + rng.integers(-40, 41, size=(frames, ch))
    hi = np.clip(hi, -top, top - 1)
    pcm = ((hi << (8 * bs)) | rng.integers(0, 1 << (8 * bs), size=(frames, ch))) if bs else hi
    return np.ascontiguousarray(pcm, dtype=np.int32)


def _elem(synth, cfg, order_u, order_v=None, **kw):
    e = synth.default_elem(order=order_u, mix_res=kw.pop("mix_res", 1), mix_bits=kw.pop("mix_bits", 2),
                           bytes_shifted=_bs(cfg.bit_depth), never_escape=1, **kw)
    if order_v is not None:
        e.order_v = order_v
    return e


def count_set(synth, cfg, counts, order_u, order_v=None, seed=3):
    """One packet per entry of `counts` (frames), all of one key: the lanes of one wave slot, in this order."""
    rng = np.random.default_rng(seed + 131 * order_u + len(counts))
    return [synth.encode_packet(cfg, [_elem(synth, cfg, order_u, order_v, mix_res=i % 3)], quiet_pcm(cfg, rng, k))
            for i, k in enumerate(counts)]


def slot_sets(n=64):
    """Frame counts of a wave slot of n packets: each count of COUNTS alone (every lane ends in the same chunk; for counts
    below 8, 16, 24 the slot holds 0, 1, 2 whole chunks: consumer and writer lag are longer than the stream), all of them
    mixed (lanes that end in different chunks), and one lane with a single frame beside lanes with 33."""
    sets = [("all %d" % k, [k] * n) for k in COUNTS]
    sets.append(("mixed", [COUNTS[i % len(COUNTS)] for i in range(n)]))
    sets.append(("one short lane", [33] * (n // 2) + [1] + [33] * (n - n // 2 - 1)))
    return sets


# ---- coefficients at the int16 limits ---------------------------------------------------------------------------------

def _sign(x):
    return (x > 0) - (x < 0)


def _i16(x):
    return ((x + 32768) & 0xffff) - 32768


def wrap_channel(order, start, upper, frames, tap=None, den_shift=15, step=3):
    """Samples of one channel, built step by step against the reference's predictor (predictor.go:623-684), whose
    coefficient `tap` starts `start` steps away from +32767 (upper) or -32768 and moves one step towards it with every
    sample after the warm-up: the sample is put `step` above or below the prediction, on the side whose residual sign moves
    the coefficient the wanted way (:664, :675). The adaptation loop runs from the last tap down and ends when the residual
    is used up (:666, :677), so the driven tap is the last one unless the caller names another. Orders 4, 5, 6 and 8 keep
    their coefficients in int32 (:99-618) and walk on through the limit; every other order wraps. -> (samples, coefficients,
    indices of the samples whose step wraps a coefficient)."""
    tap = order - 1 if tap is None else tap
    wrapping = order not in (4, 5, 6, 8)
    coefs = [0] * order
    coefs[tap] = 32767 - start if upper else -32768 + start
    half = 1 << (den_shift - 1)
    out = list(range(order + 1))  # out[0] and the warm-up: a small ramp (what the lower limit's streams do to it grows)
    start_coefs = list(coefs)
    wraps = []
    for i in range(order + 1, frames):
        hist = out[i - order - 1:i]
        top = hist[0]
        sum1 = sum(coefs[k] * (hist[order - k] - top) for k in range(order))
        pred = top + ((sum1 + half) >> den_shift)
        a = hist[order - tap] - top
        s = (_sign(a) if upper else -_sign(a)) or 1
        x = pred + s * step
        assert -30000 < x < 30000, "the driven channel left the 16-bit range at sample %d" % i
        out.append(x)
        rest, wrapped = s * step, False
        for k in range(order - 1, -1, -1):
            dd = top - hist[order - k]
            sgn = _sign(dd)
            c = coefs[k] - sgn if s > 0 else coefs[k] + sgn
            if wrapping:
                wrapped |= _i16(c) != c
                c = _i16(c)
            coefs[k] = c
            rest -= (order - k) * ((s * sgn * dd) >> den_shift)
            if (s > 0 and rest <= 0) or (s < 0 and rest >= 0):
                break
        if wrapped:
            wraps.append(i)
    return out[:frames], start_coefs, wraps


def wrap_packet(synth, cfg, order, start, upper, frames, tap=None):
    """A packet (mono or an unmatrixed pair with the same samples and coefficients in both channels) whose coefficient
    `tap` crosses the int16 limit `start` steps behind the warm-up. 24- and 32-bit streams carry the driven 16-bit channel
    in their high bytes, over one or two shift bytes per sample (so the keys stay narrow: alac_decode_24q / _32q).
    -> (packet, indices of the wrapping steps)."""
    x, coefs, wraps = wrap_channel(order, start, upper, frames, tap)
    bs = _bs(cfg.bit_depth)
    assert cfg.bit_depth != 20, "a 20-bit channel is not 16 bits wide"
    hi = np.stack([x] * cfg.num_channels, axis=1).astype(np.int64)
    low = np.random.default_rng(order * 100 + start).integers(0, 1 << (8 * bs), size=hi.shape) if bs else 0
    pcm = np.ascontiguousarray((hi << (8 * bs)) | low, dtype=np.int32)
    e = synth.default_elem(order=order, den_shift=15, mix_res=0, mix_bits=0, bytes_shifted=bs, never_escape=1,
                           coef_mode=synth.COEF_GIVEN, coefs_u=coefs, coefs_v=coefs)
    return synth.encode_packet(cfg, [e], pcm), wraps


def far_packets(synth, cfg, order, n, frames, seed=5):
    """Packets of the same key whose coefficients stay far from the limits (the encoder's own)."""
    rng = np.random.default_rng(seed + order)
    return [synth.encode_packet(cfg, [synth.default_elem(order=order, mix_res=0, mix_bits=0, bytes_shifted=_bs(cfg.bit_depth), never_escape=1)],
                                quiet_pcm(cfg, rng, frames))
            for _ in range(n)]


def goref_wraps(packet, cfg):
    """The steps at which the reference's general predictor wraps a coefficient while it decodes `packet` (oracle/goref.py's
    trace), per channel: [(sample index, ...), ...]. A wrap shows as a coefficient that moves by more than one."""
    from oracle import goref
    trace = []
    gc = goref.PacketConfig(cfg.frame_length, cfg.bit_depth, cfg.num_channels, PB=cfg.pb, MB=cfg.mb, KB=cfg.kb, MaxRun=cfg.max_run)
    goref.decode_packet(gc, packet, trace=trace)
    chans, prev, last_idx = [], None, None
    for rec in trace:
        if not isinstance(rec, tuple) or rec[0] != "gen":
            continue
        idx, coefs = rec[1], rec[6]
        if last_idx is None or idx < last_idx:
            chans.append([])
            prev = None
        if prev is not None and any(abs(a - b) > 1 for a, b in zip(prev, coefs)):
            chans[-1].append(idx)
        prev, last_idx = coefs, idx
    return chans


WRAP_FRAMES = 56  # the longest stream the lower limit's order-5 channel keeps inside 16 bits


def wrap_starts(order):
    """WRAP_STARTS and the distances that put the wrapping step first and last in a chunk of 8 and of 16 steps."""
    extra = [s for s in range(2, 40) if (order + 1 + s) % 16 in (0, 7, 8, 15)]
    return sorted(set(WRAP_STARTS) | set(extra[:6]))


def wrap_set(synth, cfg, order, check_trace=False):
    """wrap_packet for both limits and every distance of wrap_starts(order). -> (packets, the wrapping steps modulo 16).
    check_trace: the model's wrapping steps are compared with the reference's trace (slow: pure Python)."""
    packets, where = [], set()
    for upper in (True, False):
        for start in wrap_starts(order):
            pkt, wraps = wrap_packet(synth, cfg, order, start, upper, WRAP_FRAMES)
            if order in (4, 5, 6, 8):
                assert wraps == []
            else:
                assert wraps and wraps[0] == order + 1 + start, (order, start, upper, wraps)
            if check_trace:  # (the int32 orders leave no records of the general predictor)
                assert goref_wraps(pkt, cfg) == ([wraps] * cfg.num_channels if wraps else []), (order, start, upper, wraps)
            where |= {w % 16 for w in wraps}
            packets.append(pkt)
    return packets, where
