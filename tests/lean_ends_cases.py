"""Packet sets for the entropy role at a packet's ends (alac_regular.h: ALAC_LEAN_ENDS, on in k_dec16l.hip), 16-bit streams:
shared by tests/test_lean_ends_host.py (tests/host_sim/lean_ends_sim.cpp) and tests/test_gpu_lean_ends.py (the kernel).

What the switch changes is decided by three distances: bits from a step's position to the packet's last bit (the END form of
the step from the chunk on in which a lane could reach it, the exact overrun test inside it), steps from a group to the lane's
last sample (the exact sample-end term: a group that the last sample closes runs plain), and dwords from a ring block to the
packet's last byte (tail blocks fetched whole, then masked). The sets below put codes of every kind at those distances.

Every generator returns a list of packets (bytes) of one configuration; what they should decode to comes from the oracle."""
import numpy as np

from tests import chunk_pipeline_cases as base

ORDERS = (4, 0, 12)


def _enc(synth, cfg, pcm, order=4, mix_res=1):
    e = synth.default_elem(order=order, mix_res=mix_res, mix_bits=2, bytes_shifted=0, never_escape=1)
    return synth.encode_packet(cfg, [e], np.ascontiguousarray(pcm, dtype=np.int32))


def _sparse(rng, frames, ch, one_in=64):
    """Mostly zeros with isolated +-1: the Golomb mean falls below 128 after a few samples and zero runs start everywhere."""
    return rng.choice([0] * (one_in - 2) + [1, -1], size=(frames, ch)).astype(np.int64)


def zero_run_endings(synth, cfg, counts, seed=11):
    """Quiet packets whose last samples are: a nonzero value followed by 0 .. 9 zeros (a zero run that starts at the last,
    the next-to-last, ... sample, or the packet ends inside one), and a lone nonzero value as the very last sample behind a
    run. One packet per (frame count, tail); orders rotate."""
    rng = np.random.default_rng(seed)
    out = []
    for n in counts:
        for tail in range(0, 10):
            x = _sparse(rng, n, cfg.num_channels)
            if tail < n:
                x[n - 1 - tail] = rng.choice([1, -1, 2, -3], size=cfg.num_channels)
                x[n - tail:] = 0
            out.append(_enc(synth, cfg, x, order=ORDERS[(n + tail) % 3] if n > 12 else 0, mix_res=tail % 2))
    return out


def escape_endings(synth, cfg, counts, seed=12):
    """A quiet signal whose last 1 .. 4 samples (and one in the middle) are full-scale: with the mean small their codes are
    escape codes (nine ones and chanBits literal bits, golomb.go:184-186), so the packet's last codes are escape codes; with
    the element kept compressed (never_escape). Order 0: the samples are the residuals."""
    rng = np.random.default_rng(seed)
    out = []
    for n in counts:
        for last in (1, 2, 3, 4):
            x = rng.integers(-6, 7, size=(n, cfg.num_channels)).astype(np.int64)
            spikes = rng.choice([-32768, 32767, -30000, 29999], size=(min(last, n), cfg.num_channels))
            x[n - min(last, n):] = spikes
            if n > 20:
                x[n // 2] = 32767
            out.append(_enc(synth, cfg, x, order=0, mix_res=0))
    return out


def loud_and_quiet(synth, cfg, counts, seed=13):
    """Music-like and near-silent packets of the given frame counts, orders rotating: streams of 2 .. 12 bits per sample, so
    that lanes of one wave come within reach of their packet's end at different top-ups."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(counts):
        for amp in (3, 40, 3000):
            t = np.arange(n)[:, None]
            x = (amp * 4 * np.sin(t / 7.0 + rng.uniform(0, 6.28, size=(1, cfg.num_channels)))).astype(np.int64)
            x += rng.integers(-amp, amp + 1, size=x.shape)
            out.append(_enc(synth, cfg, x, order=ORDERS[i % 3] if n > 12 else 0, mix_res=i % 3))
    return out


def short_v(synth, cfg, seed=14):
    """2 .. 40 frames of a near-silent signal: the V channel is shorter than 329 bits, so the U channel, too, ends within reach
    of the packet's end."""
    rng = np.random.default_rng(seed)
    return [_enc(synth, cfg, _sparse(rng, n, cfg.num_channels, one_in=16), order=0 if n <= 12 else 4) for n in range(2, 41)]


def appended(packets, seed=15):
    """Valid packets with 1 .. 48 bytes behind the END tag's byte: random ones, all ones and zeros in turn."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(1, 49):
        p = packets[k % len(packets)]
        extra = [rng.integers(0, 256, k, dtype=np.uint8).tobytes(), b"\xff" * k, b"\0" * k][k % 3]
        out.append(p + extra)
    return out


def crafted(synth, cfg, counts):
    """All of the above for one configuration -> list of packets, every one valid (the oracle decodes it without error)."""
    zr = zero_run_endings(synth, cfg, counts)
    esc = escape_endings(synth, cfg, counts)
    lq = loud_and_quiet(synth, cfg, counts)
    return zr + esc + lq + short_v(synth, cfg) + appended(zr[::7] + esc[::3] + lq[::2])


def end_faults(packets, last_bytes=64, flip_bytes=8):
    """The prefixes that cut the last `last_bytes` bytes of each packet, and the one-bit faults of its last `flip_bytes`."""
    out = []
    for p in packets:
        out += [p[:k] for k in range(max(len(p) - last_bytes, 0), len(p))]
        a = np.frombuffer(p, np.uint8)
        for bit in range(8 * max(len(p) - flip_bytes, 0), 8 * len(p)):
            b = a.copy()
            b[bit >> 3] ^= 0x80 >> (bit & 7)
            out.append(b.tobytes())
    return out


def tile(pool, n, stride):
    """n packets out of the pool, walked with a stride coprime to its length: every run of 64 holds a mixture."""
    assert np.gcd(stride, len(pool)) == 1, (stride, len(pool))
    return [pool[(i * stride) % len(pool)] for i in range(n)]
