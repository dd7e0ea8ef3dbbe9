"""Every one-bit fault and every truncation of small packets: the corpus of tests/test_single_fault.py (CPU) and
tests/test_gpu_single_fault.py (GPU).

A packet's result is decided twice: by classify_regular (alac_regular.h), which reads the element header and picks a
route, and by the route, which relies on what the classifier promised. Each promise is an edge in packet space that one
header bit or one byte of length crosses. The packets here are small (24-80 frames, 40-700 bytes), so ALL their one-bit
faults and ALL their prefixes are a few thousand packets per seed.

  seeds()        one valid packet per row of ROWS, signal and frame count
  prefixes()     p[:k] for k = 0..len(p)
  flips()        p with bit k inverted, for every bit k
  counts()       the o4 seed at every frame count 1..FrameLength
  loud_counts()  1..12 frames of full-scale noise: entropy streams of 8-12 bytes, both sides of the ten-byte rule of
                 classify_regular
  field_of()     the name of the header field a bit lies in (failure messages and reach assertions only)
  corpus()       all of the above for one stream configuration, cached, with the oracle's answer for every packet

The expected result of a packet is the oracle's (PCM of the frames, frame count, status word) on the padded layout
(conftest.pack_packets). Nothing here filters, skips or samples packets.
"""
import numpy as np

SHIFT = {16: 0, 20: 0, 24: 1, 32: 2}  # the shift bytes real encoders use
COOKIES = {"std": dict(pb=40, mb=10, kb=14), "pb100": dict(pb=100, mb=10, kb=14), "kb0": dict(pb=40, mb=10, kb=0)}

# (depth, channels, frame length, cookie): every route is the only or the main one somewhere
LEAN = [(16, 2, 48, "std"), (24, 2, 48, "std"), (32, 2, 40, "std"), (16, 1, 64, "std"), (24, 1, 50, "std"), (32, 1, 40, "std"),
        (20, 2, 33, "std")]                                   # lean pairs and wide pairs
SHORT = [(16, 2, 24, "std")]                                  # frame length <= 32: nothing is regular
WHOLE = [(16, 2, 48, "pb100"), (16, 2, 48, "kb0")]            # not a lean config: the whole-packet decoder
MULTI = [(24, 3, 36, "std"), (16, 8, 34, "std")]              # scan, predictor pass, interleave
CONFIGS = LEAN + SHORT + WHOLE + MULTI
COUNT_CONFIGS = [(24, 2, 80), (32, 2, 80), (24, 1, 80), (32, 1, 80), (16, 2, 80)]
LOUD_FL = 80
LOUD_SETS = [(24, 2, 1), (24, 2, 2), (32, 2, 2), (32, 2, 1), (24, 1, 1), (32, 1, 2), (32, 1, 1)]  # depth, channels, bytes_shifted
GOREF_CONFIGS = [(16, 2, 48, "std"), (24, 2, 48, "std"), (32, 1, 40, "std"), (24, 3, 36, "std"), (20, 2, 33, "std")]
GOREF_SEEDS = ("o4/music", "o17/music", "noshift/music", "esc/music", "uv/quiet", "mode/quiet")
VARIANT_ROWS = ("o4", "uv", "esc", "noshift")  # lane_sim variants -2 and 3 run on the faults of these

KEY_WIDE, KEY_IRREGULAR = 1024, 2048  # alac_regular.h


def ROWS(synth, depth, channels):
    """name -> Elem settings (never_escape and the width's shift bytes are added by seeds())."""
    # chanBits 33 (a 32-bit pair without shift bytes) decodes to zeros (predictor.go:46): one shift byte there
    rows = {"o%d" % k: dict(order=k) for k in (0, 1, 4, 8, 9, 16, 31)}
    rows["o17"] = dict(order=17)                       # no lean instantiation: irregular from the start
    rows["uv"] = dict(order_u=5, order_v=12)           # different keys per channel
    rows["mode"] = dict(order=6, mode_u=1, mode_v=2)   # the delta pass in front: irregular
    rows["esc"] = dict(force_escape=1, never_escape=0)
    rows["noshift"] = dict(order=4, bytes_shifted=1 if (depth == 32 and channels >= 2) else 0)  # the wide keys at 24 / 32 bits
    rows["den0"] = dict(order=4, den_shift=0)
    rows["pbf0"] = dict(order=4, pb_factor=0)
    rows["fil"] = dict(order=4, flags=synth.FLAG_LEADING_FIL)  # the first tag is not the audio element
    return rows


def make_cfg(oracle, depth, channels, fl, cookie="std"):
    return oracle.make_config(fl, depth, channels, **COOKIES[cookie])


def cfg_name(cfg):
    extra = "" if (cfg.pb, cfg.kb) == (40, 14) else " PB %d KB %d" % (cfg.pb, cfg.kb)
    return "%d-bit %dch %d%s" % (cfg.bit_depth, cfg.num_channels, cfg.frame_length, extra)


# ---- signals --------------------------------------------------------------------------------------------------------
def music(cfg, frames, rng):
    """A sine of a sixth of full scale plus small noise."""
    top = 1 << (cfg.bit_depth - 1)
    t = np.arange(frames)[:, None]
    ph = rng.uniform(0, 6.28, size=(1, cfg.num_channels))
    x = (top // 6 * np.sin(t / 7.0 + ph)).astype(np.int64) + rng.integers(-(top >> 11) - 2, (top >> 11) + 3, size=(frames, cfg.num_channels))
    return np.ascontiguousarray(np.clip(x, -top, top - 1), dtype=np.int32)


def quiet(cfg, frames, rng, bytes_shifted):
    """Mostly zeros with isolated +-1, shifted up by the shift bytes."""
    x = rng.choice([0] * 62 + [1, -1], size=(frames, cfg.num_channels)).astype(np.int64)
    return np.ascontiguousarray(x << (8 * bytes_shifted), dtype=np.int32)


def _encode(synth, cfg, settings, pcm):
    kw = dict(never_escape=1, bytes_shifted=SHIFT[cfg.bit_depth])
    kw.update(settings)
    flags = kw.pop("flags", 0)
    elems = [synth.default_elem(**kw) for _ in range(synth.num_elements(cfg.num_channels))]
    return synth.encode_packet(cfg, elems, pcm, flags=flags)


# ---- the corpus -----------------------------------------------------------------------------------------------------
def seeds(synth, cfg, frames, rng):
    """-> list of (name, packet, source PCM bytes): one packet per row of ROWS and per signal, `frames` frames long."""
    out = []
    for row, settings in ROWS(synth, cfg.bit_depth, cfg.num_channels).items():
        bs = settings.get("bytes_shifted", SHIFT[cfg.bit_depth])
        for sig in ("music", "quiet"):
            pcm = music(cfg, frames, rng) if sig == "music" else quiet(cfg, frames, rng, bs)
            out.append(("%s/%s" % (row, sig), _encode(synth, cfg, settings, pcm), synth.pack_pcm(cfg, pcm)))
    return out


def prefixes(p):
    return [p[:k] for k in range(len(p) + 1)]


def flips(p):
    """p with bit k inverted (bit 0 is the top bit of byte 0, the order the decoder reads them in), for every k."""
    a = np.frombuffer(p, np.uint8)
    n = len(a)
    m = np.tile(a, (8 * n, 1))
    k = np.arange(8 * n)
    m[k, k >> 3] ^= (0x80 >> (k & 7)).astype(np.uint8)
    return [r.tobytes() for r in m]


def counts(synth, cfg, rng):
    """The o4 seed, music and quiet, at every frame count 1..FrameLength (valid packets only; a count that does not exceed
    the order takes order 0: UnpcBlock's warm-up needs order < frames, predictor.go:76-79)
    -> list of (name, packet, source PCM bytes)."""
    out = []
    bs = SHIFT[cfg.bit_depth]
    for n in range(1, cfg.frame_length + 1):
        for sig in ("music", "quiet"):
            pcm = music(cfg, n, rng) if sig == "music" else quiet(cfg, n, rng, bs)
            out.append(("count %d/%s" % (n, sig), _encode(synth, cfg, dict(order=4 if n > 4 else 0), pcm), synth.pack_pcm(cfg, pcm)))
    return out


def entropy_bytes(cfg, packet):
    """Packet size minus the byte in which the entropy stream starts (what classify_regular's ten-byte rule counts)."""
    for a, b, name in fields(cfg, packet):
        if name == "entropy":
            return len(packet) - (a >> 3)
    raise AssertionError("no entropy stream")


def loud_counts(synth, cfg, bytes_shifted, rng):
    """Valid packets of 1..12 frames of full-scale noise that stay compressed: every sample is an escape code, a few frames
    make an entropy stream of 8-12 bytes. Orders 0 and 4 (0 where the count does not exceed the order), mix_res 0 and 1,
    six packets of each. The set must hold a packet whose entropy stream is 8 or 9 bytes and one where it is 10 or 11 (the
    two sides of classify_regular's ten-byte rule): where full scale alone does not give both, the same sweep is added at
    half the amplitude, and again, until it does. -> list of (name, packet, source PCM bytes)."""
    depth, ch = cfg.bit_depth, cfg.num_channels
    hi_bits = depth - 8 * bytes_shifted
    out, sizes = [], set()
    for drop in range(hi_bits - 1):
        top = 1 << (hi_bits - 1 - drop)
        for n in range(1, 13):
            for mix_res in (0, 1):
                for j in range(6):
                    hi = rng.integers(-top, top, size=(n, ch)).astype(np.int64)
                    pcm = (hi << (8 * bytes_shifted)) | rng.integers(0, 1 << (8 * bytes_shifted), size=(n, ch))
                    pcm = np.ascontiguousarray(pcm, dtype=np.int32)
                    order = 4 if (j % 2 and n > 4) else 0
                    p = _encode(synth, cfg, dict(order=order, mix_res=mix_res, bytes_shifted=bytes_shifted), pcm)
                    out.append(("loud %d frames o%d mixRes %d amplitude 2^%d #%d" % (n, order, mix_res, hi_bits - 1 - drop, j), p,
                                synth.pack_pcm(cfg, pcm)))
                    sizes.add(entropy_bytes(cfg, p))
        if sizes & {8, 9} and sizes & {10, 11}:
            return out
    raise AssertionError("%s shift %d: entropy streams of %s bytes only" % (cfg_name(cfg), bytes_shifted, sorted(sizes)))


# ---- header fields --------------------------------------------------------------------------------------------------
def fields(cfg, packet):
    """[(first bit, end bit, name)] of the packet's first element, in the order the reference reads them
    (decoder.go:213-235 the element header of an SCE / LFE, :354-376 of a CPE; :272-285 and :421-450 the compressed
    element's mix and predictor fields; :289-293 and :453-457 the shift bytes). Empty for streams of more than two
    channels and for packets whose first tag is not the stream's audio element."""
    nbits = 8 * len(packet)
    bits = np.unpackbits(np.frombuffer(packet, np.uint8))

    def get(pos, n):
        return int("".join(map(str, bits[pos:pos + n])), 2) if pos + n <= nbits else None

    ch = cfg.num_channels
    if ch > 2 or nbits < 23 or get(0, 3) != (1 if ch == 2 else 0):
        return []
    out = [(0, 3, "tag"), (3, 7, "instance"), (7, 19, "unused"), (19, 20, "partial"), (20, 22, "shift"), (22, 23, "escape")]
    pos, ns = 23, cfg.frame_length
    if bits[19]:
        ns = get(pos, 32)
        out.append((pos, pos + 32, "count"))
        pos += 32
    nz = np.nonzero(bits)[0]
    end = int(nz[-1]) - 2  # `element END pad`: END is 111 and the pad is zero
    if bits[22]:
        out.append((pos, end, "samples"))
    else:
        out += [(pos, pos + 8, "mixBits"), (pos + 8, pos + 16, "mixRes")]
        pos += 16
        for c in "UV"[:ch]:
            order = get(pos + 11, 5)
            out += [(pos, pos + 4, c + ".mode"), (pos + 4, pos + 8, c + ".denShift"), (pos + 8, pos + 11, c + ".pbFactor"),
                    (pos + 11, pos + 16, c + ".order")]
            pos += 16
            for j in range(order or 0):
                out.append((pos, pos + 16, "%s.coef[%d]" % (c, j)))
                pos += 16
        bs = get(20, 2)
        if bs:
            out.append((pos, pos + 8 * bs * ch * ns, "shift bytes"))
            pos += 8 * bs * ch * ns
        out.append((pos, end, "entropy"))
    out.append((end, nbits, "behind the first element"))
    return out


def field_of(cfg, packet, bit):
    """The field of `packet` (an intact one) that bit `bit` lies in; "bit k" where fields() does not say."""
    for a, b, name in fields(cfg, packet):
        if a <= bit < b:
            return name
    return "bit %d" % bit


# ---- a configuration's whole corpus ---------------------------------------------------------------------------------
class Seed:
    """One seed packet and where its faults lie in the configuration's packet list: [first, first + npre) its prefixes
    (prefix k at first + k), [first + npre, end) its flips (bit k at first + npre + k)."""

    def __init__(self, name, row, sig, frames, packet, pcm, first):
        self.name, self.row, self.sig, self.frames, self.packet, self.pcm, self.first = name, row, sig, frames, packet, pcm, first
        self.npre = len(packet) + 1
        self.end = first + self.npre + 8 * len(packet)

    def what(self, cfg, i):
        """Packet i of the list (first <= i < end) in words."""
        k = i - self.first
        if k < self.npre:
            return "%s %s: prefix %d of %d" % (cfg_name(cfg), self.name, k, len(self.packet))
        k -= self.npre
        return "%s %s: bit %d (%s)" % (cfg_name(cfg), self.name, k, field_of(cfg, self.packet, k))

    def flip_index(self, cfg, field):
        """Indices (into the configuration's list) of the flips inside `field`."""
        return [self.first + self.npre + k for a, b, name in fields(cfg, self.packet) if name == field for k in range(a, b)]


class Corpus:
    """cfg, seeds (list of Seed), packets (every seed's prefixes, then its flips, seed after seed), ref (the oracle's out,
    frames, status for `packets`), seed_ref (the same for the intact seed packets)."""


_cache = {}


def oracle_ref(oracle, cfg, packets):
    from tests.conftest import pack_packets
    blob, offs, sizes = pack_packets(packets)
    return oracle.decode_batch(cfg, blob, offs, sizes, threads=8)


def corpus(synth, oracle, depth, channels, fl, cookie="std"):
    key = ("faults", depth, channels, fl, cookie)
    if key not in _cache:
        c = Corpus()
        c.cfg = make_cfg(oracle, depth, channels, fl, cookie)
        rng = np.random.default_rng([depth, channels, fl, sorted(COOKIES).index(cookie)])
        c.seeds, c.packets = [], []
        for frames in (fl, fl - 11):  # no count in the header; partial flag and a 32-bit count
            for name, p, pcm in seeds(synth, c.cfg, frames, rng):
                row, sig = name.split("/")
                s = Seed("%s %s" % (name, "fl" if frames == fl else "fl-11"), row, sig, frames, p, pcm, len(c.packets))
                c.seeds.append(s)
                c.packets += prefixes(p)
                c.packets += flips(p)
                assert len(c.packets) == s.end
        c.ref = oracle_ref(oracle, c.cfg, c.packets)
        c.seed_ref = oracle_ref(oracle, c.cfg, [s.packet for s in c.seeds])
        _cache[key] = c
    return _cache[key]


def what(c, i):
    for s in c.seeds:
        if s.first <= i < s.end:
            return s.what(c.cfg, i)
    raise IndexError(i)


def sweeps(synth, oracle, depth, channels):
    """The counts sweep and the loud-counts sets of one (depth, channels) -> list of (set name, cfg, [(name, packet, pcm)],
    the oracle's (out, frames, status)), cached."""
    key = ("sweeps", depth, channels)
    if key not in _cache:
        out = []
        cfg = make_cfg(oracle, depth, channels, 80)
        rng = np.random.default_rng([depth, channels, 80])
        items = counts(synth, cfg, rng)
        out.append(("counts", cfg, items, oracle_ref(oracle, cfg, [p for _, p, _ in items])))
        for d, ch, bs in LOUD_SETS:
            if (d, ch) == (depth, channels):
                cfg = make_cfg(oracle, d, ch, LOUD_FL)
                items = loud_counts(synth, cfg, bs, rng)
                out.append(("loud counts, %d shift bytes" % bs, cfg, items, oracle_ref(oracle, cfg, [p for _, p, _ in items])))
        _cache[key] = out
    return _cache[key]


def first_difference(ref, got, bpf, names):
    """None, or a sentence about the first packet whose (status, frame count, PCM of the frames) differ. names: i -> str."""
    (o1, f1, s1), (o2, f2, s2) = ref, got
    f1, f2 = np.asarray(f1).astype(np.int64), np.asarray(f2).astype(np.int64)
    nb = f1 * bpf
    w = o1.shape[1]
    have = np.arange(w)[None, :] < nb[:, None]
    bad = (np.asarray(s1) != np.asarray(s2)) | (f1 != f2) | ((o1 != o2[:, :w]) & have).any(axis=1)
    if not bad.any():
        return None
    i = int(np.nonzero(bad)[0][0])
    d = np.nonzero((o1[i] != o2[i, :w]) & have[i])[0]
    return "%s: oracle status %#x, %d frames; got status %#x, %d frames; first differing PCM byte %s; %d packets differ" % (
        names(i), s1[i], f1[i], s2[i], f2[i], d[0] if len(d) else "none", int(bad.sum()))
