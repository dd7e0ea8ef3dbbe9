"""Packets whose element order is not the channel layout's own: a composer that splices synth-made elements into any
sequence, and a model of what the reference makes of such a sequence.

The reference reads a packet as a run of tagged elements (decoder.go:142-203) and never checks that run against
NumChannels: element k writes at channelLayoutOffsets[numChan-1][chanIdx] (decoder.go:55-64), a later element overwrites
an earlier one where they meet, a channel nobody wrote stays zero (decoder.go:120,127), an element without the partial
flag takes the count of the element before it and the packet's frame count is the last element's.

  element()   one SCE / LFE / CPE, cut at bit level out of a one-element packet of the synth (an element's bits do not
              depend on the stream's channel count)
  fil(), dse()  filler elements in both count forms (decoder.go:538-574)
  compose()   parts -> packet bytes
  expected()  THE MODEL: walks a sequence with chanIdx, numSamples and the layout table and copies each element's SOURCE
              PCM into a zeroed frame buffer. It never calls a decoder.
  CORPUS()    a seeded generator of (name, packet, seq); the name starts with the number of the list in its docstring.

A sequence (`seq`) is a list of items: (kind, count, pcm, bits) for an audio element — kind "SCE" / "LFE" / "CPE", count
the explicit frame count or None for the carried one, pcm int32 [frames][1 or 2] —, ("FIL", nbytes, ext), ("DSE", nbytes,
align) and ("END",).
"""
import numpy as np

LAYOUT = [  # channelLayoutOffsets, decoder.go:55-64
    [0], [0, 1], [2, 0, 1], [2, 0, 1, 3], [2, 0, 1, 3, 4], [2, 0, 1, 4, 5, 3], [2, 0, 1, 4, 5, 6, 3],
    [2, 6, 7, 0, 1, 4, 5, 3],
]
SHIFT = {16: 0, 20: 0, 24: 1, 32: 2}  # the shift bytes real encoders use
TAG = {"SCE": 0, "CPE": 1, "LFE": 3}
COOKIES = {"std": dict(pb=40, mb=10, kb=14), "pb255": dict(pb=255, mb=10, kb=14), "kb0": dict(pb=40, mb=10, kb=0)}
ORDERS = (0, 1, 4, 5, 6, 8, 9, 16, 17, 30, 31)
AUDIO = ("SCE", "LFE", "CPE")


def to_bits(value, nbits):
    return np.array([(value >> (nbits - 1 - k)) & 1 for k in range(nbits)], np.uint8)


END_BITS = to_bits(7, 3)


# ---- elements -------------------------------------------------------------------------------------------------------
def element(synth, oracle, kind, depth, frames, partial, cookie, pcm=None, instance=None, **elem_settings):
    """One SCE / LFE / CPE of `frames` frames -> (bits, pcm). partial: the element carries its count (the flag is set,
    whatever the stream's FrameLength); otherwise it takes the count carried from the element before it. cookie: pb / mb / kb
    of the stream. instance: the 4-bit instance tag (the synth writes 0). elem_settings: fields of synth.Elem."""
    nch = 2 if kind == "CPE" else 1
    pcm = np.ascontiguousarray(pcm, dtype=np.int32)
    assert pcm.shape == (frames, nch) and frames >= 1
    # the synth sets the partial flag iff frames != frame_length (alac_synth.c: encode_element)
    cfg = oracle.make_config(frames + 1 if partial else frames, depth, nch, **cookie)
    pkt = synth.encode_packet(cfg, [synth.default_elem(**elem_settings)], pcm)
    bits = np.unpackbits(np.frombuffer(pkt, np.uint8))
    # `X END pad`: END is 111 and the pad is zero, so the element ends two bits before the packet's last set bit
    last = int(np.nonzero(bits)[0][-1])
    assert last >= len(bits) - 8 and last >= 22 and bits[last - 2:last + 1].all(), "no END behind the element"
    bits = bits[:last - 2].copy()
    assert int(bits[:3] @ (4, 2, 1)) == TAG["CPE" if nch == 2 else "SCE"] and bits[19] == (1 if partial else 0)
    if partial:
        assert int("".join(map(str, bits[23:55])), 2) == frames
    if kind == "LFE":
        bits[:3] = to_bits(TAG["LFE"], 3)
    if instance is not None:
        bits[3:7] = to_bits(instance, 4)
    return bits, pcm


def _payload(nbytes, salt):
    return np.unpackbits(((np.arange(nbytes) * 37 + salt) % 255 + 1).astype(np.uint8))


def fil(nbytes, ext=None):
    """FIL (decoder.go:538-552): a 4-bit count, 15 means 15 + an 8-bit count - 1. ext: force the long form (14..269 bytes)."""
    ext = nbytes >= 15 if ext is None else ext
    if ext:
        assert 14 <= nbytes <= 269
        head = [to_bits(6, 3), to_bits(15, 4), to_bits(nbytes - 14, 8)]
    else:
        assert 0 <= nbytes <= 14
        head = [to_bits(6, 3), to_bits(nbytes, 4)]
    return np.concatenate(head + [_payload(nbytes, 0xAB)])


def dse(nbytes, align):
    """DSE (decoder.go:555-574): instance tag, align flag, an 8-bit count, 255 means 255 + another 8 bits. Where its data
    starts depends on where the element lands, so compose() builds it in place."""
    assert 0 <= nbytes <= 510
    return ("DSE", nbytes, 1 if align else 0)


def _dse_bits(pos, nbytes, align):
    head = [to_bits(4, 3), to_bits(9, 4), to_bits(align, 1)]
    head.append(to_bits(nbytes, 8) if nbytes < 255 else np.concatenate([to_bits(255, 8), to_bits(nbytes - 255, 8)]))
    n = pos + sum(len(h) for h in head)
    if align and n % 8:
        head.append(np.ones(8 - n % 8, np.uint8))  # ByteAlign skips them whatever they hold
    return np.concatenate(head + [_payload(nbytes, 0x5D)])


def compose(parts, end=True):
    """Bit strings (and dse() specs) -> packet bytes: the parts, END, zero bits up to a byte."""
    out, pos = [], 0
    for p in list(parts) + ([END_BITS] if end else []):
        if isinstance(p, tuple):
            p = _dse_bits(pos, p[1], p[2])
        out.append(p)
        pos += len(p)
    return np.packbits(np.concatenate(out) if out else np.zeros(0, np.uint8)).tobytes()


def parts_of(seq):
    out = []
    for it in seq:
        if it[0] in AUDIO:
            out.append(it[3])
        elif it[0] == "FIL":
            out.append(fil(it[1], it[2]))
        elif it[0] == "DSE":
            out.append(dse(it[1], it[2]))
        else:
            out.append(END_BITS)
    return out


def packet_of(seq, end=True):
    return compose(parts_of(seq), end=end)


# ---- the model ------------------------------------------------------------------------------------------------------
def expected(num_channels, frame_length, seq):
    """What DecodePacket makes of `seq` -> ("ok", frames, pcm[frames][num_channels]) or ("malformed",).

    decoder.go:133-207: numSamples starts as FrameLength and every audio element replaces it (by its own count with the
    partial flag, by itself otherwise); element k writes its channels at offsets[chanIdx] of a zeroed frame buffer, in
    sequence order, so later writes win; the walk stops at END, at chanIdx >= numChan (:200-202) and at a CPE with chanIdx +
    2 > numChan (:163-165). Two classes are malformed: a CPE whose offsets[chanIdx] + 2 > numChan (the reference writes
    outside the frame) and a count above FrameLength (mixBuffer[:numSamples] panics)."""
    offsets = LAYOUT[num_channels - 1]
    out = np.zeros((frame_length, num_channels), np.int32)
    chan_idx, ns = 0, frame_length
    for it in seq:
        kind = it[0]
        if kind == "END":
            break
        if kind in ("FIL", "DSE"):
            continue
        nch_e = 2 if kind == "CPE" else 1
        if nch_e == 2 and chan_idx + 2 > num_channels:
            break
        o = offsets[chan_idx]
        if o + nch_e > num_channels:
            return ("malformed",)
        count, pcm = it[1], it[2]
        n = ns if count is None else count
        if n > frame_length:
            return ("malformed",)
        assert len(pcm) == n, "a carried count must be the element's own length"
        out[:n, o:o + nch_e] = pcm
        ns = n
        chan_idx += nch_e
        if chan_idx >= num_channels:
            break
    return ("ok", ns, out[:ns].copy())


def walk(num_channels, seq):
    """Bookkeeping for the corpus and the reach assertions (no PCM): -> dict(slots: bitstream channels consumed, writes: [(first
    output channel, width)] per decoded element, overlap: two elements meet, pair_last: a pair in the last output slot,
    quiet: a CPE that did not fit ended the packet)."""
    offsets = LAYOUT[num_channels - 1]
    chan_idx, writes, seen, overlap, pair_last, quiet = 0, [], set(), False, False, False
    for it in seq:
        if it[0] == "END":
            break
        if it[0] not in AUDIO:
            continue
        w = 2 if it[0] == "CPE" else 1
        if w == 2 and chan_idx + 2 > num_channels:
            quiet = True
            break
        o = offsets[chan_idx]
        if o + w > num_channels:
            pair_last = True
            break
        cs = set(range(o, o + w))
        overlap = overlap or bool(cs & seen)
        seen |= cs
        writes.append((o, w))
        chan_idx += w
        if chan_idx >= num_channels:
            break
    return dict(slots=chan_idx, writes=writes, overlap=overlap, pair_last=pair_last, quiet=quiet)


# ---- the corpus -----------------------------------------------------------------------------------------------------
def compositions(num_channels):
    """Every sequence of 1- and 2-channel elements whose channel sum is at most num_channels, and those that overshoot by
    one with a last pair (which does not fit) -> list of tuples of 1 / 2, the empty one included."""
    out = []

    def rec(prefix, total):
        out.append(tuple(prefix))
        for w in (1, 2):
            if total + w <= num_channels:
                rec(prefix + [w], total + w)
            elif w == 2 and total + w == num_channels + 1:
                out.append(tuple(prefix + [2]))

    rec([], 0)
    return out


class _Maker:
    """Elements of one stream config with seeded signals: every element gets its own constant offset (so that swapped
    channels cannot cancel out) and the opposite sign of the element before it (so that OR and replace differ where two
    writers meet)."""

    def __init__(self, synth, oracle, depth, frame_length, cookie, rng, override=None):
        self.synth, self.oracle, self.depth, self.fl, self.cookie, self.rng = synth, oracle, depth, frame_length, cookie, rng
        self.override = dict(override or {})
        self.eid = 0

    def pcm(self, frames, nch, style):
        rng, top = self.rng, 1 << (self.depth - 1)
        eid = self.eid
        self.eid += 1
        sign = 1 if eid % 2 == 0 else -1
        t = np.arange(frames)[:, None]
        ph = rng.uniform(0, 6.28, size=(1, nch))
        if style == "antiphase":  # loud pairs, L = -R - 1 near full scale (conftest.antiphase_packets)
            amp = top - 40 - 16 * (eid % 8)
            x = (sign * amp * np.sin(t / 9.0 + ph[:, :1] + 1.0)).astype(np.int64) + rng.integers(-30, 31, size=(frames, 1))
            x = np.clip(x, -top, top - 1)
            x = np.concatenate([x, np.clip(-x - 1, -top, top - 1)], axis=1)[:, :nch]
            bs = SHIFT[self.depth]
            if bs:  # the synth splits the low bytes off: keep the high part's anti-phase and give the low bytes noise
                x = ((x >> (8 * bs)) << (8 * bs)) | rng.integers(0, 1 << (8 * bs), size=x.shape)
        else:
            dc = sign * (top // 4 + (eid % 8) * (top // 64)) + np.arange(nch)[None, :] * (top // 128)
            x = (top // 8 * np.sin(t / (5.0 + eid % 7) + ph)).astype(np.int64) + dc + rng.integers(-top // 512 - 2, top // 512 + 3, size=(frames, nch))
        return np.ascontiguousarray(np.clip(x, -top, top - 1), dtype=np.int32)

    def item(self, kind, frames, explicit, style="music", **kw):
        """A seq item; explicit: carries its count (else the count must be the one carried to it)."""
        nch = 2 if kind == "CPE" else 1
        kw.setdefault("bytes_shifted", SHIFT[self.depth])
        if style == "antiphase":
            kw.update(mix_res=1, mix_bits=2, never_escape=1)
        kw.update(self.override)
        kw.setdefault("order", 4)
        if kw["order"] >= frames:  # UnpcBlock's warm-up needs order < frames (predictor.go:76-79)
            kw["order"] = 0
        bits, pcm = element(self.synth, self.oracle, kind, self.depth, frames, explicit, self.cookie,
                            pcm=self.pcm(frames, nch, style), **kw)
        return (kind, frames if explicit else None, pcm, bits)


def _kinds(comp, lfe_at=()):
    return ["CPE" if w == 2 else ("LFE" if k in lfe_at else "SCE") for k, w in enumerate(comp)]


def _counts(pattern, n, fl, a=None):
    """Frame counts of n elements -> list of (frames, explicit)."""
    a = fl if a is None else a
    if pattern == "full":
        return [(fl, False)] * n
    if pattern == "flagged_full":  # a count equal to FrameLength with the flag set
        return [(fl, True)] + [(fl, k % 2 == 1) for k in range(1, n)]
    if pattern == "first":  # first explicit, then carried
        return [(a, True)] + [(a, False)] * (n - 1)
    if pattern == "one":
        return [(1, True)] + [(1, k % 2 == 0) for k in range(1, n)]
    if pattern == "last_one":
        return [(fl, False)] * (n - 1) + [(1, True)]
    if pattern in ("grow", "shrink"):
        lo = max(1, a // 3)
        c = [lo + (a - lo) * k // max(n - 1, 1) for k in range(n)] if n > 1 else [a]
        if pattern == "shrink":
            c = c[::-1]
        return [(x, True) for x in c]
    if pattern == "zigzag":  # a and a neighbour of it in turn, carried in between
        b = a - 1 if a > 1 else min(a + 1, fl)
        return [((a, b)[(k // 2) % 2], k % 2 == 0) for k in range(n)]  # the odd ones carry the count before them
    raise ValueError(pattern)


def edge_counts(fl):
    """Counts on both sides of 4, 64, 256 and 1024 — the interleave kernels' lane, slice and span sizes — that fit."""
    return sorted({c for m in (4, 64, 256, 1024) for c in (m - 1, m, m + 1) if 1 <= c <= fl})


FILLERS = [("FIL", 0, False), ("DSE", 0, 0), ("FIL", 3, False), ("DSE", 5, 1), ("FIL", 14, False), ("FIL", 14, True),
           ("DSE", 254, 0), ("FIL", 15, True), ("DSE", 255, 1), ("FIL", 40, True), ("DSE", 300, 0), ("DSE", 1, 1), ("FIL", 269, True)]


def CORPUS(synth, oracle, depth, num_channels, frame_length, rng, cookie=None, budget=None, override=None):
    """-> list of (name, packet bytes, seq) for one stream config; deterministic for a given rng state. The name begins with
    the number of the item below that the packet is there for.

      1  every composition of 1- and 2-channel elements up to the channel count, and one past it (a last pair that does not
         fit), with END and, where the sequence ends the walk by itself, without; the frame-count patterns of 3 in turn
      2  END after 0, 1, ... elements, the rest of the elements behind it
      3  frame counts: all full; first explicit then carried; growing; shrinking; 1; FrameLength with the flag; both sides of
         4, 64, 256 and 1024
      4  every composition in which two elements meet in an output channel (layout table), with equal counts and with the
         longer writer first and second
      5  element kinds mixed in one packet: escape and compressed, the orders of ORDERS, mode != 0, shift bytes next to none,
         mix_res 0 / positive / negative, LFE tags, instance tags 0 and 15
      6  fillers of every count form between any two elements and in front of END
      7  loud anti-phase pairs
      8  the malformed classes on purpose: an explicit count above FrameLength (a pair in the last output slot comes with 1)

    budget: at most that many compositions per item, drawn with rng (the long frame lengths); None: all. override: Elem
    settings forced on every element (KB 0 is lossless for escape elements only: the synth's Golomb coder needs k >= 1)."""
    nc, fl = num_channels, frame_length
    cookie = dict(COOKIES["std"] if cookie is None else cookie)
    mk = _Maker(synth, oracle, depth, fl, cookie, rng, override)
    out = []
    comps = compositions(nc)
    full = [c for c in comps if sum(c) >= nc]  # ends the walk by itself

    def pick(cs):
        cs = list(cs)
        if budget is None or len(cs) <= budget:
            return cs
        idx = sorted(rng.choice(len(cs), size=budget, replace=False).tolist())
        return [cs[k] for k in idx]

    def build(comp, counts, style="music", lfe_at=(), settings=None):
        seq = []
        for k, (kind, (frames, explicit)) in enumerate(zip(_kinds(comp, lfe_at), counts)):
            kw = dict(settings[k]) if settings else {}
            seq.append(mk.item(kind, frames, explicit, style=kw.pop("style", style), **kw))
        return seq

    def add(name, seq, end=True):
        out.append((name, packet_of(seq, end=end), seq))

    def tag(comp):
        return "".join("SC"[w - 1] for w in comp) or "-"

    patterns = ["full", "first", "grow", "shrink", "one", "flagged_full", "last_one", "zigzag"]
    # 1 -------------------------------------------------------------------------------------------------------------
    for k, comp in enumerate(pick(comps)):
        pat = patterns[k % len(patterns)]
        a = max(1, fl - 1 - k % 5)
        seq = build(comp, _counts(pat, len(comp), fl, a), lfe_at=(len(comp) - 1,) if k % 3 == 0 else ())
        add("1 %s %s end" % (tag(comp), pat), seq)
        if comp in full:
            add("1 %s %s noend" % (tag(comp), pat), seq, end=False)
    # 2 -------------------------------------------------------------------------------------------------------------
    canon = tuple(2 if t == 1 else 1 for t in [[0], [1], [0, 1], [0, 1, 0], [0, 1, 1], [0, 1, 1, 3], [0, 1, 1, 0, 3], [0, 1, 1, 1, 3]][nc - 1])
    for comp in {canon, (1,) * nc}:
        for pat in ("full", "grow"):
            seq = build(comp, _counts(pat, len(comp), fl, max(1, fl - 2)))
            for k in range(len(comp)):
                add("2 %s %s END@%d" % (tag(comp), pat, k), seq[:k] + [("END",)] + seq[k:])
    # 3 -------------------------------------------------------------------------------------------------------------
    trio = [c for c in {canon, (1,) * nc, tuple([1] + [2] * ((nc - 1) // 2) + [1] * ((nc - 1) % 2))} if walk(nc, [(("CPE" if w == 2 else "SCE"),) for w in c])["pair_last"] is False]
    for comp in trio:
        for pat in patterns:
            add("3 %s %s" % (tag(comp), pat), build(comp, _counts(pat, len(comp), fl, max(1, fl * 2 // 3))))
        for c in edge_counts(fl):
            for pat in ("first", "grow", "shrink", "zigzag"):
                if len(comp) == 1 and pat != "first":
                    continue
                add("3 %s %s@%d" % (tag(comp), pat, c), build(comp, _counts(pat, len(comp), fl, c)))
    # 4 -------------------------------------------------------------------------------------------------------------
    meet = [c for c in comps if walk(nc, [(("CPE" if w == 2 else "SCE"),) for w in c])["overlap"]]
    for k, comp in enumerate(pick(meet)):
        for pat in ("full", "shrink", "grow"):
            style = "antiphase" if (k + len(pat)) % 2 else "music"
            add("4 %s %s" % (tag(comp), pat), build(comp, _counts(pat, len(comp), fl, fl), style=style), end=k % 2 == 0 or comp not in full)
    # 5 -------------------------------------------------------------------------------------------------------------
    wide = dict(bytes_shifted=0) if depth in (24, 32) else {}
    pool = [dict(force_escape=1), dict(order=4, never_escape=1), dict(order=0, never_escape=1), dict(order=8, mix_res=0, never_escape=1),
            dict(order=5, mix_res=-3, mix_bits=2, never_escape=1), dict(order=1, never_escape=1, instance=15),
            dict(order=6, mode_u=1, mode_v=1, never_escape=1), dict(order=9, mix_res=2, mix_bits=3, never_escape=1, **wide),
            dict(order=16, never_escape=1, instance=0), dict(order=31, never_escape=1), dict(order=4, den_shift=4, pb_factor=7, never_escape=1, **wide),
            dict(force_escape=1, instance=15), dict(order=8, mode_u=3, never_escape=1)]
    paper = [dict(order=17, never_escape=1), dict(order=30, never_escape=1)]  # no lean instantiation: the whole packet is legacy
    mixed = [c for c in {canon, (1,) * nc, tuple([1] * (nc % 2) + [2] * (nc // 2))} if not walk(nc, [(("CPE" if w == 2 else "SCE"),) for w in c])["pair_last"]]
    for comp in mixed + [c for c in pick(meet)[:2] if c not in mixed]:
        n = len(comp)
        for r in range(len(pool)):
            st = []
            for k in range(n):
                s = dict(pool[(r + k) % len(pool)])
                # chanBits 33 (a 32-bit pair without shift bytes) decodes to zeros (predictor.go:46): one shift byte there
                if depth == 32 and comp[k] == 2 and s.get("bytes_shifted") == 0:
                    s["bytes_shifted"] = 1
                st.append(s)
            pat = ("full", "grow", "first")[r % 3]
            add("5 %s mix%d %s" % (tag(comp), r, pat), build(comp, _counts(pat, n, fl, max(1, fl - 3)), lfe_at=(r % n,), settings=st), end=r % 4 != 3 or comp not in full)
        for r, pp in enumerate(paper):
            st = [dict(pp) if k == r % n else dict(pool[(k + 1) % len(pool)]) for k in range(n)]
            for s, w in zip(st, comp):
                if depth == 32 and w == 2 and s.get("bytes_shifted") == 0:
                    s["bytes_shifted"] = 1
            add("5 %s paper%d" % (tag(comp), pp["order"]), build(comp, _counts("full", n, fl), settings=st))
    if nc <= 2:  # one or two channels: escape-only packets take the split route, everything else the whole-packet decoder
        for comp in [c for c in comps if c and sum(c) == nc]:
            add("5 %s escapes" % tag(comp), build(comp, _counts("first", len(comp), fl, max(1, fl - 1)), settings=[dict(force_escape=1)] * len(comp)))
    # 6 -------------------------------------------------------------------------------------------------------------
    for comp in mixed:
        seq = build(comp, _counts("grow", len(comp), fl, fl))
        for k in range(len(FILLERS)):
            p = k % (len(seq) + 1)
            add("6 %s %s%d@%d" % (tag(comp), FILLERS[k][0], FILLERS[k][1], p), seq[:p] + [FILLERS[k]] + seq[p:])
        every = []
        for k, it in enumerate(seq):
            every += [FILLERS[(2 * k) % len(FILLERS)], FILLERS[(2 * k + 5) % len(FILLERS)], it]
        add("6 %s everywhere" % tag(comp), every + [FILLERS[3]])
    # 7 -------------------------------------------------------------------------------------------------------------
    for comp in [c for c in pick(comps) if 2 in c][:24]:
        for pat in ("full", "shrink"):
            add("7 %s %s" % (tag(comp), pat), build(comp, _counts(pat, len(comp), fl, fl), style="antiphase"))
    # 8 -------------------------------------------------------------------------------------------------------------
    for comp in trio:
        for k in sorted({0, len(comp) - 1}):
            seq = build(comp, _counts("full", len(comp), fl))
            kind = seq[k][0]
            seq[k] = mk.item(kind, fl + 1 + k, True)
            add("8 %s over@%d" % (tag(comp), k), seq)
    return out
