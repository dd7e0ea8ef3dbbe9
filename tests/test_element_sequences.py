"""Packets whose element order is not the channel layout's own (tests/element_splice.py), on the CPU: the model of the
reference's element walk against both restatements of the reference (oracle, goref), and the kernel's decode logic as
built for the host (tests/host_sim) against the oracle, route by route."""
import collections

import numpy as np
import pytest

from oracle import goref
from tests import element_splice as es

ROUTE_NONE, ROUTE_SPLIT, ROUTE_LEGACY = 2048, 2049, 2050  # lane_sim's classes: 2048 + PktDesc.route (alac_wave.h)
VARIANTS = (-1, -2, 0, 1, 2, 3)
DEPTHS = (16, 20, 24, 32)


def goref_cfg(cfg):
    return goref.PacketConfig(cfg.frame_length, cfg.bit_depth, cfg.num_channels, cfg.pb, cfg.mb, cfg.kb, cfg.max_run)


def seed_of(depth, ch, fl, salt=0):
    return [depth, ch, fl, salt]


def decode_all(oracle, helpers, cfg, packets):
    blob, offs, sizes = helpers.pack_packets(packets)
    return (blob, offs, sizes), oracle.decode_batch(cfg, blob, offs, sizes, threads=4)


def check_model(synth, cfg, corpus, ref):
    """Every "ok" packet: status 0, the model's frame count and the model's bytes; every "malformed" one: bare status 6 and
    no frames, and nothing but the two classes the model knows. -> (the model's answers, malformed packets per class)"""
    nc, fl = cfg.num_channels, cfg.frame_length
    bpf = nc * {16: 2, 20: 3, 24: 3, 32: 4}[cfg.bit_depth]
    answers, classes = [], collections.Counter()
    for i, (name, _, seq) in enumerate(corpus):
        e = es.expected(nc, fl, seq)
        answers.append(e)
        if e[0] == "ok":
            assert ref[2][i] == 0 and ref[1][i] == e[1], "%s: oracle status %#x frames %d, model %d frames" % (name, ref[2][i], ref[1][i], e[1])
            want = np.frombuffer(synth.pack_pcm(cfg, e[2]), np.uint8)
            got = ref[0][i, :e[1] * bpf]
            assert np.array_equal(got, want), "%s: oracle and model differ at byte %d" % (name, np.nonzero(got != want)[0][0])
        else:
            assert ref[2][i] == 6 and ref[1][i] == 0, "%s: oracle status %#x, the model says malformed" % (name, ref[2][i])
            classes["pair in the last slot" if es.walk(nc, seq)["pair_last"] else "count above FrameLength"] += 1
            if not es.walk(nc, seq)["pair_last"]:
                assert any(it[0] in es.AUDIO and it[1] is not None and it[1] > fl for it in seq), name
    return answers, classes


def check_goref(cfg, corpus, ref, picks):
    gc = goref_cfg(cfg)
    bpf = cfg.num_channels * {16: 2, 20: 3, 24: 3, 32: 4}[cfg.bit_depth]
    for i in picks:
        info = {}
        pcm, frames, st = goref.decode_packet(gc, corpus[i][1], info=info)
        if ref[2][i] == 6 and info["cpe_last_slot"]:
            continue  # the documented deviation: the reference writes outside the frame
        assert (st, frames) == (ref[2][i], ref[1][i]), "%s: goref status %#x frames %d" % (corpus[i][0], st, frames)
        assert pcm == ref[0][i, :frames * bpf].tobytes(), "%s: goref PCM" % corpus[i][0]


def goref_share(corpus, rng, extra):
    """The first packet of every composition and of every (item, pattern), and `extra` seeded ones."""
    first = {}
    for i, (name, _, _) in enumerate(corpus):
        w = name.split()
        first.setdefault(("comp", w[1]), i)
        first.setdefault((w[0], w[2].split("@")[0] if len(w) > 2 else ""), i)
    picks = set(first.values()) | set(rng.choice(len(corpus), size=min(extra, len(corpus)), replace=False).tolist())
    return sorted(picks)


def check_lanes(lane_sim, helpers, cfg, packed, ref, answers, variants=VARIANTS):
    """Every variant at the aligned stride and at stride_pad 4: the oracle's status, frames and PCM; a channel the model
    leaves zero reads zero inside the frames although lane_sim poisons the slot first. -> routing of variant -1"""
    blob, offs, sizes = packed
    nc = cfg.num_channels
    bps = {16: 2, 20: 3, 24: 3, 32: 4}[cfg.bit_depth]
    bpf = nc * bps
    classes = None
    for variant in variants:
        for pad in (0, 4):
            got = lane_sim(cfg, blob, offs, sizes, variant=variant, stride_pad=pad, want_classes=True)
            helpers.assert_same_decode(cfg, ref, got[:3], bpf, "variant %d pad %d" % (variant, pad))
            if variant == -1 and pad == 0:
                classes = got[3]
            for i, e in enumerate(answers):
                if e[0] == "ok" and e[1]:
                    zero = ~e[2].any(axis=0)  # channels nobody wrote, or wrote zeros to
                    pcm = got[0][i, :e[1] * bpf].reshape(e[1], nc, bps)
                    assert not pcm[:, zero].any(), "variant %d pad %d packet %d: an unwritten channel is not zero" % (variant, pad, i)
    return classes


def check_reach(cfg, corpus, answers, classes):
    """Conditions on the corpus (not measurements): it cannot shrink without this failing."""
    nc, fl = cfg.num_channels, cfg.frame_length
    lean = cfg.kb != 0 and cfg.pb <= 73  # alac_regular.h: lean_config
    items = {name.split()[0] for name, _, _ in corpus}
    assert items >= ({"1", "2", "3", "5", "6", "8"} | ({"7"} if nc >= 2 else set()) | ({"4"} if nc >= 4 else set())), items
    ok = [i for i, e in enumerate(answers) if e[0] == "ok"]
    counts = collections.defaultdict(set)
    for i in ok:
        counts[int(classes[i])].add(len(es.walk(nc, corpus[i][2])["writes"]))
    if not lean:  # every packet takes the whole-packet decoder; lane_sim reports no scan route for it
        assert not (set(counts) & {ROUTE_SPLIT, ROUTE_LEGACY}), sorted(counts)
    elif nc > 2:
        assert counts[ROUTE_SPLIT] >= set(range(0, nc + 1)), (nc, sorted(counts[ROUTE_SPLIT]))
        assert len(counts[ROUTE_LEGACY]) >= 1, "no packet on ROUTE_LEGACY"
        assert set(counts) <= {ROUTE_SPLIT, ROUTE_LEGACY}
    else:
        assert counts[ROUTE_SPLIT] and counts[ROUTE_LEGACY], "1-2 channels: the escape-only split route and the whole-packet route"
        assert fl <= 32 or any(k < 2048 for k in counts), "no packet on the wave pairs"
    if nc >= 4:
        assert sum(1 for i in ok if es.walk(nc, corpus[i][2])["overlap"]) >= 6
    assert sum(1 for i in ok if es.walk(nc, corpus[i][2])["quiet"]) >= (1 if nc > 1 else 0)
    part = [answers[i][1] for i in ok]
    assert min(part) == 1 and max(part) == fl and len(set(part)) >= 5
    # one frame count per written channel differs: a slot written for fewer frames than the packet has
    assert nc == 1 or any(len({it[2].shape[0] for it in corpus[i][2] if it[0] in es.AUDIO}) > 1 for i in ok)


def count_shrinking(nc, fl, corpus):
    """Packets in which a decoded element holds more frames than the packet does."""
    n = 0
    for _, _, seq in corpus:
        e = es.expected(nc, fl, seq)
        audio = [it for it in seq if it[0] in es.AUDIO]  # the walk decodes a prefix of them
        held = [it[2].shape[0] for it in audio[:len(es.walk(nc, seq)["writes"])]]
        n += e[0] == "ok" and bool(held) and max(held) > e[1]
    return n


CASES = [(d, c, fl) for d in DEPTHS for c in range(1, 9) for fl in (40, 300)]


@pytest.mark.parametrize("depth,ch,fl", CASES)
def test_spliced_sequences(oracle, synth, lane_sim, helpers, depth, ch, fl):
    """The whole corpus of one stream config: model == oracle (== goref on a share), every lane_sim variant == oracle,
    unwritten channels zero, and the corpus reaches every route."""
    rng = np.random.default_rng(seed_of(depth, ch, fl))
    cfg = oracle.make_config(fl, depth, ch)
    corpus = es.CORPUS(synth, oracle, depth, ch, fl, rng)
    packed, ref = decode_all(oracle, helpers, cfg, [p for _, p, _ in corpus])
    answers, mal = check_model(synth, cfg, corpus, ref)
    assert mal["count above FrameLength"] >= 1 and set(mal) <= {"pair in the last slot", "count above FrameLength"}
    # which channel counts can put a pair in the last output slot follows from the layout table (decoder.go:55-64)
    can = any(o + 2 > ch for k, o in enumerate(es.LAYOUT[ch - 1]) if k + 2 <= ch)
    assert can == (ch in (3, 6, 7, 8)) and (mal["pair in the last slot"] >= 2) == can, dict(mal)
    check_goref(cfg, corpus, ref, goref_share(corpus, rng, 24) if fl == 40 else sorted(rng.choice(len(corpus), 10, replace=False).tolist()))
    classes = check_lanes(lane_sim, helpers, cfg, packed, ref, answers)
    check_reach(cfg, corpus, answers, classes)


@pytest.mark.parametrize("depth,ch,fl,cookie,budget", [
    (16, 2, 300, "pb255", None), (24, 6, 40, "pb255", None), (20, 5, 300, "pb255", None), (32, 8, 40, "pb255", None),
    (16, 8, 40, "kb0", None), (32, 3, 40, "kb0", None), (24, 2, 300, "kb0", None),
    (16, 2, 4096, "std", 6), (24, 8, 4096, "std", 6), (32, 5, 1030, "std", 8)])
def test_spliced_sequences_other_cookies_and_long_frames(oracle, synth, lane_sim, helpers, depth, ch, fl, cookie, budget):
    """PB 255 and KB 0 are not lean_config (alac_regular.h): every packet takes the whole-packet decoder. The long frame
    lengths run every item on a seeded choice of compositions; their counts straddle 256 and 1024."""
    rng = np.random.default_rng(seed_of(depth, ch, fl, 1))
    cfg = oracle.make_config(fl, depth, ch, **es.COOKIES[cookie])
    # KB 0: Golomb codes of k = 0 (golomb.go:171-173), which the synth's coder cannot write losslessly: the model holds
    # for escape elements only, and the corpus with compressed elements is compared decoder against decoder
    corpus = es.CORPUS(synth, oracle, depth, ch, fl, rng, cookie=es.COOKIES[cookie], budget=budget,
                       override=dict(force_escape=1) if cookie == "kb0" else None)
    if cookie == "kb0":
        lossy = es.CORPUS(synth, oracle, depth, ch, fl, rng, cookie=es.COOKIES[cookie])
        packed, ref = decode_all(oracle, helpers, cfg, [p for _, p, _ in lossy])
        assert (ref[2] == 0).sum() > len(lossy) // 2
        check_lanes(lane_sim, helpers, cfg, packed, ref, [])
    packed, ref = decode_all(oracle, helpers, cfg, [p for _, p, _ in corpus])
    answers, mal = check_model(synth, cfg, corpus, ref)
    assert mal["count above FrameLength"] >= 1
    check_goref(cfg, corpus, ref, sorted(rng.choice(len(corpus), 12 if fl <= 300 else 2, replace=False).tolist()))
    classes = check_lanes(lane_sim, helpers, cfg, packed, ref, answers, variants=(-1, -2, 0, 3) if fl > 300 else VARIANTS)
    check_reach(cfg, corpus, answers, classes)
    if fl >= 1030:
        fr = {e[1] for e in answers if e[0] == "ok"}
        assert fr >= {255, 256, 257, 1023, 1024, 1025}, sorted(fr)


@pytest.mark.parametrize("depth,ch,fl,cookie", [(16, 2, 40, "std"), (16, 2, 300, "std"), (24, 2, 300, "pb255"), (16, 4, 40, "std"),
                                                 (24, 6, 300, "std"), (32, 8, 40, "pb255"), (20, 5, 40, "kb0"), (32, 1, 40, "std"),
                                                 (16, 3, 40, "std"), (24, 8, 300, "std"), (20, 7, 40, "std")])
def test_no_element_writes_behind_the_packets_frames(oracle, synth, lane_sim, helpers, depth, ch, fl, cookie):
    """The packet's frame count is the LAST element's; an element in front of it may hold more (SCE 26 frames, SCE 8 frames in
    a stereo stream is an 8-frame packet). The device entry's footprint (include/alacgpu.h) is [0, frames * bytes per frame)
    of the slot and nothing else. Found by this corpus: the whole-packet decoder wrote every element's own frames, so with
    shrinking counts the first element's samples landed behind the packet's frames — first seen at 16-bit 2-channel
    FrameLength 40, packet `3 SS shrink` (SCE 26 frames, SCE 8 frames), byte 32 of the slot = frame 8 channel 0, routes
    ROUTE_LEGACY (2 channels) and every whole-packet variant. lane_sim poisons the slot with 0xa5 first."""
    rng = np.random.default_rng(seed_of(depth, ch, fl, 2))
    cfg = oracle.make_config(fl, depth, ch, **es.COOKIES[cookie])
    bpf = ch * oracle.bytes_per_sample(depth)
    corpus = [c for c in es.CORPUS(synth, oracle, depth, ch, fl, rng, cookie=es.COOKIES[cookie]) if c[0].split()[0] in "1345"]
    (blob, offs, sizes), ref = decode_all(oracle, helpers, cfg, [p for _, p, _ in corpus])
    assert count_shrinking(ch, fl, corpus) >= (4 if ch > 1 else 0)
    for variant in (-1, -2, 0, 3):
        for pad in (0, 4):
            out, fr, st = lane_sim(cfg, blob, offs, sizes, variant=variant, stride_pad=pad)
            for i in np.nonzero(st == 0)[0]:
                tail = out[i, int(fr[i]) * bpf:]
                assert (tail == 0xa5).all(), "variant %d pad %d %s: byte %d of the slot written, the packet has %d frames" % (
                    variant, pad, corpus[i][0], int(fr[i]) * bpf + np.nonzero(tail != 0xa5)[0][0], fr[i])


def _set_bits(bits, at, value, n):
    out = bits.copy()
    out[at:at + n] = es.to_bits(value, n)
    return out


@pytest.mark.parametrize("depth,ch,fl,cookie", [(16, 2, 40, "std"), (16, 3, 40, "std"), (24, 4, 40, "std"), (20, 5, 40, "std"),
                                                 (16, 6, 300, "std"), (32, 7, 40, "std"), (24, 8, 40, "std"), (16, 8, 40, "pb255"),
                                                 (32, 4, 40, "kb0")])
def test_errors_in_later_elements(oracle, synth, lane_sim, helpers, depth, ch, fl, cookie):
    """The element that fails is not the first: packets cut at every byte of their last 64 bytes and at every element
    boundary, non-zero unused header bits, bytesShifted 3, CCE / PCE in the 2nd, 3rd and last position, fillers that run off
    the packet. Status words — code, context and stage — must be the oracle's (and goref's on a share)."""
    rng = np.random.default_rng(seed_of(depth, ch, fl, 3))
    cfg = oracle.make_config(fl, depth, ch, **es.COOKIES[cookie])
    bpf = ch * oracle.bytes_per_sample(depth)
    mk = es._Maker(synth, oracle, depth, fl, es.COOKIES[cookie], rng)
    comps = [c for c in es.compositions(ch) if sum(c) == ch and len(c) >= 2
             and not es.walk(ch, [(("CPE" if w == 2 else "SCE"),) for w in c])["pair_last"]]
    comps = [comps[k] for k in sorted(rng.choice(len(comps), size=min(4, len(comps)), replace=False).tolist())]
    packets = []
    for comp in comps:
        for kw in (dict(never_escape=1), dict(force_escape=1), dict(never_escape=1, order=8, mode_u=1)):
            # the first and the last element carry their own counts, the ones between take the first one's
            seq = [mk.item("CPE" if w == 2 else "SCE", max(1, fl // 2) if k == len(comp) - 1 else fl - 1, k in (0, len(comp) - 1), **kw)
                   for k, w in enumerate(comp)]
            parts = es.parts_of(seq)
            whole = es.compose(parts)
            cuts = set(range(max(1, len(whole) - 64), len(whole)))
            pos = 0
            for p in parts:  # ... and inside every element: its header, a pair's U and V streams
                cuts |= {(pos + len(p) * f // 16) // 8 for f in (1, 4, 6, 8, 10, 12, 14, 15)}
                pos += len(p)
                cuts |= {pos // 8, pos // 8 + 1}
            packets += [whole[:k] for k in sorted(cuts) if 0 < k <= len(whole)]
            for k in sorted({1, min(2, len(seq) - 1), len(seq) - 1}):
                bits = seq[k][3]
                for bad in (_set_bits(bits, 7 + int(rng.integers(12)), 1, 1), _set_bits(bits, 20, 3, 2), es.to_bits(2, 3), es.to_bits(5, 3)):
                    packets.append(es.compose(parts[:k] + [bad] + parts[k + 1:]))
                # fillers that announce more bytes than the packet has left
                for f, nbytes in ((es.fil(269), 269), (es.fil(14), 14), (es.dse(510, 1), 510), (es.dse(254, 0), 254)):
                    q = es.compose(parts[:k] + [f])
                    packets.append(q[:len(q) - nbytes // 2 - 1])
    (blob, offs, sizes), ref = decode_all(oracle, helpers, cfg, packets)
    codes = {int(s) & 0xff for s in ref[2]}
    assert codes >= {1, 3, 4, 5}, sorted(codes)                      # overrun, header, shift, CCE / PCE
    ctx = {(int(s) >> 8) & 0xf for s in ref[2] if s}
    assert ctx >= ({1, 2, 3, 4} if any(2 in c for c in comps) else {1, 3, 4}), sorted(ctx)  # SCE/LFE, CPE, DSE, FIL
    stages = {(int(s) >> 12) & 3 for s in ref[2]}
    print("codes", sorted(codes), "contexts", sorted(ctx), "stages", sorted(stages), "packets", len(packets))
    assert stages >= {0} | ({1} if any(1 in c for c in comps) else set()) | ({2, 3} if any(2 in c for c in comps) else set()), sorted(stages)
    for variant in (-1, -2, 0, 3):
        for pad in (0, 4):
            got = lane_sim(cfg, blob, offs, sizes, variant=variant, stride_pad=pad)
            helpers.assert_same_decode(cfg, ref, got, bpf, "variant %d pad %d" % (variant, pad))
    corpus = [("cut %d" % i, p, None) for i, p in enumerate(packets)]
    check_goref(cfg, corpus, ref, sorted(rng.choice(len(packets), size=min(40 if fl == 40 else 8, len(packets)), replace=False).tolist()))
