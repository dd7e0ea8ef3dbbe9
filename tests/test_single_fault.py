"""Every one-bit fault and every truncation of small packets (tests/single_fault.py) on the CPU: the oracle's losslessness
on the intact packets, the kernel's decode logic as built for the host (tests/host_sim) against the oracle on the dense
layout, oracle/goref.py against the oracle as a second reading, and the reach of the corpus: which edges of
classify_regular (alac_regular.h) its packets cross.

lane_sim runs the decode logic as the HOST compiler builds it. It does not see the GPU build's intrinsics, LDS rings or
the hand-off between waves: tests/test_gpu_single_fault.py runs the same corpus there."""
import numpy as np
import pytest

from oracle import goref
from tests import single_fault as sf


def ids(configs):
    return ["-".join(map(str, c)) for c in configs]


def bpf_of(oracle, cfg):
    return cfg.num_channels * oracle.bytes_per_sample(cfg.bit_depth)


@pytest.mark.parametrize("depth,ch,fl,cookie", sf.CONFIGS, ids=ids(sf.CONFIGS))
def test_intact_seeds_decode_to_their_source(oracle, synth, depth, ch, fl, cookie):
    """The lossless property of tests/conformance_test.go:282-291 on every seed packet (KB 0: the synth's Golomb coder
    needs k >= 1, so only the escape seeds are lossless there)."""
    c = sf.corpus(synth, oracle, depth, ch, fl, cookie)
    bpf = bpf_of(oracle, c.cfg)
    assert len(c.seeds) == 60
    for i, s in enumerate(c.seeds):
        if cookie == "kb0" and s.row != "esc":
            continue
        assert c.seed_ref[2][i] == 0 and c.seed_ref[1][i] == s.frames, "%s %s: status %#x, %d frames" % (
            sf.cfg_name(c.cfg), s.name, c.seed_ref[2][i], c.seed_ref[1][i])
        assert c.seed_ref[0][i, :s.frames * bpf].tobytes() == s.pcm, "%s %s: the oracle lost the source PCM" % (sf.cfg_name(c.cfg), s.name)
        # the intact packet is also its own longest prefix
        j = s.first + s.npre - 1
        assert c.packets[j] == s.packet and c.ref[2][j] == 0


@pytest.mark.parametrize("depth,ch,fl", sf.COUNT_CONFIGS, ids=ids(sf.COUNT_CONFIGS))
def test_count_sweeps_decode_to_their_source_in_every_layout(oracle, synth, lane_sim, helpers, depth, ch, fl):
    """Every frame count 1..FrameLength and the loud few-frame packets around the ten-byte rule: lossless in the oracle, and
    the decode logic equals the oracle on the dense layout at every blob lead, against a guard page."""
    for name, cfg, items, ref in sf.sweeps(synth, oracle, depth, ch):
        bpf = bpf_of(oracle, cfg)
        packets = [p for _, p, _ in items]
        for i, (what, p, pcm) in enumerate(items):
            assert ref[2][i] == 0 and int(ref[1][i]) * bpf == len(pcm) and ref[0][i, :len(pcm)].tobytes() == pcm, "%s %s: %s" % (
                sf.cfg_name(cfg), name, what)
        for lead in (0, 1, 2, 3):
            blob, offs, sizes = helpers.pack_dense(packets, lead=lead)
            got = lane_sim(cfg, blob, offs, sizes, variant=-1, guard=True)
            bad = sf.first_difference(ref, got, bpf, lambda i: "%s %s lead %d: %s" % (sf.cfg_name(cfg), name, lead, items[i][0]))
            assert bad is None, bad


@pytest.mark.parametrize("depth,ch,fl,cookie", sf.CONFIGS, ids=ids(sf.CONFIGS))
def test_lane_logic_equals_the_oracle_on_every_fault(oracle, synth, lane_sim, helpers, depth, ch, fl, cookie):
    """Variant -1 (the library's routing) on every prefix and every flip of every seed, one blob per seed at a lead that
    rotates with the seed; on the faults of the o4, uv, esc and noshift seeds also variant -2 (split pipeline; the
    full-length seeds) and variant 3 (whole-packet decoder; the partial ones) — thinned to that because this file takes
    longer than tests/test_lane_logic.py; the corpus is whole. Dense blobs against a guard page: a read behind the blob is
    fatal."""
    c = sf.corpus(synth, oracle, depth, ch, fl, cookie)
    bpf = bpf_of(oracle, c.cfg)
    for k, s in enumerate(c.seeds):
        ref = tuple(r[s.first:s.end] for r in c.ref)
        blob, offs, sizes = helpers.pack_dense(c.packets[s.first:s.end], lead=k % 4)
        for variant in (-1, -2 if s.frames == fl else 3) if s.row in sf.VARIANT_ROWS else (-1,):
            got = lane_sim(c.cfg, blob, offs, sizes, variant=variant, guard=True)
            bad = sf.first_difference(ref, got, bpf, lambda i: "variant %d lead %d, %s" % (variant, k % 4, s.what(c.cfg, s.first + i)))
            assert bad is None, bad


@pytest.mark.parametrize("depth,ch,fl,cookie", sf.GOREF_CONFIGS, ids=ids(sf.GOREF_CONFIGS))
def test_goref_equals_the_oracle_on_every_fault(oracle, synth, depth, ch, fl, cookie):
    """A second reading of the reference on all faults of six seeds at both frame counts. The only packets left out are
    those of the documented deviation (a pair that does not fit the frame); they are counted."""
    c = sf.corpus(synth, oracle, depth, ch, fl, cookie)
    gc = goref.PacketConfig(fl, depth, ch, c.cfg.pb, c.cfg.mb, c.cfg.kb, c.cfg.max_run)
    bpf = bpf_of(oracle, c.cfg)
    picked = [s for s in c.seeds if "%s/%s" % (s.row, s.sig) in sf.GOREF_SEEDS]
    assert len(picked) == 12
    n, left_out = 0, 0
    for s in picked:
        for i in range(s.first, s.end):
            st, frames = int(c.ref[2][i]), int(c.ref[1][i])
            info = {}
            g_pcm, g_frames, g_st = goref.decode_packet(gc, c.packets[i], info=info)
            n += 1
            if st == 6 and info["cpe_last_slot"]:
                left_out += 1
                continue
            assert (g_st, g_frames) == (st, frames), "%s: oracle status %#x, %d frames; goref status %#x, %d frames" % (
                s.what(c.cfg, i), st, frames, g_st, g_frames)
            if st == 0:
                assert g_pcm == c.ref[0][i, :frames * bpf].tobytes(), "%s: PCM differs" % s.what(c.cfg, i)
    print("%s: goref on %d packets, %d left out" % (sf.cfg_name(c.cfg), n, left_out))
    assert left_out <= 0.005 * n, (left_out, n)


# ---- reach: the sweep must keep crossing the edges it is there for ---------------------------------------------------
def keys_of(lane_sim, helpers, cfg, packets):
    blob, offs, sizes = helpers.pack_dense(packets)
    return lane_sim(cfg, blob, offs, sizes, variant=-1, want_classes=True, guard=True)[3]


@pytest.mark.parametrize("depth,ch,fl,cookie", sf.CONFIGS, ids=ids(sf.CONFIGS))
def test_the_faults_reach_the_classifiers_edges(oracle, synth, lane_sim, helpers, depth, ch, fl, cookie):
    """Floors on what the oracle and classify_regular make of the corpus (conditions, below what they give today)."""
    c = sf.corpus(synth, oracle, depth, ch, fl, cookie)
    cfg, st = c.cfg, c.ref[2]
    assert (st == 0).mean() >= 0.5, (st == 0).mean()
    assert len(np.unique(st)) >= (6 if ch == 1 else 10), np.unique(st)
    if cookie != "std":
        return
    keys = keys_of(lane_sim, helpers, cfg, c.packets)
    seed_keys = keys_of(lane_sim, helpers, cfg, [s.packet for s in c.seeds])
    if (depth, ch, fl, cookie) not in sf.LEAN:
        assert (keys >= sf.KEY_IRREGULAR).all() and (seed_keys >= sf.KEY_IRREGULAR).all()
        return
    narrow = np.unique(keys[keys < sf.KEY_WIDE])
    wide = np.unique(keys[(keys >= sf.KEY_WIDE) & (keys < sf.KEY_IRREGULAR)])
    assert len(narrow) >= (40 if ch == 2 else 12), narrow
    if depth in (24, 32):
        assert len(wide) >= 8, wide
    regular = [(s, int(k)) for s, k in zip(c.seeds, seed_keys) if k < sf.KEY_IRREGULAR]
    assert len(regular) >= 20
    if depth in (24, 32):  # a quiet packet's entropy stream is shorter than ten bytes: irregular by the ten-byte rule
        assert any(k >= sf.KEY_IRREGULAR and s.sig == "quiet" and s.row not in ("o17", "mode", "esc", "fil") for s, k in zip(c.seeds, seed_keys))
    order_keys, order_irregular, count_own, count_irregular = set(), 0, 0, 0
    for s, own in regular:
        pre = keys[s.first:s.first + s.npre]
        assert (pre < sf.KEY_IRREGULAR).any() and (pre >= sf.KEY_IRREGULAR).any(), s.name
        assert pre[-1] == own
        for field, n in (("tag", 3), ("unused", 12), ("escape", 1), ("U.mode", 4)) + ((("V.mode", 4),) if ch == 2 else ()):
            idx = s.flip_index(cfg, field)
            assert len(idx) == n and (keys[idx] >= sf.KEY_IRREGULAR).all(), "%s: %s" % (s.name, field)
        for field in ("U.order", "V.order")[:ch]:
            k = keys[s.flip_index(cfg, field)]
            assert len(k) == 5
            order_irregular += int((k >= sf.KEY_IRREGULAR).sum())
            order_keys |= {(s.name, int(x)) for x in k if x < sf.KEY_IRREGULAR and x != own}
        if s.frames != fl:
            k = keys[s.flip_index(cfg, "count")]
            assert len(k) == 32
            count_own += int((k == own).sum())
            count_irregular += int((k >= sf.KEY_IRREGULAR).sum())
    assert order_irregular >= 1 and len({k for _, k in order_keys}) >= 3, (order_irregular, order_keys)
    assert count_own >= 1 and count_irregular >= 1, (count_own, count_irregular)


@pytest.mark.parametrize("depth,ch,fl", sf.COUNT_CONFIGS, ids=ids(sf.COUNT_CONFIGS))
def test_the_count_sweeps_cross_the_ten_byte_rule(oracle, synth, lane_sim, helpers, depth, ch, fl):
    """With shift bytes the frame count decides on which side of the ten-byte rule a quiet packet falls: both sides at 24
    and 32 bits, regular keys only at 16. Every loud-counts set holds entropy streams of 8-9 and of 10-11 bytes, with
    irregular keys among the former and regular ones among the latter."""
    for name, cfg, items, ref in sf.sweeps(synth, oracle, depth, ch):
        keys = keys_of(lane_sim, helpers, cfg, [p for _, p, _ in items])
        if name == "counts":
            q = keys[[i for i, it in enumerate(items) if it[0].endswith("/quiet")]]
            assert len(q) == fl
            if depth == 16:
                assert (keys < sf.KEY_IRREGULAR).all()
            else:
                assert (q < sf.KEY_IRREGULAR).any() and (q >= sf.KEY_IRREGULAR).any()
        else:
            eb = np.array([sf.entropy_bytes(cfg, p) for _, p, _ in items])
            assert ((eb == 8) | (eb == 9)).any() and ((eb == 10) | (eb == 11)).any(), np.unique(eb)
            assert (keys[eb < 10] >= sf.KEY_IRREGULAR).any() and (keys[eb >= 10] < sf.KEY_IRREGULAR).any()
