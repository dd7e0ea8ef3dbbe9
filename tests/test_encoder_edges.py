"""Edge-case PCM (tests/edge_pcm.py) through the encoder's logic and the decoder's logic on the CPU: digital silence, clicks at
a packet's ends, zero runs at and around the 65 535 cap, dual mono, full-scale DC / Nyquist / anti-phase, noise bursts out
of silence, samples that live in the shift bytes; short last packets of 1..9 frames.

For every case: the host build of the encoder (tests/host_sim/enc_sim.cpp) round-trips through the oracle, every packet equals
synth's writer with its header's parameters (the bit-exact pin), and the host build of the decoder kernels (lane_sim) decodes
every packet to the oracle's bytes in every class variant. The edges are not assumed: oracle.goref's trace (the independent
pure-Python restatement of the reference) shows the zero runs, escape codes and mean clamps each signal is here for."""
import numpy as np
import pytest

from oracle import goref
from tests import edge_pcm
from tests.test_encoder_host import BPS, EncSim, header_elem, oracle_round_trip

EXTRA = (0, 1, 2, 8, 9)  # frames of the short last packet: none, fewer than the order-8 filter's taps, and one more


@pytest.fixture(scope="module")
def enc_sim():
    return EncSim()


class Case:
    pass


def encode_case(enc_sim, synth, oracle, name, depth, ch, fl, total, seed=0):
    c = Case()
    c.cfg = oracle.make_config(fl, depth, ch)
    c.pcm = edge_pcm.make(name, synth, c.cfg, total, seed)
    assert c.pcm.shape == (total, ch) and c.pcm.dtype == np.int32
    c.total = total
    c.pcm_bytes = synth.pack_pcm(c.cfg, c.pcm)
    c.blob, c.offsets, c.esc, c.starts = enc_sim.encode(c.cfg, c.pcm_bytes, total, want_starts=True)
    c.n = len(c.offsets) - 1
    return c


def packet(c, i):
    return c.blob[int(c.offsets[i]):int(c.offsets[i + 1])].tobytes()


def check_case(c, synth, oracle, lane_sim, helpers, variants=(-1, -2, 0, 1, 2, 3)):
    """round trip, pin, lane_sim in every variant -> lane_sim's classes (variant -1)"""
    cfg, fl = c.cfg, c.cfg.frame_length
    oracle_round_trip(oracle, cfg, c.blob, c.offsets, c.pcm_bytes, c.total)
    ne = synth.num_elements(cfg.num_channels)
    for i in range(c.n):
        pkt = packet(c, i)
        elems = [header_elem(synth, cfg, pkt, int(c.starts[i, e])) for e in range(ne)]
        assert all(bool(el.force_escape) == bool(c.esc[i] >> e & 1) for e, el in enumerate(elems))
        assert synth.encode_packet(cfg, elems, c.pcm[i * fl:(i + 1) * fl]) == pkt, "packet %d differs from synth" % i
    offs = c.offsets[:-1].copy()
    sizes = np.diff(c.offsets).astype(np.uint32)
    blob = c.blob if len(c.blob) else np.zeros(1, np.uint8)
    ref = oracle.decode_batch(cfg, blob, offs, sizes, threads=8)
    bpf = cfg.num_channels * BPS[cfg.bit_depth]
    classes = None
    for v in variants:
        got = lane_sim(cfg, blob, offs, sizes, variant=v, want_classes=True)
        helpers.assert_same_decode(cfg, ref, got[:3], bpf, "variant %d" % v)
        if v == -1:
            classes = got[3]
    return classes


def chains(c, i):
    """goref decode of packet i (must be the source PCM) -> one list per compressed chain, in bitstream order, of
    ("code", index, k, residual, zmode, mean after it) and ("zrun", first index, length, m)"""
    cfg = c.cfg
    g = goref.PacketConfig(cfg.frame_length, cfg.bit_depth, cfg.num_channels, cfg.pb, cfg.mb, cfg.kb, cfg.max_run)
    t = []
    pcm, frames, st = goref.decode_packet(g, packet(c, i), trace=t)
    fl, bpf = cfg.frame_length, cfg.num_channels * BPS[cfg.bit_depth]
    assert st == 0 and pcm == c.pcm_bytes[i * fl * bpf:(i + 1) * fl * bpf]
    out, pos = [], 0
    for e in t:
        if e[0] == "code":
            if e[1] == 0:
                out.append([])
            out[-1].append(("code", e[1], e[2], e[3], e[4], e[6]))
            pos = e[1] + 1
        elif e[0] == "zrun":
            out[-1].append(("zrun", pos, e[3], e[2]))
            pos += e[3]
    return out


def runs(chain):
    return [e for e in chain if e[0] == "zrun"]


def escapes(chain):
    """codes whose quotient reached the escape (residual // (2^k - 1) >= 9: the encoder writes 9 ones and a literal)"""
    return [e for e in chain if e[0] == "code" and e[3] // ((1 << e[2]) - 1) >= 9]


# ---- every signal through the matrix -------------------------------------------------------------------------------------
NAMES = [n for n in edge_pcm.SIGNALS if n != "run_ladder"]
SHORT = [(name, d, ch, EXTRA[(i + j) % 5]) for i, name in enumerate(NAMES) for j, (d, ch) in
         enumerate((d, ch) for d in (16, 20, 24, 32) for ch in (1, 2, 8 if d in (16, 24) else 6))]


@pytest.mark.parametrize("name,depth,ch,extra", SHORT)
def test_edge_signals_at_4096_frames(enc_sim, synth, oracle, lane_sim, helpers, name, depth, ch, extra):
    c = encode_case(enc_sim, synth, oracle, name, depth, ch, 4096, 2 * 4096 + extra)
    check_case(c, synth, oracle, lane_sim, helpers)
    if name in ("silence", "click_first", "click_last", "dual_mono", "low_byte_only"):
        assert not c.esc[:c.total // 4096].any(), "full packets of these compress whatever the depth"


LONG = [(name, d, ch, EXTRA[i % 5]) for i, (name, d, ch) in enumerate(
    (name, d, ch) for name in ("silence", "click_first", "click_last", "dual_mono", "bursts", "antiphase_full", "dc_min")
    for d, ch in ((16, 1), (16, 2), (24, 2), (32, 1)))]


@pytest.mark.parametrize("name,depth,ch,extra", LONG)
def test_edge_signals_at_65536_frames(enc_sim, synth, oracle, lane_sim, helpers, name, depth, ch, extra):
    """the longest regular packets: mono and stereo 16-bit at frame_length 65 536 take the wave-pair decoder (lane_sim's class
    < 2048) unless an element went out raw; with shift bytes, the silent and clicked packets have fewer than ten bytes of
    entropy stream behind the shift block and take the scan route (alac_regular.h: classify_regular)"""
    c = encode_case(enc_sim, synth, oracle, name, depth, ch, 65536, 65536 + extra)
    classes = check_case(c, synth, oracle, lane_sim, helpers, variants=(-1, -2, 0, 3))
    for i in range(c.n):
        if depth == 16 and not c.esc[i] and c.offsets[i + 1] - c.offsets[i] >= 12:
            assert classes[i] < 2048, "packet %d of %s is not regular" % (i, name)


@pytest.mark.parametrize("depth,ch", [(16, 1), (16, 2), (20, 2), (24, 1), (32, 2)])
def test_run_ladder_round_trips(enc_sim, synth, oracle, lane_sim, helpers, depth, ch):
    """LADDER_FL > 65 536: the packets take the scan route (lane_sim class 2048 + route)"""
    c = encode_case(enc_sim, synth, oracle, "run_ladder", depth, ch, edge_pcm.LADDER_FL, 7 * edge_pcm.LADDER_FL + 2)
    assert not c.esc.any()
    classes = check_case(c, synth, oracle, lane_sim, helpers, variants=(-1, -2, 0, 3))
    assert (classes >= 2048).all()


# ---- the edges are there ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,ch", [(16, 1), (16, 2), (24, 2)])
def test_silence_at_65536_is_one_code_and_one_full_run_to_the_last_sample(enc_sim, synth, oracle, lane_sim, helpers, depth, ch):
    c = encode_case(enc_sim, synth, oracle, "silence", depth, ch, 65536, 65536)
    classes = check_case(c, synth, oracle, lane_sim, helpers, variants=(-1,))
    assert (classes[0] < 2048) == (depth == 16), "regular without a shift block"
    ch_list = chains(c, 0)
    assert len(ch_list) == ch
    for chain in ch_list:  # mono, and U and V of the pair: the run of 65 535 from index 1 ends on the chain's last sample
        assert chain == [("code", 0, chain[0][2], 0, 0, chain[0][5]), ("zrun", 1, 65535, chain[1][3])]


def test_run_ladder_has_every_run_it_promises(enc_sim, synth, oracle):
    """mono 16-bit: the run lengths of LADDER_RUNS in order, each packet's last run reaching the chain's last sample; runs of
    26 / 27 behind a click with m = 3 and of 2 294 / 2 295 behind a full run with m = 255, either side of the escape"""
    c = encode_case(enc_sim, synth, oracle, "run_ladder", 16, 1, edge_pcm.LADDER_FL, 7 * edge_pcm.LADDER_FL)
    fl = edge_pcm.LADDER_FL
    for p in range(7):
        (chain,) = chains(c, p)
        lens = [r[2] for r in runs(chain)]
        want = edge_pcm.LADDER_RUNS[p]
        it = iter(lens)
        assert all(any(x == w for x in it) for w in want), "packet %d: runs %s, want %s in order" % (p, lens, want)
        last = chain[-1]
        assert last[0] == "code" and last[1] == fl - 1 or last[0] == "zrun" and last[1] + last[2] == fl
        full = [r for r in runs(chain) if r[2] == edge_pcm.MAX_RUN]
        if p > 0:  # a full run with samples after it: the next code has zmode 0 (the reset of golomb.go:243)
            k = chain.index(full[0])
            assert k + 1 < len(chain) and chain[k + 1][0] == "code" and chain[k + 1][4] == 0
    (chain,) = chains(c, 0)
    m3 = [r for r in runs(chain) if r[2] in (26, 27)]
    assert [(r[2], r[3]) for r in m3] == [(26, 3), (27, 3)]
    for p, n in ((3, edge_pcm.RUN_ESC_M255 - 1), (4, edge_pcm.RUN_ESC_M255)):
        (chain,) = chains(c, p)
        assert (n, 255) in [(r[2], r[3]) for r in runs(chain)]
    (chain,) = chains(c, 6)
    assert [r[2] for r in runs(chain)].count(edge_pcm.MAX_RUN) >= 2, "two full runs in one chain"


def test_run_ladder_in_stereo(enc_sim, synth, oracle):
    """the pair: the ladder in U, silence in V; two full runs in a chain on both sides"""
    c = encode_case(enc_sim, synth, oracle, "run_ladder", 16, 2, edge_pcm.LADDER_FL, 7 * edge_pcm.LADDER_FL)
    u, v = chains(c, 6)
    assert [r[2] for r in runs(u)].count(65535) == 2 and [r[2] for r in runs(v)].count(65535) == 2
    u, v = chains(c, 0)
    assert [r[2] for r in runs(u) if r[2] > 20] == [65534, 26, 27, 65463]


@pytest.mark.parametrize("depth,ch", [(16, 1), (16, 2), (20, 1), (24, 2)])
def test_bursts_put_escape_codes_right_behind_zero_runs(enc_sim, synth, oracle, lane_sim, helpers, depth, ch):
    c = encode_case(enc_sim, synth, oracle, "bursts", depth, ch, 4096, 4096)
    check_case(c, synth, oracle, lane_sim, helpers, variants=(-1,))
    assert not c.esc.any()
    allc = [e for chain in chains(c, 0) for e in chain]
    assert any(e[4] == 1 for e in escapes(allc)), "an escape code with zmode 1"
    if depth > 16 or ch == 2:  # chains wider than 16 bits: residuals above 0xffff clamp the mean (golomb.go:216-218)
        assert any(e[0] == "code" and e[3] > 0xffff and e[5] == 0xffff for e in allc)


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_antiphase_full_scale_has_escape_codes_in_a_compressed_element(enc_sim, synth, oracle, depth):
    c = encode_case(enc_sim, synth, oracle, "antiphase_full", depth, 2, 4096, 4096)
    assert not c.esc[0], "the sine packet must stay compressed"
    u, v = chains(c, 0)
    assert escapes(u + v), "escape codes of chanBits = %d bits" % (depth - 8 * edge_pcm.SHIFT[depth] + 1)


@pytest.mark.parametrize("depth,ch", [(16, 1), (24, 2)])
def test_clicks_at_the_packet_ends(enc_sim, synth, oracle, depth, ch):
    """click_first: the run behind it is cut off by the chain's end; click_last: the run in front of it ends one sample
    early and no run follows the last sample (i + 1 < n). The click is on channel 0 alone: in a pair it is the V chain's."""
    c = encode_case(enc_sim, synth, oracle, "click_first", depth, ch, 4096, 4096 + 9)
    for p, n in ((0, 4096), (1, 9)):
        chain = chains(c, p)[-1]
        assert chain[-1][0] == "zrun" and chain[-1][1] + chain[-1][2] == n
    c = encode_case(enc_sim, synth, oracle, "click_last", depth, ch, 4096, 4096 + 9)
    for p, n in ((0, 4096), (1, 9)):
        chain = chains(c, p)[-1]
        assert chain[-1][0] == "code" and chain[-1][1] == n - 1 and chain[-1][3] != 0
        if n > 9:
            assert chain[-2][0] == "zrun" and chain[-2][1] + chain[-2][2] == n - 1


@pytest.mark.parametrize("depth", [16, 24])
def test_dual_mono_has_a_silent_difference_chain(enc_sim, synth, oracle, depth):
    c = encode_case(enc_sim, synth, oracle, "dual_mono", depth, 2, 4096, 4096)
    u, v = chains(c, 0)
    assert v == [("code", 0, v[0][2], 0, 0, v[0][5]), ("zrun", 1, 4095, v[1][3])]
    assert any(e[3] for e in u)


@pytest.mark.parametrize("name", ["silence", "bursts", "antiphase_full", "nyquist_full", "dual_mono"])
def test_low_bits_of_20_bit_edge_samples_are_ignored(enc_sim, synth, oracle, name):
    cfg = oracle.make_config(4096, 20, 2)
    pcm = edge_pcm.make(name, synth, cfg, 4096 + 8)
    clean = bytearray(synth.pack_pcm(cfg, pcm))
    dirty = bytearray(clean)
    rng = np.random.default_rng(5)
    dirty[0::3] = (np.frombuffer(bytes(dirty[0::3]), np.uint8) | rng.integers(0, 16, len(dirty[0::3]), dtype=np.uint8)).tobytes()
    a = enc_sim.encode(cfg, bytes(clean), 4096 + 8)
    b = enc_sim.encode(cfg, bytes(dirty), 4096 + 8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
