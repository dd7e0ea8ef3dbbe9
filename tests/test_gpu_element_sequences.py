"""Packets whose element order is not the channel layout's own (tests/element_splice.py) through the C ABI on the GPU: the
scan's PktDesc (nslots, written[], route), one task per bitstream slot, rows indexed by slot, the interleave kernels' zero
fill and overwrite order, and the whole-packet decoder, each on packets built for it. Expected bytes: the oracle's, which
for every packet the model calls "ok" are the model's (checked here again, on the same packets).

Footprints as in test_gpu_output_layout.py (whose helpers this file uses): the device entry writes [0, frames * bytes per
frame) of a slot and nothing else, the host entries zero the rest of the frame buffer."""
import numpy as np
import pytest

from tests import element_splice as es
from tests import test_element_sequences as seqs
from tests import test_gpu_output_layout as lay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch(pkg):
    import importlib
    t = importlib.import_module("torch")
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


def want_kernels(cfg):
    """alacgpu_last_dispatch's irregular_kernels for a config (alacgpu.hip)"""
    bps = {16: 2, 20: 3, 24: 3, 32: 4}[cfg.bit_depth]
    if not (cfg.kb != 0 and cfg.pb <= 73):  # alac_regular.h: lean_config
        return "alac_scan (whole-packet decoder)"
    if cfg.num_channels > 2:
        il = "alac_interleave4" if (cfg.num_channels * bps) % 4 == 0 else "alac_interleave"
        return "alac_scan + alac_chan_predict + %s (+ alac_legacy)" % il
    return "alac_scan + alac_interleave (+ alac_legacy)"


def spliced(oracle, synth, depth, ch, fl, cookie, seed, budget=None, rounds=1):
    """-> (cfg, corpus): `rounds` corpora of one config, each with its own seed"""
    cfg = oracle.make_config(fl, depth, ch, **es.COOKIES[cookie])
    corpus = []
    for r in range(rounds):
        rng = np.random.default_rng(seqs.seed_of(depth, ch, fl, seed + r))
        corpus += es.CORPUS(synth, oracle, depth, ch, fl, rng, cookie=es.COOKIES[cookie], budget=budget,
                            override=dict(force_escape=1) if cookie == "kb0" else None)
    return cfg, corpus


def with_canonical(synth, cfg, corpus, n_each, seed):
    """The spliced packets shuffled among canonical synth packets (MUSIC and STRESS) of the same config, so that the sort
    sees both. -> (packets, index of every corpus packet in that list)"""
    packets = [p for _, p, _ in corpus]
    for prof in (synth.PROFILE_MUSIC, synth.PROFILE_STRESS):
        b = synth.gen_batch(cfg, n_each, profile=prof, base_seed=seed + prof, threads=8)
        packets += [b.packet(i) for i in range(b.n)]
    perm = np.random.default_rng(seed).permutation(len(packets))
    where = np.empty(len(packets), np.int64)
    where[perm] = np.arange(len(packets))
    return [packets[i] for i in perm], where[:len(corpus)]


def check_routes(lane_sim, helpers, cfg, packets, ref):
    """The batch holds every route the config has (lane_sim's classes for the same packets), before it is decoded."""
    blob, offs, sizes = helpers.pack_packets(packets)
    classes = lane_sim(cfg, blob, offs, sizes, variant=-1, want_classes=True)[3][ref[2] == 0]
    if not (cfg.kb != 0 and cfg.pb <= 73):
        return
    assert (classes == seqs.ROUTE_SPLIT).sum() >= 2 and (classes == seqs.ROUTE_LEGACY).sum() >= 2, np.unique(classes, return_counts=True)
    if cfg.num_channels <= 2 and cfg.frame_length > 32:
        assert (classes < 2048).sum() >= 2, "no packet for the wave pairs"


def check_against_model(synth, cfg, corpus, where, ref):
    sub = (ref[0][where], ref[1][where], ref[2][where])
    answers, mal = seqs.check_model(synth, cfg, corpus, sub)
    assert sum(1 for e in answers if e[0] == "ok") >= len(corpus) // 2
    return answers


IL4 = [(16, 4, 300), (16, 6, 1030), (16, 8, 4096), (24, 4, 1030), (20, 8, 300), (32, 3, 40), (32, 4, 300), (32, 5, 1030),
       (32, 6, 40), (32, 7, 300), (32, 8, 4096), (16, 8, 40), (24, 8, 1030)]          # every ALAC_IL_CASE pair (k_split.hip)
BYTES = [(16, 3, 1030), (16, 5, 300), (16, 7, 40), (24, 3, 300), (20, 5, 4096), (24, 6, 40), (20, 7, 1030)]  # alac_interleave
FEW = [(16, 1, 300), (16, 2, 4096), (24, 2, 300), (32, 2, 40), (20, 1, 1030), (16, 2, 40)]
OTHER = [(16, 2, 300, "pb255"), (24, 6, 40, "pb255"), (32, 8, 300, "pb255"), (16, 5, 1030, "pb255"), (16, 4, 40, "kb0"), (24, 2, 300, "kb0")]


@pytest.mark.parametrize("depth,ch,fl,cookie", [c + ("std",) for c in IL4 + BYTES + FEW] + OTHER)
def test_device_entry_decodes_spliced_sequences(torch, pkg, oracle, synth, lane_sim, helpers, depth, ch, fl, cookie):
    """alacgpu_decode_batch_device at an aligned and a misaligned layout, with d_sizes and without, on a patterned buffer:
    the oracle's status and frames, the model's PCM, zeros in the channels nobody wrote (that fill is the device's job),
    and the pattern behind the packet's frames, in the gap and around the slots."""
    cfg, corpus = spliced(oracle, synth, depth, ch, fl, cookie, 10, budget=None if fl <= 300 else 5)
    bpf = ch * oracle.bytes_per_sample(depth)
    fb = fl * bpf
    packets, where = with_canonical(synth, cfg, corpus, 96 if fl <= 300 else 32, depth + ch + fl)
    ref = lay.oracle_ref(oracle, helpers, cfg, packets)
    answers = check_against_model(synth, cfg, corpus, where, ref)
    check_routes(lane_sim, helpers, cfg, packets, ref)
    # a packet with fewer frames than one of its elements: what the whole-packet decoder must not write behind
    assert ch == 1 or seqs.count_shrinking(ch, fl, corpus) >= 2
    inp = lay.DeviceInputs(torch, helpers, packets)
    mis = (0, fb) if fb % 16 else (4, lay.r16(fb) + 16)
    with pkg.NewPacketDecoder(lay.pkg_cfg(pkg, cfg)) as dec:
        for off, stride in ((0, lay.r16(fb)), mis):
            for use_sizes in (True, False):
                lead, pat, got, fr, st = lay.device_decode(torch, dec, inp, off, stride, use_sizes)
                what = "%d-bit %d-ch %d %s offset %d stride %d sizes %s" % (depth, ch, fl, cookie, off, stride, use_sizes)
                lay.check_layout(what, ref, bpf, lead, stride, pat, got, fr, st, device=True)
                d = dec.last_dispatch()
                assert d["irregular_kernels"] == want_kernels(cfg), (what, d)
                if ch > 2 or not lay.aligned(off, stride) or cookie != "std":
                    assert d["irregular_slots"] == d["slots"] > 0 and d["narrow_slots"] == 0 and d["wide_slots"] == 0, (what, d)
                else:
                    assert d["irregular_slots"] > 0 and (fl <= 32 or d["narrow_slots"] > 0), (what, d)


@pytest.mark.parametrize("depth,ch,cookie", [(16, 2, "std"), (16, 6, "std"), (24, 8, "std"), (32, 5, "std"), (20, 3, "std"),
                                              (16, 8, "pb255"), (24, 1, "std")])
def test_host_entry_decodes_spliced_sequences(torch, pkg, oracle, synth, lane_sim, helpers, depth, ch, cookie):
    """alacgpu_decode_batch on dense blobs (no padding; lead 0 and 3 shift every packet's alignment): at least 2 000 spliced
    packets of FrameLength 300 among canonical ones — several waves per task key. The whole frame buffer of every packet
    is accounted for: PCM, then zeros (behind a partial frame, and a failing packet's whole slot)."""
    fl = 300
    cfg, corpus = spliced(oracle, synth, depth, ch, fl, cookie, 20, rounds={1: 40, 2: 16, 3: 12, 5: 8, 6: 7, 8: 5}[ch])
    assert len(corpus) >= 2000
    bpf = ch * oracle.bytes_per_sample(depth)
    packets, where = with_canonical(synth, cfg, corpus, 256, depth * ch)
    ref = lay.oracle_ref(oracle, helpers, cfg, packets)
    check_against_model(synth, cfg, corpus, where, ref)
    check_routes(lane_sim, helpers, cfg, packets, ref)
    want = np.where(np.arange(fl * bpf)[None, :] < (ref[1].astype(np.int64) * bpf)[:, None], ref[0], np.uint8(0))
    with pkg.NewPacketDecoder(lay.pkg_cfg(pkg, cfg)) as dec:
        for lead in (0, 3):
            blob, offs, _ = helpers.pack_dense(packets, lead=lead)
            offsets = np.concatenate([offs, [np.uint64(len(blob))]]).astype(np.uint64)
            out, fr, st = dec.decode_batch(blob, offsets)
            helpers.assert_same_decode(cfg, ref, (out, fr, st), bpf, "lead %d" % lead)
            bad = np.nonzero((out != want).any(axis=1))[0]
            assert len(bad) == 0, "lead %d: %d slots differ behind their frames, first %d (status %#x, %d frames)" % (
                lead, len(bad), bad[0], ref[2][bad[0]], ref[1][bad[0]])
            d = dec.last_dispatch()
            assert d["irregular_kernels"] == want_kernels(cfg), d
            if ch > 2 or cookie != "std":
                assert d["irregular_slots"] == d["slots"] > 0, d


def test_decode_packet_on_spliced_sequences(torch, pkg, oracle, synth, helpers):
    """(*PacketDecoder).DecodePacket, a batch of one: the model's bytes, or ErrDecode with the oracle's status word."""
    for depth, ch, fl, cookie in ((16, 4, 40, "std"), (24, 7, 300, "std"), (32, 2, 40, "std"), (20, 8, 40, "pb255")):
        cfg, corpus = spliced(oracle, synth, depth, ch, fl, cookie, 30)
        rng = np.random.default_rng(seqs.seed_of(depth, ch, fl, 31))
        picks = sorted(rng.choice(len(corpus), size=40, replace=False).tolist())
        picks += [i for i, c in enumerate(corpus) if c[0].startswith("8 ")][:2]
        n_bad = 0
        with pkg.NewPacketDecoder(lay.pkg_cfg(pkg, cfg)) as dec:
            for i in picks:
                name, p, seq = corpus[i]
                e = es.expected(ch, fl, seq)
                if e[0] == "ok":
                    assert dec.DecodePacket(p) == synth.pack_pcm(cfg, e[2]), "%d-bit %d-ch %s" % (depth, ch, name)
                else:
                    with pytest.raises(pkg.ErrDecode) as err:
                        dec.DecodePacket(p)
                    assert err.value.status == 6, name
                    n_bad += 1
        assert n_bad >= 2


@pytest.mark.parametrize("depth,fl", [(16, 300), (32, 40), (24, 300), (20, 1030)])
def test_two_decodes_back_to_back_do_not_share_descriptors(torch, pkg, oracle, synth, helpers, depth, fl):
    """Two device decodes on one handle without a synchronize in between, the first with eight bitstream slots per packet,
    the second with one element and then END: the workspace (rows, ChanDesc, PktDesc) is reused, and a stale nslots or
    written[] of the first batch would give the second one seven channels that are not zero."""
    ch = 8
    cfg, corpus = spliced(oracle, synth, depth, ch, fl, "std", 40, budget=None if fl <= 300 else 8, rounds=2)
    bpf = ch * oracle.bytes_per_sample(depth)
    fb = fl * bpf
    eight = [c for c in corpus if es.walk(ch, c[2])["slots"] == 8 and es.expected(ch, fl, c[2])[0] == "ok"]
    one = [c for c in corpus if len(es.walk(ch, c[2])["writes"]) == 1 and es.walk(ch, c[2])["slots"] <= 2 and es.expected(ch, fl, c[2])[0] == "ok"]
    n = min(len(eight), len(one) * 8)
    assert n >= 24 and len(one) >= 4
    first = eight[:n]
    second = [one[i % len(one)] for i in range(n)]
    stride = lay.r16(fb)
    dev = torch.device("cuda:0")
    runs = []
    with pkg.NewPacketDecoder(lay.pkg_cfg(pkg, cfg)) as dec:
        for batch in (first, second):
            packets = [p for _, p, _ in batch]
            inp = lay.DeviceInputs(torch, helpers, packets)
            pat = lay.pattern(lay.LEAD + n * stride + lay.TAIL)
            d_buf = torch.from_numpy(pat).to(dev)
            d_fr = torch.full((n,), -1, dtype=torch.int32, device=dev)
            d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
            runs.append((batch, packets, inp, pat, d_buf, d_fr, d_st))
        torch.cuda.synchronize()  # the handle's stream does not order against torch's
        for batch, packets, inp, pat, d_buf, d_fr, d_st in runs:
            dec.decode_batch_device(inp.blob.data_ptr(), inp.blob_bytes, inp.off.data_ptr(), inp.sz.data_ptr(), n,
                                    d_buf.data_ptr() + lay.LEAD, stride, d_fr.data_ptr(), d_st.data_ptr(), sync=False)
        dec.synchronize()
        for k, (batch, packets, inp, pat, d_buf, d_fr, d_st) in enumerate(runs):
            ref = lay.oracle_ref(oracle, helpers, cfg, packets)
            seqs.check_model(synth, cfg, batch, ref)
            lay.check_layout("batch %d" % k, ref, bpf, lay.LEAD, stride, pat, d_buf.cpu().numpy(),
                             d_fr.cpu().numpy().view(np.uint32), d_st.cpu().numpy(), device=True)
