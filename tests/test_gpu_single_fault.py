"""Every one-bit fault and every truncation of small packets (tests/single_fault.py) through the C ABI on the GPU.

tests/test_single_fault.py runs the same corpus through the decode logic as the HOST compiler builds it. What only this
file sees: the GPU build's intrinsics once a flipped bit changes chanBits or denShift, the LDS rings and tail loads at a
packet's end, the hand-off between entropy, predictor and writer waves when one lane of 64 fails, and waves filled with
64 almost identical packets whose keys differ in one tap count.

Every input is a byte string the API accepts; statuses are compared with the oracle's, never forced. Every decode runs
on a guarded buffer (tests/test_gpu_output_layout.py): PCM where the oracle has frames, nothing behind a partial frame,
in the gap, in front of slot 0 or behind the last slot."""
import numpy as np
import pytest

from tests import single_fault as sf
from tests import test_gpu_output_layout as lay
from tests.test_single_fault import ids

pytestmark = pytest.mark.gpu

WHOLE_PACKET = "alac_scan (whole-packet decoder)"


@pytest.fixture(scope="module")
def torch(pkg):
    import importlib
    t = importlib.import_module("torch")
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


def device_inputs(torch, helpers, packets, lead=0):
    """lay.DeviceInputs with `lead` bytes of 0xFF in front of the blob (every packet's alignment moves)."""
    inp = lay.DeviceInputs.__new__(lay.DeviceInputs)
    blob, offs, sizes = helpers.pack_dense(packets, lead=lead)
    dev = torch.device("cuda:0")
    inp.n = len(packets)
    inp.blob_bytes = len(blob)
    inp.blob = torch.from_numpy(np.ascontiguousarray(blob)).to(dev)
    inp.off = torch.from_numpy(np.concatenate([offs, [np.uint64(len(blob))]]).astype(np.int64)).to(dev)
    inp.sz = torch.from_numpy(sizes.astype(np.int32)).to(dev)
    return inp


def decode_and_check(torch, dec, inp, ref, cfg, names, what, use_sizes=True):
    """One device decode at stride round16(frame bytes): the oracle's status, frames and PCM (reported by the packet's
    name), then the footprint."""
    bpf = cfg.num_channels * {16: 2, 20: 3, 24: 3, 32: 4}[cfg.bit_depth]
    fb = cfg.frame_length * bpf
    stride = lay.r16(fb)
    lead, pat, got, fr, st = lay.device_decode(torch, dec, inp, 0, stride, use_sizes)
    slots = got[lead:lead + inp.n * stride].reshape(inp.n, stride)
    bad = sf.first_difference(ref, (slots, fr, st), bpf, lambda i: "%s, %s" % (what, names(i)))
    assert bad is None, bad
    lay.check_layout(what, ref, bpf, lead, stride, pat, got, fr, st, device=True)
    return slots


def check_dispatch(key, cfg, d, what):
    """What ran, read back from the launch plan (alacgpu_last_dispatch)."""
    depth, ch, fl, cookie = key
    if cookie != "std":
        assert d["irregular_kernels"] == WHOLE_PACKET and d["narrow_slots"] == 0 and d["wide_slots"] == 0, (what, d)
    elif key in sf.LEAN:
        assert d["narrow_slots"] > 0 and d["narrow_kernel"] != "", (what, d)
        if depth in (24, 32):
            assert d["wide_slots"] > 0, (what, d)
    else:
        assert d["narrow_slots"] == 0 and d["wide_slots"] == 0 and d["irregular_slots"] == d["slots"] > 0, (what, d)
        assert d["irregular_kernels"] != WHOLE_PACKET, (what, d)


@pytest.mark.parametrize("depth,ch,fl,cookie", sf.CONFIGS, ids=ids(sf.CONFIGS))
def test_each_seeds_faults_as_one_batch(torch, pkg, oracle, synth, helpers, depth, ch, fl, cookie):
    """A seed's prefixes and flips in order, so that a wave holds 64 neighbours of one packet (a batch of this size puts a
    packet on two or four lanes): device entry, with d_sizes and with d_sizes = NULL."""
    c = sf.corpus(synth, oracle, depth, ch, fl, cookie)
    n_regular = 0
    with pkg.NewPacketDecoder(lay.pkg_cfg(pkg, c.cfg)) as dec:
        for s in c.seeds:
            ref = tuple(r[s.first:s.end] for r in c.ref)
            inp = lay.DeviceInputs(torch, helpers, c.packets[s.first:s.end])
            for use_sizes in (True, False):
                decode_and_check(torch, dec, inp, ref, c.cfg, lambda i: s.what(c.cfg, s.first + i), "sizes %s" % use_sizes, use_sizes)
                d = dec.last_dispatch()
                n_regular += d["narrow_slots"] + d["wide_slots"]
                if (depth, ch, fl, cookie) not in sf.LEAN:
                    check_dispatch((depth, ch, fl, cookie), c.cfg, d, s.name)
    assert ((depth, ch, fl, cookie) in sf.LEAN) == (n_regular > 0)


def mixed(c, salt):
    """All faulted packets of a configuration shuffled with a fixed seed, every fifth slot an intact seed packet.
    -> (packets, ref, names, [(slot, Seed)] of the intact ones)"""
    perm = np.random.default_rng([salt, len(c.packets)]).permutation(len(c.packets))
    n = len(perm) + len(perm) // 4
    is_seed = np.arange(n) % 5 == 4
    src = np.empty(n, np.int64)
    src[~is_seed] = perm
    src[is_seed] = np.arange(is_seed.sum()) % len(c.seeds)
    packets = [c.seeds[j].packet if sd else c.packets[j] for j, sd in zip(src.tolist(), is_seed.tolist())]
    ref = tuple(np.where(is_seed.reshape((-1,) + (1,) * (a.ndim - 1)), b[np.where(is_seed, src, 0)], a[np.where(is_seed, 0, src)])
                for a, b in zip(c.ref, c.seed_ref))
    intact = [(int(i), c.seeds[int(src[i])]) for i in np.nonzero(is_seed)[0]]

    def names(i):
        return "slot %d, intact %s" % (i, c.seeds[int(src[i])].name) if is_seed[i] else "slot %d, %s" % (i, sf.what(c, int(src[i])))

    return packets, ref, names, intact


def check_intact(c, cookie, slots, intact, what):
    """A damaged neighbour does not touch an intact packet: it comes out as its source PCM."""
    for i, s in intact:
        if cookie == "kb0" and s.row != "esc":
            continue  # not lossless (the synth's Golomb coder needs k >= 1); compared with the oracle like the rest
        assert slots[i, :len(s.pcm)].tobytes() == s.pcm, "%s: slot %d, intact %s is not its source PCM" % (what, i, s.name)


@pytest.mark.parametrize("depth,ch,fl,cookie", sf.CONFIGS, ids=ids(sf.CONFIGS))
def test_a_configurations_faults_as_one_batch(torch, pkg, oracle, synth, helpers, monkeypatch, depth, ch, fl, cookie):
    """Device entry at blob leads 0..3 in the default environment, with ALACGPU_PPW=64 and with ALACGPU_LANES_MIN=3 (read
    when the handle is made); the host entry; DecodePacket on the intact seeds and 200 faulted packets."""
    key = (depth, ch, fl, cookie)
    c = sf.corpus(synth, oracle, depth, ch, fl, cookie)
    cfg = c.cfg
    bpf = ch * oracle.bytes_per_sample(depth)
    packets, ref, names, intact = mixed(c, 5)
    assert len(packets) >= 20000 and len(intact) >= len(c.seeds)
    for env in ({}, {"ALACGPU_PPW": "64"}, {"ALACGPU_LANES_MIN": "3"}):
        for k in ("ALACGPU_PPW", "ALACGPU_LANES_MIN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with pkg.NewPacketDecoder(lay.pkg_cfg(pkg, cfg)) as dec:
            for lead in (0, 1, 2, 3) if not env else (0,):
                what = "%s, lead %d %s" % (sf.cfg_name(cfg), lead, env or "")
                inp = device_inputs(torch, helpers, packets, lead)
                slots = decode_and_check(torch, dec, inp, ref, cfg, names, what)
                check_intact(c, cookie, slots, intact, what)
                d = dec.last_dispatch()
                check_dispatch(key, cfg, d, what)
                if "ALACGPU_PPW" in env and key in sf.LEAN:
                    assert d["packets_per_slot"] == 64, d
            if env:
                continue
            # host entry: PCM, then zeros (behind a partial frame, and a failing packet's whole slot)
            blob, offsets = lay.host_inputs(helpers, packets)
            out, fr, st = dec.decode_batch(blob, offsets)
            bad = sf.first_difference(ref, (out, fr, st), bpf, lambda i: "host entry, %s" % names(i))
            assert bad is None, bad
            want = np.where(np.arange(out.shape[1])[None, :] < (ref[1].astype(np.int64) * bpf)[:, None], ref[0], np.uint8(0))
            rows = np.nonzero((out != want).any(axis=1))[0]
            assert len(rows) == 0, "host entry: %d slots differ behind their frames, first: %s" % (len(rows), names(int(rows[0])))
            check_dispatch(key, cfg, dec.last_dispatch(), "host entry")
            check_intact(c, cookie, out, intact, "host entry")
            # a batch of one
            rng = np.random.default_rng([7, depth, ch, fl])
            ones = [(s.name, s.packet, tuple(r[i] for r in c.seed_ref)) for i, s in enumerate(c.seeds)]
            ones += [(sf.what(c, i), c.packets[i], tuple(r[i] for r in c.ref)) for i in sorted(rng.choice(len(c.packets), 200, replace=False).tolist())]
            n_err = 0
            for name, p, (r_out, r_frames, r_st) in ones:
                if r_st == 0:
                    assert dec.DecodePacket(p) == r_out[:int(r_frames) * bpf].tobytes(), "DecodePacket, %s" % name
                else:
                    with pytest.raises(pkg.ErrDecode) as err:
                        dec.DecodePacket(p)
                    assert err.value.status == r_st, "DecodePacket, %s: status %#x, oracle %#x" % (name, err.value.status, r_st)
                    n_err += 1
            assert n_err >= 10


@pytest.mark.parametrize("depth,ch,fl", sf.COUNT_CONFIGS, ids=ids(sf.COUNT_CONFIGS))
def test_count_sweeps_on_both_sides_of_the_ten_byte_rule(torch, pkg, oracle, synth, helpers, depth, ch, fl):
    """Every frame count 1..FrameLength, and few-frame packets of full-scale noise whose entropy streams are 8-12 bytes
    (classify_regular's ten-byte rule: shorter ones must not take the lean route, whose fetches on the shift bytes would
    be pulled back into the shift values): each set as a batch of its own and all of them shuffled into one, at blob leads
    0..3, device entry with d_sizes and with NULL, and the host entry. All of these packets are valid: status 0 and the
    source PCM."""
    sets = sf.sweeps(synth, oracle, depth, ch)
    assert len(sets) == 1 + sum(1 for d, c, _ in sf.LOUD_SETS if (d, c) == (depth, ch))
    cfg = sets[0][1]
    bpf = ch * oracle.bytes_per_sample(depth)
    items, refs = [], []
    for name, c2, it, ref in sets:
        assert (c2.frame_length, c2.bit_depth, c2.num_channels) == (cfg.frame_length, cfg.bit_depth, cfg.num_channels)
        items += [("%s, %s" % (name, w), p, pcm) for w, p, pcm in it]
        refs.append(ref)
    perm = np.random.default_rng([depth, ch, 9]).permutation(len(items))
    everything = ("all sets shuffled", cfg, [items[i] for i in perm], tuple(np.concatenate([r[k] for r in refs])[perm] for k in range(3)))
    with pkg.NewPacketDecoder(lay.pkg_cfg(pkg, cfg)) as dec:
        for name, _, it, ref in sets + [everything]:
            packets = [p for _, p, _ in it]
            assert (ref[2] == 0).all()
            for lead in (0, 1, 2, 3):
                inp = device_inputs(torch, helpers, packets, lead)
                for use_sizes in (True, False):
                    what = "%s %s, lead %d sizes %s" % (sf.cfg_name(cfg), name, lead, use_sizes)
                    slots = decode_and_check(torch, dec, inp, ref, cfg, lambda i: it[i][0], what, use_sizes)
                    for i, (w, _, pcm) in enumerate(it):
                        assert slots[i, :len(pcm)].tobytes() == pcm, "%s: %s is not its source PCM" % (what, w)
                    d = dec.last_dispatch()
                    assert d["narrow_slots"] + d["wide_slots"] > 0, (what, d)
                    if depth != 16:
                        assert d["irregular_slots"] > 0, (what, d)
                blob, offs, _ = helpers.pack_dense(packets, lead=lead)
                out, fr, st = dec.decode_batch(blob, np.concatenate([offs, [np.uint64(len(blob))]]).astype(np.uint64))
                bad = sf.first_difference(ref, (out, fr, st), bpf, lambda i: "%s %s, host entry lead %d: %s" % (sf.cfg_name(cfg), name, lead, it[i][0]))
                assert bad is None, bad
