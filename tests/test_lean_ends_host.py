"""The entropy role at a packet's ends on the host: alac_regular.h / alac_duo.h with ALAC_LEAN_ENDS and the other settings of
k_dec16l.hip (tests/host_sim/lean_ends_sim.cpp), one lane playing every role, against the oracle: status word, frame count,
PCM. With the switch, the chunks of a channel run the FAR form of the Golomb step (no packet-end term at all) while the
packet's end is more than a chunk of the longest steps away, and the END form from there on (the plain step plus the exact
overrun test of golomb.go:168) instead of golomb_slow within 329 bits of the end; a group that the lane's last sample closes
runs plain; and a ring block that reaches past the packet is fetched whole before it is masked.

* every prefix and every one-bit fault of the small packets of tests/single_fault.py, lean 16-bit configurations: the corpus
  that walks the overrun test across every byte of a packet's end;
* frame counts 1 .. 70 of 72 for eight orders: every residue of the sample count modulo the group of 8 steps;
* crafted endings (tests/lean_ends_cases.py): zero runs that start at the last samples or run to the end, escape codes as the
  last codes, bytes behind the END tag, V channels shorter than the reach — dense blobs at the four misalignments against an
  inaccessible page;
* a stand-alone program, built with the address and undefined-behaviour sanitizers, that decodes every prefix of a few packets
  at every misalignment out of heap blocks no longer than RingRd's contract allows."""
import ctypes
import subprocess

import numpy as np
import pytest

from tests import chunk_pipeline_cases as base
from tests import host_build
from tests import lean_ends_cases as cases
from tests import long_chunk_cases as long_cases
from tests import single_fault as sf

CONFIGS = [(16, 2, 48, "std"), (16, 1, 64, "std")]  # the lean 16-bit configurations of tests/single_fault.py


def build_lean_ends_sim():
    return host_build.shared("lean_ends_sim.cpp", "liblean_ends_sim.so", host_build.SIM)


@pytest.fixture(scope="module")
def lean_sim(oracle):
    """The host build, called like conftest's lane_sim (variant -1: the library's routing, the four-wave workgroups' roles);
    guard: the blob ends at an inaccessible page."""
    L = build_lean_ends_sim()
    vp = ctypes.c_void_p
    L.lane_sim_decode_batch.argtypes = [vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_size_t, vp, ctypes.c_size_t, vp, vp,
                                        ctypes.c_int, ctypes.c_int, vp, ctypes.c_int]

    def run(cfg, blob, offsets, sizes, guard=True):
        n = len(offsets)
        stride = (oracle.frame_bytes(cfg) + 15) // 16 * 16
        out = np.zeros((n, stride), np.uint8)
        classes = np.zeros(n, np.uint32)
        fr = np.zeros(n, np.uint32)
        st = np.zeros(n, np.int32)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        sizes = np.ascontiguousarray(sizes, np.uint32)
        rc = L.lane_sim_decode_batch(ctypes.byref(cfg), blob.ctypes.data, len(blob), offsets.ctypes.data, sizes.ctypes.data, n,
                                     out.ctypes.data, stride, fr.ctypes.data, st.ctypes.data, 1, -1, classes.ctypes.data,
                                     1 if guard else 0)
        assert rc == 0
        return (out, fr, st), classes

    return run


def bpf_of(oracle, cfg):
    return cfg.num_channels * oracle.bytes_per_sample(cfg.bit_depth)


def test_the_build_has_the_switch(lean_sim):
    """The library under test has all three parts and the 32-step chunks: a copy of long_chunk_sim would pass every comparison."""
    L = build_lean_ends_sim()
    L.lean_ends_sim_switch.restype = ctypes.c_uint32
    L.lean_ends_sim_steps.restype = ctypes.c_uint32
    assert L.lean_ends_sim_switch() == 7 and L.lean_ends_sim_steps() == 32


@pytest.mark.parametrize("depth,ch,fl,cookie", CONFIGS, ids=["-".join(map(str, c)) for c in CONFIGS])
def test_every_prefix_and_every_one_bit_fault(oracle, synth, helpers, lean_sim, depth, ch, fl, cookie):
    """All rows of the corpus, one dense blob per seed at a lead that rotates with the seed, against a guard page."""
    c = sf.corpus(synth, oracle, depth, ch, fl, cookie)
    bpf = bpf_of(oracle, c.cfg)
    lean = 0
    for k, s in enumerate(c.seeds):
        ref = tuple(r[s.first:s.end] for r in c.ref)
        blob, offs, sizes = helpers.pack_dense(c.packets[s.first:s.end], lead=k % 4)
        got, classes = lean_sim(c.cfg, blob, offs, sizes)
        lean += int((classes < 2048).sum())
        bad = sf.first_difference(ref, got, bpf, lambda i: "lead %d, %s" % (k % 4, s.what(c.cfg, s.first + i)))
        assert bad is None, bad
    assert lean > len(c.packets) // 3  # the lean path is what most of the corpus takes


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("order", long_cases.ORDERS)
def test_frame_counts_1_to_70(oracle, synth, helpers, lean_sim, order, ch):
    """Lanes that end in every step of a group of 8: the exact sample-end term sends a lane to golomb_slow only in a group
    that holds a step behind its last sample."""
    cfg = oracle.make_config(long_cases.FRAMES, 16, ch)
    packets = base.count_set(synth, cfg, long_cases.COUNTS, order)
    ref = oracle.decode_batch(cfg, *helpers.pack_packets(packets), threads=4)
    assert (ref[2] == 0).all() and list(ref[1]) == list(long_cases.COUNTS)
    assert {n % 8 for n in long_cases.COUNTS} == set(range(8))
    for lead in (0, 3):
        got, classes = lean_sim(cfg, *helpers.pack_dense(packets, lead=lead))
        assert (classes < 2048).all()
        helpers.assert_same_decode(cfg, ref, got, bpf_of(oracle, cfg), "order %d, %d ch, lead %d" % (order, ch, lead))


@pytest.mark.parametrize("ch", [2, 1])
def test_long_packets_run_far_from_their_end_first(oracle, synth, helpers, lean_sim, ch):
    """1 024 frames: dozens of chunks in the FAR form (the packets above are shorter than its reach and run the END form from
    their first chunk), then the END form; frame counts that leave tails of 31, 25 and 1 steps and a lane that ends early."""
    cfg = oracle.make_config(1024, 16, ch)
    for order in (4, 12, 0):
        packets = base.count_set(synth, cfg, (1024, 1023, 1017, 993, 700), order)
        # the FAR form's reach is 72 bits x the chunk's steps + 1 (32 steps in a pair's U phase, 16 where a writer role takes
        # half of each buffer: mono): at least three quarters of the shortest packet lie further from its end
        assert min(len(p) for p in packets) * 8 > 4 * 72 * (32 if ch == 2 else 16)
        ref = oracle.decode_batch(cfg, *helpers.pack_packets(packets), threads=4)
        assert (ref[2] == 0).all()
        got, classes = lean_sim(cfg, *helpers.pack_dense(packets, lead=order % 4))
        assert (classes < 2048).all()
        helpers.assert_same_decode(cfg, ref, got, bpf_of(oracle, cfg), "order %d, %d ch" % (order, ch))


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("fl", [96, 136])
def test_crafted_endings(oracle, synth, helpers, lean_sim, fl, ch):
    """Zero runs at and across the last samples, escape codes as the last codes, bytes behind the END tag, V channels shorter
    than the reach; frame counts fl - 7 .. fl. Valid packets all: the oracle gives back every frame."""
    cfg = oracle.make_config(fl, 16, ch)
    packets = cases.crafted(synth, cfg, range(fl - 7, fl + 1))
    ref = oracle.decode_batch(cfg, *helpers.pack_packets(packets), threads=4)
    assert (ref[2] == 0).all()
    for lead in (0, 1, 2, 3):
        got, classes = lean_sim(cfg, *helpers.pack_dense(packets, lead=lead))
        assert (classes < 2048).mean() > 0.9
        bad = sf.first_difference(ref, got, bpf_of(oracle, cfg), lambda i: "%d ch, fl %d, lead %d, packet %d" % (ch, fl, lead, i))
        assert bad is None, bad


def test_faults_at_the_end_of_crafted_packets(oracle, synth, helpers, lean_sim):
    """The prefixes that cut the last 64 bytes and the one-bit faults of the last 8 bytes of a sample of the crafted packets:
    the set tests/test_gpu_lean_ends.py mixes among valid packets."""
    cfg = oracle.make_config(96, 16, 2)
    pool = cases.crafted(synth, cfg, (89, 96))
    packets = cases.end_faults(pool[::9])
    ref = oracle.decode_batch(cfg, *helpers.pack_packets(packets), threads=4)
    assert (ref[2] != 0).any() and (ref[2] == 0).any()
    got, _ = lean_sim(cfg, *helpers.pack_dense(packets, lead=1))
    bad = sf.first_difference(ref, got, bpf_of(oracle, cfg), lambda i: "fault %d" % i)
    assert bad is None, bad


def test_standalone_program_under_the_sanitizers(tmp_path):
    """tests/host_sim/lean_ends_san_main.cpp with -fsanitize=address,undefined: every prefix of ten packets at the four byte
    misalignments, out of heap blocks that are dword-aligned at both ends and hold nothing behind the packet's last dword."""
    exe = str(tmp_path / "lean_ends_san")
    host_build.compile("lean_ends_san_main.cpp", exe,
                       ["-O1", "-g", "-fwrapv", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-x", "c++"],
                       libs=["-x", "c", "saprobe-alac_amd/synth/alac_synth.c", "-lm", "-lpthread"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 differ, switch 7" in r.stdout
