"""The waveform augmentation pass on the CPU: csrc/alac_waveaug.h built with g++, contraction off (tests/host_sim/waveaug_sim.cpp),
workgroup for workgroup and work item for work item what the gfx950 kernels of k_waveaug.hip run, against tests/waveaug_ref.py's
numpy restatement bit for bit (output, draws and stats), against the properties the definition promises, and against float64
within a bound derived from the order of the sums.

* Philox4x32-10's two known answers through this header's include; the streams 2 and 3 against stream 0;
* the parameter sets of wa.PARAMS (nothing, gain only, noise only, dither only, everything with clamp) at T = 1, 255, 256, 257,
  tile - 1, tile, tile + 1 and 2 tile + 3, six rows with the lengths -2, 0, 1, T - 1, T and T + 9, banks of 0, 1 and 3 clips of the
  lengths 0, 1, 2, 257, tile + 1 and longer than T, every base offset of input, output and bank from a 16-byte boundary, rows and
  clips padded apart, in place and not, NaN / Inf behind n_r, behind m_k and in every gap, canaries around output, draws and stats;
* the dither variate's mean and variance over 65 536 samples; the properties; the energies against float64;
* what is refused (by the host build, by the library before any HIP call, by the Python entries and by the C++ mirror), the
  structs' sizes, the stand-alone program that the sanitizer run uses, the new names."""
import ctypes
import inspect
import math
import os
import subprocess

import numpy as np
import pytest

from tests import host_build
from tests import waveaug_ref as wa

F32 = np.float32
CANARY = F32(-12345.5)
SEED = 0x1234_5678_9ABC_DEF1
TILE = wa.TILE
LONG = 2 * TILE + 20  # a clip longer than every T here


@pytest.fixture(scope="module")
def sim():
    return wa.build_waveaug_sim()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the random words and the plan ------------------------------------------------------------------------------------
def test_philox_known_answers_through_this_header(sim):
    zero = [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    pi = [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    counter, key = [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0)
    assert wa.philox4x32_10([0, 0, 0, 0], (0, 0)) == zero and wa.sim_philox(sim, [0, 0, 0, 0], (0, 0)) == zero
    assert wa.philox4x32_10(counter, key) == pi and wa.sim_philox(sim, counter, key) == pi
    # the row's words: the two blocks at (id low, id high, 0 / 1, 2) under (seed low, seed high)
    ident, seed = 0x85A308D3_243F6A88, 0x299F31D0_A4093822
    want = wa.sim_philox(sim, [0x243F6A88, 0x85A308D3, 0, 2], key) + wa.sim_philox(sim, [0x243F6A88, 0x85A308D3, 1, 2], key)
    assert [int(v) for v in wa.row_words(seed, [ident])[0]] == want


def test_streams_share_no_block(sim):
    """SpecAugment's blocks (stream 0) of one (seed, id) against this pass's row blocks (stream 2) and dither blocks (stream 3):
    the counters differ in the fourth word, so no block is computed twice; the words bear that out"""
    ident = 77
    idx = np.arange(4096)
    blocks = {s: wa.philox_blocks(ident, 0, idx, s, SEED) for s in (0, wa.ROW_STREAM, wa.DITHER_STREAM)}
    as_rows = {s: {tuple(int(v) for v in b) for b in blk} for s, blk in blocks.items()}
    assert all(len(v) == 4096 for v in as_rows.values())
    assert not (as_rows[0] & as_rows[2]) and not (as_rows[0] & as_rows[3]) and not (as_rows[2] & as_rows[3])
    assert wa.ROW_STREAM == 2 and wa.DITHER_STREAM == 3


def test_plan_tables_are_the_doubles_rounded_once(sim):
    for cfg in [c for c, _ in wa.PARAMS.values()] + [(-16384, 0, 0, 16384, 0, 0), (0, 16384, -16384, 0, 65536, 1)]:
        rc, info, snr, gain = wa.sim_plan(sim, cfg)
        want_snr, want_gain = wa.tables(cfg)
        assert rc == 0 and info == dict(tile=TILE, draws=5, snr_entries=cfg[1] - cfg[0] + 1, gain_entries=cfg[3] - cfg[2] + 1,
                                        lds_bytes=4 * (TILE + 2 * 256 + 12))
        assert wa.same_bits(snr, want_snr) and wa.same_bits(gain, want_gain) and max(len(snr), len(gain)) <= 16385
    _, _, snr, gain = wa.sim_plan(sim, (0, 5120, 0, 5120, 0, 0))
    assert snr[0] == 1.0 and gain[0] == 1.0 and snr[5120] == F32(0.1) and gain[5120] == 10.0 and snr[2560] == F32(10 ** -0.5)


# ---- 2. bit for bit against the numpy restatement: offsets, gaps, poisoned padding, canaries ------------------------------
def run_over_buffers(sim, x, lengths, cfg, dither, bank, bank_lengths, k, in_place, row_base=11, want_draws=True, want_stats=True):
    """x and the bank laid out at odd offsets with gaps, poison behind n_r and m_k and in the gaps -> (y, draws, stats) of the host
    build, None for draws or stats that the pass is not given a block for; asserts that nothing but the output's elements, the
    rows' draws and the rows' stats changed"""
    rows, T = x.shape
    poison = (F32(np.nan), F32(np.inf), F32(-np.inf), F32(1e30))[k % 4]
    xin = x.copy()
    for r, n in enumerate(wa.clamp_lengths(lengths, rows, T)):
        xin[r, n:] = poison
    buf, off, view, rs = wa.lay_out(xin, (0, 5, 1, 7)[k % 4], k % 4, poison)
    nptr, nrs, N, Tn = None, 0, 0, 0
    if bank is not None and bank.size:
        N, Tn = bank.shape
        bz = bank.copy()
        for j, m in enumerate(wa.clamp_lengths(bank_lengths, N, Tn)):
            bz[j, m:] = poison
        nbuf, noff, _, nrs = wa.lay_out(bz, (3, 0, 2, 1)[k % 4], (k + 2) % 4, poison)
        nptr = nbuf.ctypes.data + 4 * noff
    if in_place:
        obuf, ooff, ors = buf, off, rs
    else:
        # every fifth case the output is aligned as the input is, row for row, which is where x is loaded 16 bytes at a time
        olead, ogap = (k % 4, (0, 5, 1, 7)[k % 4]) if k % 5 == 0 else ((k + 1) % 4, (2, 0, 6, 1)[k % 4])
        obuf, ooff, _, ors = wa.lay_out(np.zeros_like(x), ogap, olead, CANARY)
    before = buf.copy()
    draws, stats = np.full((rows + 2, 5), -77, np.int32), np.full((rows + 2, 4), CANARY, F32)
    rc = wa.host_run(sim, cfg, buf.ctypes.data + 4 * off, rs, rows, T, lengths, SEED, obuf.ctypes.data + 4 * ooff, ors, nptr, nrs, N, Tn,
                     bank_lengths, draws[1:] if want_draws else None, stats[1:] if want_stats else None, row_base=row_base, dither=dither,
                     pad_value=-3.5)
    assert rc == 0
    if in_place:
        assert np.array_equal(bits(wa.outside(buf, off, x.shape, rs)), bits(wa.outside(before, off, x.shape, rs))), "a gap was written"
    else:
        assert np.array_equal(bits(buf), bits(before)), "the input changed"
        rest = wa.outside(obuf, ooff, x.shape, ors)
        assert rest.size and (bits(rest) == bits(CANARY)).all(), "an element outside the output was written"
    assert (draws[0] == -77).all() and (draws[-1] == -77).all(), "exactly rows x 5 draws are written"
    assert (bits(stats[0]) == bits(CANARY)).all() and (bits(stats[-1]) == bits(CANARY)).all(), "exactly rows x 4 stats are written"
    y = np.lib.stride_tricks.as_strided(obuf[ooff:], x.shape, (4 * ors, 4)).copy()
    assert want_draws or (draws == -77).all(), "draws were written without a block for them"
    assert want_stats or (bits(stats) == bits(CANARY)).all(), "stats were written without a block for them"
    return y, draws[1:-1] if want_draws else None, stats[1:-1] if want_stats else None


def banks_of(rng, name):
    """(bank, its lengths) per case: no bank, one clip of each length, three clips"""
    one = [(wa.waves(rng, 1, LONG, 0.1), [m]) for m in (0, 1, 2, 257, TILE + 1, LONG)]
    three = (wa.waves(rng, 3, LONG, 0.1), [257, LONG + 5, TILE + 1])
    if name in ("noise", "all"):
        return [(None, None)] + one + [three, (three[0], None)]
    return [(None, None), three]


@pytest.mark.parametrize("name", list(wa.PARAMS))
def test_bits_against_the_reference(sim, name):
    cfg, dither = wa.PARAMS[name]
    assert wa.accepted(cfg, dither)
    rng = np.random.default_rng(2000 + len(name))
    banks = banks_of(rng, name)
    k = 0
    seen_applied = set()
    for T in wa.SAMPLES:
        lengths = wa.lengths_of(T)
        x = wa.waves(rng, len(lengths), T)
        for bank, bl in banks:
            want = wa.reference(x, lengths, cfg, SEED, bank, bl, row_base=11, dither=dither, pad_value=-3.5)
            got = run_over_buffers(sim, x, lengths, cfg, dither, bank, bl, k, in_place=k % 3 == 2)
            k += 1
            what = "T %d, bank %s, case %d" % (T, None if bank is None else bl, k)
            assert wa.same_bits(got[0], want[0]), "output: " + what
            assert np.array_equal(got[1], want[1]), "draws: " + what
            assert wa.same_bits(got[2], want[2]), "stats: " + what
            if bank is not None and bl is not None and len(bl) == 1:
                seen_applied |= {(bl[0], int(b != 0)) for b in want[2][3:, 3]}
        # no lengths: every sample is valid; ids in place of the row base; neither draws nor stats wanted
        ids = [2 ** 63 - 1, -1, 13]
        bank, bl = banks[-1]
        y, d, _ = wa.host_values(sim, x[:3], None, cfg, SEED, bank, bl, want_stats=False, ids=ids, dither=dither)
        want = wa.reference(x[:3], None, cfg, SEED, bank, bl, ids=ids, dither=dither)
        assert wa.same_bits(y, want[0]) and np.array_equal(d, want[1])
    if name in ("noise", "all"):  # every clip length but 0 was mixed in at least once, and a clip of no samples never
        assert {m for m, on in seen_applied if on} == {1, 2, 257, TILE + 1, LONG} and (0, 1) not in seen_applied


# ---- 3. the dither variate -------------------------------------------------------------------------------------------------
def test_dither_variate_moments(sim):
    """65 536 variates of one row: the mean within 5 / sqrt(N); the variance within 0.03 of 1 (the sample variance's standard
    deviation is sqrt(1.85 / N) = 0.0053 at Irwin-Hall(8)'s kurtosis, and 0.03 is more than five of them); |g| < 4.9. They are the
    host build's own: a dither-only pass with dither 1 over zeros gives fmaf(1, g, 1 * 0) = g"""
    n = 65536
    want = wa.dither_variates(SEED, 12345, np.arange(n))
    y, _, _ = wa.host_values(sim, np.zeros((1, n), F32), None, wa.PARAMS["dither"][0], SEED, ids=[12345], dither=1.0)
    assert wa.same_bits(y[0], want), "the host build's variates are the restatement's"
    g = y[0].astype(np.float64)
    print("mean %.6f, variance %.6f, largest |g| %.4f" % (g.mean(), g.var(), np.abs(g).max()))
    assert abs(g.mean()) <= 5.0 / math.sqrt(n) and abs(g.var() - 1.0) <= 0.03 and np.abs(g).max() < 4.9
    assert float(wa.KSCALE) == float.fromhex("0x1.3988e2p-16")
    assert wa.same_bits(want, wa.dither_variates(SEED, 12345, np.arange(n))), "deterministic for the seed"


# ---- 4. the properties ---------------------------------------------------------------------------------------------------
def test_nothing_to_do_is_one_times_x(sim):
    """gain (0, 0), no noise, no dither, no clamp: 1.0f * x, that is the sample's own bits (infinities, -0.0, subnormals and quiet
    NaN payloads included) with a signalling NaN made quiet; pad_value behind n_r"""
    rng = np.random.default_rng(3)
    T = 700
    raw = rng.integers(0, 2 ** 32, (5, T), dtype=np.uint64).astype(np.uint32)
    raw[0, :6] = np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0x80000000, 0x7F800001, 0x00000001], np.uint32)
    x = raw.view(F32)
    lengths = [T, 0, 33, 256, 699]
    y, draws, stats = wa.host_values(sim, x, lengths, wa.PARAMS["noop"][0], SEED, pad_value=9.0)
    signalling = ((raw & 0x7F800000) == 0x7F800000) & ((raw & 0x007FFFFF) != 0) & ((raw & 0x00400000) == 0)
    assert signalling[0, 4] and signalling.sum() > 1
    want = np.where(signalling, raw | 0x00400000, raw)
    for r, n in enumerate(lengths):
        assert np.array_equal(bits(y[r, :n]), want[r, :n]) and (y[r, n:] == 9.0).all()
    assert (draws[:, :3] == 0).all() and (stats[:, 2] == 1.0).all() and (stats[:, 3] == 0.0).all() and (stats[:, 1] == 0.0).all()


def test_a_row_alone_is_the_row_in_its_batch(sim):
    rng = np.random.default_rng(4)
    T = TILE + 300
    cfg, dither = wa.PARAMS["all"]
    x = wa.waves(rng, 6, T)
    bank, bl = wa.waves(rng, 3, 3000, 0.1), [3000, 257, 1500]
    lengths = [T, 900, 11, T - 5, 0, 4097]
    batch = wa.host_values(sim, x, lengths, cfg, SEED, bank, bl, row_base=1000, dither=dither)
    for k in range(6):
        alone = wa.host_values(sim, x[k:k + 1], lengths[k:k + 1], cfg, SEED, bank, bl, ids=[1000 + k], dither=dither)
        moved = wa.host_values(sim, x[k:k + 1], lengths[k:k + 1], cfg, SEED, bank, bl, row_base=1000 + k, dither=dither)
        for one in (alone, moved):
            assert wa.same_bits(one[0][0], batch[0][k]) and np.array_equal(one[1][0], batch[1][k])
            assert wa.same_bits(one[2][0], batch[2][k])
    other = wa.host_values(sim, x, lengths, cfg, SEED, bank, bl, row_base=2000, dither=dither)
    again = wa.host_values(sim, x, lengths, cfg, SEED + 1, bank, bl, row_base=1000, dither=dither)
    for k in (0, 1, 3, 5):
        assert not np.array_equal(other[1][k], batch[1][k]) and not wa.same_bits(other[0][k], batch[0][k]), "another row_base"
        assert not np.array_equal(again[1][k], batch[1][k]) and not wa.same_bits(again[0][k], batch[0][k]), "another seed"


def test_every_draw_in_its_range_and_every_choice_occurs(sim):
    """4096 identities at N = 3, probability 0.5: every draw in its range, every clip and both values of applied occur, the
    offsets spread over the clip, SNR and gain reach both ends of their ranges"""
    rows, T = 4096, 8
    cfg = (5 * 256, 20 * 256, -6 * 256, 3 * 256, 32768, 0)
    bl = [3000, 257, 1500]
    x = np.zeros((rows, T), F32)
    bank = np.zeros((3, 3000), F32)
    _, d, _ = wa.host_values(sim, x, None, cfg, SEED, bank, bl, row_base=7)
    _, want, _ = wa.reference(x[:64], None, cfg, SEED, bank, bl, row_base=7)
    assert np.array_equal(d[:64], want)
    applied, k, o, snr, gain = d.T
    assert set(applied.tolist()) == {0, 1} and abs(applied.mean() - 0.5) < 5 * 0.5 / math.sqrt(rows)
    assert set(k.tolist()) == {0, 1, 2} and (o >= 0).all() and (o < np.array(bl)[k]).all()
    for j, m in enumerate(bl):
        assert o[k == j].max() > 0.9 * m and o[k == j].min() < 0.1 * m
    assert (snr >= cfg[0]).all() and (snr <= cfg[1]).all() and snr.min() < cfg[0] + 40 and snr.max() > cfg[1] - 40
    assert (gain >= cfg[2]).all() and (gain <= cfg[3]).all() and gain.min() < cfg[2] + 40 and gain.max() > cfg[3] - 40
    # without a bank, or with clips of no samples: applied, k and o are 0, the SNR and the gain are drawn all the same
    _, d0, _ = wa.host_values(sim, x[:256], None, cfg, SEED, row_base=7)
    _, dz, _ = wa.host_values(sim, x[:256], None, cfg, SEED, bank, [0, -4, 0], row_base=7)
    for e in (d0, dz):
        assert not e[:, :3].any() and np.array_equal(e[:, 3:], d[:256, 3:])


def test_a_row_without_noise_never_reads_the_bank(sim):
    rng = np.random.default_rng(6)
    T = TILE + 9
    cfg = (5 * 256, 20 * 256, 0, 0, 32768, 0)
    x = wa.waves(rng, 64, T)
    bank = wa.waves(rng, 2, 5000, 0.1)
    y, d, st = wa.host_values(sim, x, None, cfg, SEED, bank, None)
    off = d[:, 0] == 0
    assert 10 < off.sum() < 54
    rows = np.flatnonzero(off)
    poisoned = np.full_like(bank, np.nan)
    y2, d2, st2 = wa.host_values(sim, x[rows], None, cfg, SEED, poisoned, None, ids=rows.tolist())
    assert wa.same_bits(y2, y[rows]) and np.array_equal(d2, d[rows]) and wa.same_bits(st2, st[rows])
    assert wa.same_bits(y2, x[rows]) and not st2[:, 1].any() and not st2[:, 3].any()
    # a silent row, or a silent clip, gets no noise either: b is 0 where Ex or En is
    silent = x.copy()
    silent[3] = 0
    _, ds, ss = wa.host_values(sim, silent, None, (0, 0, 0, 0, 65536, 0), SEED, bank, None)
    assert ds[3, 0] == 1 and ss[3, 0] == 0 and ss[3, 3] == 0 and ss[2, 3] > 0
    _, _, sz = wa.host_values(sim, x, None, (0, 0, 0, 0, 65536, 0), SEED, np.zeros_like(bank), None)
    assert not sz[:, 1].any() and not sz[:, 3].any()


def test_achieved_snr_is_the_drawn_one(sim):
    """10 log10(a^2 Ex / (b^2 En)) in float64 from the returned stats against draws[3] / 256: b carries the roundings of the
    division (halved by the root), the root, the table entry and two products, 4.5 u in all, that is 20 / ln 10 * 4.5 u dB"""
    rng = np.random.default_rng(8)
    T = 3 * TILE + 17
    cfg = (-10 * 256, 30 * 256, -6 * 256, 6 * 256, 65536, 0)
    x = wa.waves(rng, 32, T)
    lengths = rng.integers(1, T + 1, 32).tolist()
    bank = wa.waves(rng, 4, 6000, 0.05)
    y, d, st = wa.host_values(sim, x, lengths, cfg, SEED, bank, [6000, 100, 4097, 1])
    ex, en, a, b = (st[:, j].astype(np.float64) for j in range(4))
    assert (d[:, 0] == 1).all() and (b > 0).all()
    got = 10.0 * np.log10(a * a * ex / (b * b * en))
    err = np.abs(got - d[:, 3] / 256.0)
    lim = 20.0 / math.log(10.0) * 4.5 * wa.U * 1.01
    print("largest SNR error %.3g dB of %.3g dB allowed" % (err.max(), lim))
    assert (err <= lim).all()
    # and the mixture is what the stats say: y - a x is b z over the row's own samples
    r = 5
    n, z = lengths[r], bank[d[r, 1]][(d[r, 2] + np.arange(lengths[r])) % [6000, 100, 4097, 1][d[r, 1]]]
    resid = y[r, :n].astype(np.float64) - a[r] * x[r, :n] - b[r] * z
    assert np.abs(resid).max() <= 4 * wa.U * (np.abs(y[r, :n]).max() + 1e-30) and (y[r, n:] == 0).all()


# ---- 5. the energies against float64 -------------------------------------------------------------------------------------
def test_energies_against_float64(sim):
    """|Ex - sum v^2| <= gamma_L sum v^2 with L = the lane's chain (at most 16 fused steps) + the tree's 8 + the chunks, gamma_L =
    L u / (1 - L u), u = 2^-24: every sample passes through at most L roundings on its way into Ex. Prints the largest observed
    fraction of the bound"""
    rng = np.random.default_rng(9)
    worst = 0.0
    for T in (1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 9 * TILE + 100, 257 * TILE + 100):
        x = (rng.standard_normal((4, T)) * np.array([[1e-3], [1.0], [30.0], [0.3]])).astype(F32)
        x[3] = np.abs(x[3]) + 0.2  # no cancellation, nothing that hides an error
        bank = wa.waves(rng, 1, 777, 0.2)
        _, d, st = wa.host_values(sim, x, None, (0, 0, 0, 0, 65536, 0), SEED, bank, None)
        z = bank[0][(d[:, 2:3] + np.arange(T)[None]) % 777]
        for got, v in ((st[:, 0], x), (st[:, 1], z)):
            exact = (v.astype(np.float64) ** 2).sum(axis=1)
            L = wa.chain_length(T)
            lim = L * wa.U / (1 - L * wa.U) * exact
            frac = float((np.abs(got.astype(np.float64) - exact) / lim).max())
            assert frac <= 1.0, (T, frac)
            worst = max(worst, frac)
        assert wa.same_bits(st[:, 0], np.array([wa.energy(v) for v in x], F32))
    print("largest energy error / bound %.3f" % worst)


# ---- 6. what is refused --------------------------------------------------------------------------------------------------
def test_refusals_of_the_host_build(sim):
    T, rows = 40, 4
    x = np.zeros(rows * T + 64, F32)
    out = np.full(rows * T + 64, CANARY, F32)
    bank = np.full(3 * 50 + 8, 0.5, F32)
    draws = np.full(rows * 5 + 1, -77, np.int32)
    stats = np.full(rows * 4 + 1, CANARY, F32)
    ids, nl = np.zeros(5, np.int64), np.array([50, 20, 1, 0], np.int32)
    good = (5 * 256, 20 * 256, 0, 0, 65536, 0)

    def run(cfg=good, dither=0.0, rs=T, ors=T, rows=rows, T=T, inp=x.ctypes.data, outp=out.ctypes.data, lengths=None, idp=None,
            drp=draws.ctypes.data, stp=stats.ctypes.data, nzp=bank.ctypes.data, nrs=50, N=3, Tn=50, nlp=nl.ctypes.data):
        words = wa.config_words(cfg)
        return sim.waveaug_sim_run(words.ctypes.data, dither, 0.0, inp, rs, rows, T, lengths, nzp, nrs, N, Tn, nlp, SEED, 0, idp, outp,
                                   ors, drp, stp)

    assert run() == 0 and (draws[:20] != -77).all() and draws[20] == -77 and bits(stats[16]) == bits(CANARY)
    for bad in (dict(cfg=(-16385, 0, 0, 0, 0, 0)), dict(cfg=(0, 16385, 0, 0, 0, 0)), dict(cfg=(5, 4, 0, 0, 0, 0)),
                dict(cfg=(0, 0, 3, 2, 0, 0)), dict(cfg=(0, 0, -16385, 0, 0, 0)), dict(cfg=(0, 0, 0, 16385, 0, 0)),
                dict(cfg=(-1, 16384, 0, 0, 0, 0)), dict(cfg=(0, 0, -8193, 8192, 0, 0)), dict(cfg=(0, 0, 0, 0, 65537, 0)),
                dict(cfg=(0, 0, 0, 0, -1, 0)), dict(cfg=(0, 0, 0, 0, 0, 2)), dict(dither=-0.5), dict(dither=float("nan")),
                dict(dither=float("inf")),
                dict(inp=None), dict(outp=None), dict(inp=x.ctypes.data + 2), dict(outp=out.ctypes.data + 1),
                dict(lengths=x.ctypes.data + 2), dict(idp=ids.ctypes.data + 4), dict(drp=draws.ctypes.data + 2),
                dict(stp=stats.ctypes.data + 1), dict(nzp=bank.ctypes.data + 3), dict(nlp=nl.ctypes.data + 2),
                dict(rs=T - 1), dict(ors=T - 1), dict(nrs=49), dict(rs=2 ** 62), dict(nrs=2 ** 62),
                dict(T=2 ** 31, rs=2 ** 31, ors=2 ** 31), dict(Tn=2 ** 31, nrs=2 ** 31), dict(N=2 ** 31),
                # an output that overlaps the input: behind its start, ending inside it, the same base under another stride
                dict(outp=x.ctypes.data + 4 * 100), dict(inp=out.ctypes.data + 4 * 20, rows=1), dict(outp=x.ctypes.data, ors=T + 1),
                # a bank that overlaps the output
                dict(nzp=out.ctypes.data + 4 * 100), dict(nzp=out.ctypes.data, nrs=50), dict(outp=bank.ctypes.data + 4 * 100, rows=1)):
        out[...] = CANARY
        draws[...] = -77
        stats[...] = CANARY
        assert run(**bad) == -2, bad
        assert (out == CANARY).all() and not x.any() and (draws == -77).all() and (stats == CANARY).all() and (bank == 0.5).all()
    assert run(outp=x.ctypes.data) == 0, "in place"
    assert run(outp=x.ctypes.data, rs=T + 3, ors=T + 3, rows=3) == 0, "in place on a stride"
    assert run(outp=x.ctypes.data, rows=1, rs=T, ors=T + 9) == 0, "one row has no stride"
    assert run(inp=out.ctypes.data + 4 * rows * T, rows=1) == 0, "end to end is apart"
    assert run(nzp=None, nlp=None, N=0, Tn=0) == 0 and run(nzp=None) == 0 and run(N=0) == 0 and run(Tn=0) == 0, "no bank"
    assert run(nlp=None) == 0 and run(idp=ids.ctypes.data, drp=None, stp=None) == 0 and run(cfg=(0, 0, 0, 0, 0, 0), nzp=None, drp=None,
                                                                                             stp=None) == 0
    out[...] = CANARY
    assert run(rows=0) == 0 and run(T=0) == 0 and run(rows=0, inp=None, outp=None) == 0 and (out == CANARY).all()


def test_refusals_of_the_library_and_its_mirrors(pkg):
    """alacgpu_waveaug_create refuses before any HIP call (this runs without a GPU), and so do the Python class, the functional
    entries and the C++ mirror; a NULL handle is refused by every entry"""
    pkg.build()
    L = pkg.lib()
    h = ctypes.c_void_p()
    for cfg in ((-16385, 0, 0, 0, 0), (0, 16385, 0, 0, 0), (5, 4, 0, 0, 0), (0, 0, 3, 2, 0), (-1, 16384, 0, 0, 0), (0, 0, -8193, 8192, 0),
                (0, 0, 0, 0, 65537)):
        assert L.alacgpu_waveaug_create(0, ctypes.byref(pkg.WaveAugConfig(*cfg, 0.0, 0, 0.0)), ctypes.byref(h)) == -2 and not h, cfg
        assert b"no waveform augmentation plan" in L.alacgpu_last_error()
    for dither, clamp in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (0.0, 2)):
        assert L.alacgpu_waveaug_create(0, ctypes.byref(pkg.WaveAugConfig(0, 0, 0, 0, 0, dither, clamp, 0.0)), ctypes.byref(h)) == -2
    assert L.alacgpu_waveaug_create(0, None, ctypes.byref(h)) == -2
    assert L.alacgpu_waveaug_create(0, ctypes.byref(pkg.WaveAugConfig(0, 0, 0, 0, 0, 0.0, 0, 0.0)), None) == -2
    ms = ctypes.c_float()
    assert L.alacgpu_waveaug_device(None, 16, 40, 1, 40, None, None, 0, 0, 0, None, 1, 0, None, 4096, 40, None, None, 1) == -2
    assert L.alacgpu_waveaug_last_ms(None, ctypes.byref(ms)) == -2 and L.alacgpu_waveaug_synchronize(None) == -2
    assert L.alacgpu_waveaug_plan(None, ctypes.byref(pkg.WaveAugInfo()), None, 0, None, 0) == -2 and not L.alacgpu_waveaug_stream(None)
    L.alacgpu_waveaug_destroy(None)
    assert L.alacgpu_version() == b"alacgpu 0.7.0 gfx950"
    for kw in (dict(snr=(5, 70)), dict(snr=(-65, 0)), dict(snr=(20, 5)), dict(snr=(-40, 40)), dict(snr=5), dict(snr=("a", 1)),
               dict(gain=(3, -6)), dict(gain=(0, 64.5)), dict(noise_prob=1.5), dict(noise_prob=-0.1), dict(noise_prob="1"),
               dict(dither=-1e-5), dict(dither=float("nan")), dict(dither=float("inf")), dict(dither=True), dict(clamp=2),
               dict(clamp="yes")):
        with pytest.raises(ValueError):
            pkg.NewWaveAugment(**kw)
    import torch
    x = torch.zeros(2, 100)
    for call in (lambda: pkg.augment_waveform(x), lambda: pkg.augment_waveform(x, None), lambda: pkg.augment_waveform(x, seed=1, snr=(5, 70)),
                 lambda: pkg.augment_waveform(x, seed=1, dither=-1.0), lambda: pkg.augment_waveform(x.double(), seed=1),
                 lambda: pkg.augment_waveform(torch.zeros(()), seed=1), lambda: pkg.augment_waveform(np.zeros((2, 9)), seed=1),
                 lambda: pkg.load_features([], [], 1, wave_augment={"snr": (5, 20)}), lambda: pkg.load_features([], [], 1, wave_augment={}),
                 lambda: pkg.load_features([], [], 1, wave_augment=7),
                 lambda: pkg.load_features([], [], 1, wave_augment={"seed": 1, "pad_value": 1.0}),
                 lambda: pkg.load_features([], [], 1, wave_augment={"seed": 1, "out": x})):
        with pytest.raises(ValueError):
            call()
    S = wa.build_waveaug_shim(pkg)
    sizes = np.zeros(7, np.int64)
    S.waveaug_shim_sizes(sizes.ctypes.data)
    assert ctypes.sizeof(pkg.WaveAugConfig) == sizes[0] == 32 and ctypes.sizeof(pkg.WaveAugInfo) == sizes[1] == 72
    assert pkg.WaveAugConfig.dither.offset == sizes[2] == 20 and pkg.WaveAugInfo.scratch_bytes.offset == sizes[3] == 56
    assert (sizes[4], sizes[5], sizes[6]) == (20 * 256, -6 * 256, round(0.8 * 65536))
    assert S.waveaug_shim_create(ctypes.byref(pkg.WaveAugConfig(5, 4, 0, 0, 0, 0.0, 0, 0.0))) == -6
    assert b"no waveform augmentation plan" in S.waveaug_shim_last_error()
    assert S.waveaug_shim_create(ctypes.byref(pkg.WaveAugConfig(0, 0, 0, 0, 0, -1.0, 0, 0.0))) == -6


# ---- 7. the stand-alone program ------------------------------------------------------------------------------------------
def test_standalone_program_builds_and_runs(tmp_path):
    """tests/host_sim/waveaug_san_main.cpp, the program with its own main over waveaug_sim.cpp's functions that DESIGN.md §19 runs
    under the sanitizers on a CPU: here it is built plainly and run once, so that it stays in step with the header"""
    exe = str(tmp_path / "waveaug_san")
    host_build.compile("waveaug_san_main.cpp", exe, ["-O1", "-ffp-contract=off", "-fwrapv", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count("-> 0,") == 92 and "92 passes" in r.stdout and "nan" not in r.stdout.lower()
    assert ": 0 of the passes" not in r.stdout, "a combination of bank, stats and draws never ran"


# ---- 8. the names --------------------------------------------------------------------------------------------------------
def test_names_in_library_and_binding(pkg):
    for name in ("WaveAugConfig", "WaveAugInfo", "WaveAugment", "NewWaveAugment", "augment_waveform"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    for name in ("create", "destroy", "stream", "synchronize", "last_ms", "device", "plan"):
        assert "alacgpu_waveaug_" + name in pkg._EXPORTS
    assert issubclass(pkg.WaveAugment, pkg._RowPass)
    par = inspect.signature(pkg.NewWaveAugment).parameters
    assert list(par) == ["snr", "gain", "noise_prob", "dither", "clamp", "pad_value", "device"]
    assert [par[k].default for k in par] == [(5, 20), (0, 0), 1.0, 0.0, False, 0.0, 0]
    par = inspect.signature(pkg.WaveAugment.__call__).parameters
    assert list(par) == ["self", "clips", "lengths", "seed", "noise", "noise_lengths", "ids", "row_base", "out", "return_draws",
                         "return_stats"]
    par = inspect.signature(pkg.augment_waveform).parameters
    assert list(par)[:3] == ["clips", "lengths", "seed"] and par["lengths"].default is None
    assert not isinstance(par["seed"].default, (int, float)) and par["seed"].default is not None, "no usable default seed"
    assert par["dither"].default == 0.0 and par["clamp"].default is False and par["noise"].default is None
    par = inspect.signature(pkg.load_features).parameters
    assert list(par)[13:15] == ["augment", "wave_augment"] and par["wave_augment"].default is None
    mk = open(os.path.join(wa.ROOT, "saprobe-alac_amd", "csrc", "Makefile")).read()
    assert "k_waveaug" in mk.split("UNITS =")[1].split("\n")[0].split() and "build/k_waveaug.o: alac_waveaug.h" in mk
