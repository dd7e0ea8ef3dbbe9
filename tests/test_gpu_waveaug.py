"""The waveform augmentation pass on the MI355X (k_waveaug.hip), held to the host build of the same header
(tests/host_sim/waveaug_sim.cpp, which tests/test_waveaug_host.py holds to numpy, to the definition's properties and to float64).
The draws are integer arithmetic, fmaf is correctly rounded on both sides and the sums have one order, so draws, Ex, En and a are
compared bit for bit. b = (sqrtf(Ex / En) * snr_amp) * a is compared within 4 * 2^-23 relative: a bare v_sqrt_f32 and a division
of 1 ulp would move the root by at most 1.5 * 2^-23 and each of the two products adds at most 2^-23; the test prints whether it is
equal, which it is expected to be. The output is compared bit for bit against the formula over the device's own stats.

* the CPU suite's grid: the parameter sets of wa.PARAMS at T = 1, 255, 256, 257, tile - 1, tile, tile + 1 and 2 tile + 3, six rows
  with the lengths -2, 0, 1, T - 1, T and T + 9, banks of 0, 1 and 3 clips of the lengths 0, 1, 2, 257, tile + 1 and longer than T, rows
  and clips at every base offset and padded apart, in place and not, the output aligned as the input is and not, NaN / Inf behind n_r, behind m_k and in the gaps, canaries around output, draws and stats;
* the tensor interface: in place, a channel of [B, channels, L], ids against row_base, augment_waveform and its cache, numpy in;
* load_features with wave_augment over three synthesised .m4a files against the pass applied by hand between load_clips and
  kaldi_fbank, and without the keyword against the chain as it was, byte for byte;
* the lifecycle of the handle, the C++ mirror;
* 2^22 + 4 099 rows of one chunk each: the second launch of all three kernels;
* two rows more than 2^32 elements apart, in and out, and in place.

No test provokes a fault: every refusal happens on the host, and every buffer has the size the entry asks for."""
import ctypes

import numpy as np
import pytest

from tests import waveaug_ref as wa

pytestmark = pytest.mark.gpu

F32 = np.float32
CANARY = F32(-12345.5)
SEED = 0x1234_5678_9ABC_DEF1
TILE = wa.TILE
LONG = 2 * TILE + 20
B_TOL = 4.0 * 2.0 ** -23


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture(scope="module")
def sim():
    return wa.build_waveaug_sim()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def new_waveaug(pkg, cfg, dither=0.0, pad_value=0.0):
    h = pkg.NewWaveAugment((cfg[0] / 256.0, cfg[1] / 256.0), (cfg[2] / 256.0, cfg[3] / 256.0), cfg[4] / 65536.0, dither, bool(cfg[5]),
                           pad_value)
    c = h.config
    assert (c.snr_lo_q8, c.snr_hi_q8, c.gain_lo_q8, c.gain_hi_q8, c.noise_prob_q16, c.clamp) == tuple(cfg)
    return h


def hold_to_host(got, want, x, lengths, cfg, bank, bl, what, nan_ok=False, host_output=False, **kw):
    """(y, draws, stats) of the device against the host build's: draws, Ex, En and a bit for bit, b within B_TOL, the output bit
    for bit against the formula over the device's own stats -> whether b is equal too. nan_ok: where the host build has a NaN
    the device has one, of whatever sign and payload (inputs that hold NaN or overflow). host_output: where all four stats are
    the host build's bit for bit, the formula over them is the host build's own output (the CPU suite holds it to that), so
    the output is compared with it and the formula is not worked out again (rows of millions of samples)"""
    y, draws, stats = got
    same = wa.same_or_nan if nan_ok else wa.same_bits
    assert np.array_equal(draws, want[1]), "draws: " + what
    assert same(stats[:, :3], want[2][:, :3]), "Ex, En, a: " + what
    b, wb = stats[:, 3].astype(np.float64), want[2][:, 3].astype(np.float64)
    assert ((b == 0) == (wb == 0)).all() and (np.abs(b - wb) <= B_TOL * np.abs(wb)).all(), "b: " + what
    equal = wa.same_bits(stats[:, 3], want[2][:, 3])
    if host_output and equal:
        assert same(y, want[0]), "output: " + what
    else:
        assert same(y, wa.formula(x, lengths, cfg, SEED, draws, stats, bank, bl, **kw)), "output: " + what
    return equal


def device_run(torch, h, x, lengths, bank, bank_lengths, k, in_place, row_base=0, ids=None, want_draws=True, want_stats=True):
    """The pass over x and the bank laid out at odd offsets with gaps and poison, through waveaug_device -> (y, draws, stats) as
    numpy, None for draws or stats where the pass gets no block for them (d_draws = 0, d_stats = 0); asserts that nothing but the
    output's elements and the rows' draws and stats changed"""
    rows, T = x.shape
    poison = (F32(np.nan), F32(np.inf), F32(-np.inf), F32(1e30))[k % 4]
    xin = x.copy()
    for r, n in enumerate(wa.clamp_lengths(lengths, rows, T)):
        xin[r, n:] = poison
    buf, off, _, rs = wa.lay_out(xin, (0, 5, 1, 7)[k % 4], k % 4, poison)
    d_in = to_dev(torch, buf[off - k % 4:])  # the device block starts at a 16-byte boundary, row 0 k % 4 elements behind it
    lead = k % 4
    d_bank, nrs, N, Tn, d_nl, nlead = None, 0, 0, 0, None, 0
    if bank is not None:
        N, Tn = bank.shape
        bz = bank.copy()
        for j, m in enumerate(wa.clamp_lengths(bank_lengths, N, Tn)):
            bz[j, m:] = poison
        nbuf, noff, _, nrs = wa.lay_out(bz, (3, 0, 2, 1)[k % 4], (k + 2) % 4, poison)
        nlead = (k + 2) % 4
        d_bank = to_dev(torch, nbuf[noff - nlead:])
        d_nl = None if bank_lengths is None else to_dev(torch, np.asarray(bank_lengths, np.int32))
    if in_place:
        d_out, olead, ors = d_in, lead, rs
    else:
        # every fifth case the output is aligned as the input is, row for row, which is where x is loaded 16 bytes at a time
        olead, ogap = (lead, (0, 5, 1, 7)[k % 4]) if k % 5 == 0 else ((k + 1) % 4, (2, 0, 6, 1)[k % 4])
        obuf, ooff, _, ors = wa.lay_out(np.zeros_like(x), ogap, olead, CANARY)
        d_out = to_dev(torch, obuf[ooff - olead:])
    before = d_in.clone()
    d_len = None if lengths is None else to_dev(torch, np.asarray(lengths, np.int32))
    d_ids = None if ids is None else to_dev(torch, np.asarray(ids, np.int64))
    d_draws = torch.full((rows + 2, 5), -77, dtype=torch.int32, device="cuda:0")
    d_stats = torch.full((rows + 2, 4), float(CANARY), dtype=torch.float32, device="cuda:0")
    for t in (d_in, d_out) + (() if d_bank is None else (d_bank,)):
        assert t.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    h.waveaug_device(d_in.data_ptr() + 4 * lead, rs, rows, T, 0 if d_len is None else d_len.data_ptr(), SEED, d_out.data_ptr() + 4 * olead,
                     ors, 0 if d_bank is None else d_bank.data_ptr() + 4 * nlead, nrs, N, Tn, 0 if d_nl is None else d_nl.data_ptr(),
                     row_base, 0 if d_ids is None else d_ids.data_ptr(), d_draws.data_ptr() + 4 * 5 if want_draws else 0,
                     d_stats.data_ptr() + 4 * 4 if want_stats else 0, sync=True)
    assert h.last_ms() > 0
    got, draws, stats = d_out.cpu().numpy(), d_draws.cpu().numpy(), d_stats.cpu().numpy()
    if in_place:
        assert np.array_equal(bits(wa.outside(got, olead, x.shape, ors)), bits(wa.outside(before.cpu().numpy(), olead, x.shape, ors)))
    else:
        assert torch.equal(d_in.view(torch.int32), before.view(torch.int32)), "the input changed"
        rest = wa.outside(got, olead, x.shape, ors)
        assert rest.size and (bits(rest) == bits(CANARY)).all(), "an element outside the output was written"
    assert (draws[0] == -77).all() and (draws[-1] == -77).all(), "a draw outside the rows' was written"
    assert (bits(stats[0]) == bits(CANARY)).all() and (bits(stats[-1]) == bits(CANARY)).all(), "a stat outside the rows' was written"
    assert want_draws or (draws == -77).all(), "draws were written without a block for them"
    assert want_stats or (bits(stats) == bits(CANARY)).all(), "stats were written without a block for them"
    y = np.lib.stride_tricks.as_strided(got[olead:], x.shape, (4 * ors, 4)).copy()
    return y, draws[1:-1] if want_draws else None, stats[1:-1] if want_stats else None


# ---- 1. the three kernels against the host build over the CPU suite's grid --------------------------------------------------
@pytest.mark.parametrize("name", list(wa.PARAMS))
def test_the_host_cases_on_the_device(torch, pkg, sim, name):
    cfg, dither = wa.PARAMS[name]
    rng = np.random.default_rng(3000 + len(name))
    one = [(wa.waves(rng, 1, LONG, 0.1), [m]) for m in (0, 1, 2, 257, TILE + 1, LONG)]
    three = (wa.waves(rng, 3, LONG, 0.1), [257, LONG + 5, TILE + 1])
    banks = [(None, None)] + one + [three, (three[0], None)] if name in ("noise", "all") else [(None, None), three]
    k, equal = 0, []
    with new_waveaug(pkg, cfg, dither, -3.5) as h:
        pl = h.plan()
        snr, gain = wa.tables(cfg)
        assert pl["tile"] == TILE and pl["draws"] == 5 and pl["lds_bytes"] == 4 * (TILE + 2 * 256 + 12)
        assert wa.same_bits(pl["snr_amp"], snr) and wa.same_bits(pl["gain_amp"], gain)
        for T in wa.SAMPLES:
            lengths = wa.lengths_of(T)
            x = wa.waves(rng, len(lengths), T)
            for bank, bl in banks:
                want = wa.host_values(sim, x, lengths, cfg, SEED, bank, bl, row_base=11, dither=dither, pad_value=-3.5)
                got = device_run(torch, h, x, lengths, bank, bl, k, in_place=k % 3 == 2, row_base=11)
                k += 1
                equal.append(hold_to_host(got, want, x, lengths, cfg, bank, bl, "T %d, bank %s, case %d" % (T, bl, k), row_base=11,
                                          dither=dither, pad_value=-3.5))
        # no lengths: every sample is valid; ids in place of the row base
        ids = [2 ** 63 - 1, -1, 13]
        bank, bl = banks[-1]
        want = wa.host_values(sim, x[:3], None, cfg, SEED, bank, bl, ids=ids, dither=dither, pad_value=-3.5)
        got = device_run(torch, h, x[:3], None, bank, bl, k, False, ids=ids)
        equal.append(hold_to_host(got, want, x[:3], None, cfg, bank, bl, "ids", ids=ids, dither=dither, pad_value=-3.5))
        assert pl["scratch_bytes"] >= 256 and h.plan()["scratch_address"]
    print("b equal to the host build's in %d of %d passes" % (sum(equal), len(equal)))


# ---- 2. the tensor interface ---------------------------------------------------------------------------------------------
def test_in_place_channels_ids_and_the_functional_entry(torch, pkg, sim):
    rng = np.random.default_rng(7)
    B, C, L = 4, 2, TILE + 151
    clips = wa.waves(rng, B * C, L).reshape(B, C, L)
    lengths = [L, 700, 0, 4097]
    bank, bl = wa.waves(rng, 3, 5000, 0.1), [5000, 257, 1500]
    cfg, dither = (5 * 256, 20 * 256, -6 * 256, 3 * 256, 52429, 1), 0.0
    d_clips, d_bank = to_dev(torch, clips), to_dev(torch, bank)
    with new_waveaug(pkg, cfg, dither, 0.0) as h:
        # one channel of [B, channels, L] on its own row stride; draws and stats come back per row
        view = d_clips[:, 1]
        assert view.stride() == (C * L, 1)
        want = wa.host_values(sim, clips[:, 1], lengths, cfg, SEED, bank, bl, row_base=40)
        before = d_clips.clone()
        y, draws, stats = h(view, lengths, SEED, noise=d_bank, noise_lengths=bl, row_base=40, return_draws=True, return_stats=True)
        assert tuple(y.shape) == (B, L) and y.is_contiguous() and torch.equal(d_clips, before)
        assert draws.dtype is torch.int32 and tuple(draws.shape) == (B, 5) and tuple(stats.shape) == (B, 4)
        hold_to_host((y.cpu().numpy(), draws.cpu().numpy(), stats.cpu().numpy()), want, clips[:, 1], lengths, cfg, bank, bl, "channel 1",
                     row_base=40)
        assert bool((y.abs() <= 1).all()) and bool((draws[:, 0] == 1).any())
        only_draws = h(view, lengths, SEED, noise=d_bank, noise_lengths=bl, row_base=40, return_draws=True)
        assert len(only_draws) == 2 and torch.equal(only_draws[0], y) and torch.equal(only_draws[1], draws)
        # in place on the view, and on a contiguous tensor with leading dimensions
        work = d_clips.clone()
        lane = work[:, 1]
        assert h(lane, lengths, SEED, noise=d_bank, noise_lengths=bl, row_base=40, out=lane) is lane
        # [B, channels, L] in place: row r of the flattened leading dimensions is row_base + r, draws and stats come back per
        # leading dimension; against the same data as [B * channels, L] and against the host build
        both, flat, every = work.clone(), work.reshape(B * C, L), [L, 700, 0, 4097, 1, L - 1, 4096, 333]
        y2, draws2, stats2 = h(both, every, SEED, noise=d_bank, noise_lengths=bl, row_base=40, out=both, return_draws=True,
                               return_stats=True)
        assert y2 is both and tuple(draws2.shape) == (B, C, 5) and tuple(stats2.shape) == (B, C, 4)
        y1, draws1, stats1 = h(flat, every, SEED, noise=d_bank, noise_lengths=bl, row_base=40, return_draws=True, return_stats=True)
        assert tuple(y1.shape) == (B * C, L) and tuple(draws1.shape) == (B * C, 5) and tuple(stats1.shape) == (B * C, 4)
        assert torch.equal(both.reshape(B * C, L).view(torch.int32), y1.view(torch.int32)) and torch.equal(draws2.reshape(B * C, 5), draws1)
        assert torch.equal(stats2.reshape(B * C, 4).view(torch.int32), stats1.view(torch.int32))
        rows = flat.cpu().numpy()
        hold_to_host((y1.cpu().numpy(), draws1.cpu().numpy(), stats1.cpu().numpy()), wa.host_values(sim, rows, every, cfg, SEED, bank, bl,
                                                                                                    row_base=40),
                     rows, every, cfg, bank, bl, "[B, channels, L]", row_base=40)
        assert len({tuple(d) for d in draws1.tolist()}) == B * C, "every row its own draws"
        chan = d_clips[:, 1].clone()
        assert h(chan, lengths, SEED, noise=d_bank, noise_lengths=bl, row_base=40, out=chan) is chan
        # ids against row_base: a row's augmentation is its identity's, wherever it stands in the batch
        order = [2, 0, 3, 1]
        shuffled = h(view[order], [lengths[j] for j in order], SEED, noise=d_bank, noise_lengths=bl, ids=[40 + j for j in order])
        assert torch.equal(shuffled, y[order])
        alone = h(view[3:4], lengths[3:4], SEED, noise=d_bank, noise_lengths=bl, ids=torch.tensor([43], device="cuda:0"))
        assert torch.equal(alone[0], y[3])
        assert not torch.equal(h(view, lengths, SEED, noise=d_bank, noise_lengths=bl, row_base=41)[0], y[0])
        assert not torch.equal(h(view, lengths, SEED + 1, noise=d_bank, noise_lengths=bl, row_base=40)[0], y[0])
        # what the class refuses
        for call in (lambda: h(view.double(), lengths, SEED), lambda: h(view, [1, 2, 3], SEED), lambda: h(view, lengths, -1),
                     lambda: h(view, lengths, SEED, ids=[1, 2, 3]), lambda: h(view, lengths, SEED, ids=[1.0, 2.0, 3.0, 4.0]),
                     lambda: h(view, lengths, SEED, noise=d_bank[0]), lambda: h(view, lengths, SEED, noise_lengths=bl),
                     lambda: h(view, lengths, SEED, noise=d_bank, noise_lengths=[1, 2]),
                     lambda: h(view, lengths, SEED, out=torch.zeros(4, 3, device="cuda:0")),
                     lambda: h(d_clips[..., ::2], None, SEED, out=d_clips[..., ::2]),
                     lambda: h(view, lengths, SEED, noise=view, out=view),
                     lambda: h.waveaug_device(view.data_ptr(), C * L, B, L, 0, SEED, view.data_ptr() + 4, C * L)):
            with pytest.raises(ValueError):
                call()
    assert torch.equal(work[:, 1], y) and torch.equal(work[:, 0], d_clips[:, 0]) and torch.equal(chan, y)
    # the functional entry against the handle, and the cache
    before = set(pkg._WAVEAUGS)
    kw = dict(noise=d_bank, noise_lengths=bl, snr=(5, 20), gain=(-6, 3), noise_prob=52429 / 65536.0, clamp=True)
    a, a_draws, a_stats = pkg.augment_waveform(view, lengths, SEED, row_base=40, return_draws=True, return_stats=True, **kw)
    assert torch.equal(a, y) and torch.equal(a_draws, draws) and torch.equal(a_stats, stats) and len(set(pkg._WAVEAUGS) - before) == 1
    pkg.augment_waveform(view, lengths, seed=SEED + 1, **kw)
    assert len(set(pkg._WAVEAUGS) - before) == 1
    # numpy arrays are uploaded; with nothing to do the pass only masks the padding
    plain = pkg.augment_waveform(clips[:, 0], lengths, seed=1, noise=bank, noise_prob=0.0, pad_value=-2.0)
    assert plain.is_cuda and torch.equal(plain[0], d_clips[0, 0]) and torch.equal(plain[1, :700], d_clips[1, 0, :700])
    assert float(plain[2].max()) == -2.0 and float(plain[1, 700:].min()) == -2.0
    empty = pkg.augment_waveform(torch.zeros(0, 16), seed=1, return_draws=True)
    assert tuple(empty[0].shape) == (0, 16) and tuple(empty[1].shape) == (0, 5)


# ---- 3. raggedness, end to end -------------------------------------------------------------------------------------------
def test_load_features_with_wave_augment(torch, pkg, tmp_path):
    rng = np.random.default_rng(5)
    paths = []
    for k, (rate, T) in enumerate(((48000, 40000), (44100, 44100), (44100, 13230))):
        t = np.arange(T) / rate
        wave = 0.3 * np.sin(2 * np.pi * (200 + 170 * k) * t) + 0.05 * rng.standard_normal(T)
        path = str(tmp_path / ("f%d.m4a" % k))
        assert pkg.save(path, to_dev(torch, wave[None].astype(F32)), rate) == 0
        paths.append(path)
    offsets, L = [0, 1000, 0], 8000
    kw = dict(num_mel_bins=23, low_freq=20.0)
    base, flen, rate = pkg.load_features(paths, offsets, L, sample_rate=16000, **kw)
    # without the keyword, and with None, the chain as it was: byte for byte normalize_features of the same steps
    clips, lengths, _ = pkg.load_clips(paths, offsets, L, sample_rate=16000)
    assert 0 < int(lengths[2]) < L == int(lengths[0])
    counts = pkg.kaldi_frame_counts(lengths, 400, 160)
    chain = pkg.normalize_features(pkg.kaldi_fbank(clips[:, 0], sample_frequency=16000, **kw), counts, stat="mean")
    none, nlen, _ = pkg.load_features(paths, offsets, L, sample_rate=16000, wave_augment=None, **kw)
    assert torch.equal(none.view(torch.int32), chain.view(torch.int32)) and torch.equal(base.view(torch.int32), chain.view(torch.int32))
    assert torch.equal(nlen.cpu(), counts.cpu()) and torch.equal(flen.cpu(), counts.cpu())
    bank = to_dev(torch, wa.waves(rng, 2, 6000, 0.05))
    aug = dict(seed=77, ids=[900, 5, 31], noise=bank, noise_lengths=[6000, 999], snr=(5, 20), gain=(-6, 3), dither=1e-4, clamp=True)
    feats, alen, _ = pkg.load_features(paths, offsets, L, sample_rate=16000, wave_augment=aug, **kw)
    wave, draws = pkg.augment_waveform(clips[:, 0], lengths, return_draws=True, **aug)
    want = pkg.normalize_features(pkg.kaldi_fbank(wave, sample_frequency=16000, **kw), counts, stat="mean")
    assert torch.equal(feats.view(torch.int32), want.view(torch.int32)) and torch.equal(alen.cpu(), counts.cpu())
    assert not torch.equal(feats, base) and bool((draws[:, 0] == 1).all())
    for j, n in enumerate(lengths.cpu().tolist()):  # +0.0 behind the row's own samples: the feature pass relies on it
        assert not bool(wave[j, n:].view(torch.int32).any())
    # beside SpecAugment, on one (seed, ids)
    both, _, _ = pkg.load_features(paths, offsets, L, sample_rate=16000, wave_augment=aug, augment=dict(seed=77, ids=[900, 5, 31], freq_width=5,
                                                                                                      time_width=10), **kw)
    masked = pkg.spec_augment(want, counts, seed=77, ids=[900, 5, 31], freq_width=5, time_width=10)
    assert torch.equal(both.view(torch.int32), masked.view(torch.int32)) and not torch.equal(masked, want)


# ---- 4. the handle -------------------------------------------------------------------------------------------------------
def test_lifecycle_and_the_cpp_mirror(torch, pkg, sim):
    rng = np.random.default_rng(9)
    T = 700
    x = wa.waves(rng, 3, T)
    bank = wa.waves(rng, 2, 900, 0.1)
    d_x, d_bank = to_dev(torch, x), to_dev(torch, bank)
    cfg = (5 * 256, 20 * 256, -3 * 256, 3 * 256, 65536, 0)
    h = new_waveaug(pkg, cfg, 0.0, -1.0)
    with pytest.raises(ValueError):
        h.last_ms()  # no pass yet on this handle
    h.waveaug_device(0, 1, 0, T, 0, 1, 0, 1)
    h.waveaug_device(0, 1, 3, 0, 0, 1, 0, 1)
    with pytest.raises(ValueError):
        h.last_ms()  # nothing was launched
    d_y = torch.zeros(3, T, device="cuda:0")
    for kw in (dict(rs=T - 1), dict(ors=T - 1), dict(inp=0), dict(outp=0), dict(inp=d_x.data_ptr() + 2), dict(outp=d_x.data_ptr() + 4),
               dict(outp=d_x.data_ptr() + 4 * (3 * T - 1)), dict(nzp=d_y.data_ptr() + 4 * T), dict(nrs=899), dict(T=2 ** 31, rs=2 ** 31,
                                                                                                                     ors=2 ** 31)):
        a = dict(inp=d_x.data_ptr(), rs=T, T=T, outp=d_y.data_ptr(), ors=T, nzp=d_bank.data_ptr(), nrs=900)
        a.update(kw)
        with pytest.raises(ValueError):
            h.waveaug_device(a["inp"], a["rs"], 3, a["T"], 0, 1, a["outp"], a["ors"], a["nzp"], a["nrs"], 2, 900)
    with pytest.raises(ValueError):
        h.last_ms()
    assert not bool(d_y.any()) and h.out_frames(T) == T
    pl = h.plan()
    assert [pl[k] for k in ("snr_lo_q8", "snr_hi_q8", "gain_lo_q8", "gain_hi_q8", "noise_prob_q16", "clamp", "tile", "draws")] == [
        1280, 5120, -768, 768, 65536, 0, TILE, 5] and pl["pad_value"] == -1.0 and pl["dither"] == 0.0
    first = pl["scratch_address"]
    y, draws, stats = h(d_x, [T, 0, 333], SEED, noise=d_bank, return_draws=True, return_stats=True)
    want = wa.host_values(sim, x, [T, 0, 333], cfg, SEED, bank, None, pad_value=-1.0)
    hold_to_host((y.cpu().numpy(), draws.cpu().numpy(), stats.cpu().numpy()), want, x, [T, 0, 333], cfg, bank, None, "handle",
                 pad_value=-1.0)
    assert h.last_ms() > 0 and h.plan()["scratch_address"] == first, "a small pass fits the first block"
    big = torch.zeros(64, 3 * TILE, device="cuda:0")
    h(big, None, SEED, noise=d_bank)
    assert h.plan()["scratch_bytes"] >= 4 * (64 * 3 * 2 + 64 * 4), "the block grew for the partials and the stats"
    h.synchronize()
    h.close()
    h.close()
    assert h.out_frames(T) == 0
    for call in (h.synchronize, h.last_ms, h.plan, lambda: h(d_x)):
        with pytest.raises(ValueError):
            call()
    # host/wave_augment.hpp through the ctypes shim
    S = wa.build_waveaug_shim(pkg)
    c = pkg.WaveAugConfig(*cfg[:5], 0.0, cfg[5], -1.0)
    ids = [7, -9, 2 ** 40]
    want = wa.host_values(sim, x, [T, 0, 333], cfg, SEED, bank, [900, 1], ids=ids, pad_value=-1.0)
    d_len, d_ids = to_dev(torch, np.asarray([T, 0, 333], np.int32)), to_dev(torch, np.asarray(ids, np.int64))
    d_nl = to_dev(torch, np.asarray([900, 1], np.int32))
    d_draws = torch.zeros((3, 5), dtype=torch.int32, device="cuda:0")
    d_stats = torch.zeros((3, 4), dtype=torch.float32, device="cuda:0")
    info, extra = pkg.WaveAugInfo(), (ctypes.c_float * 3)()
    torch.cuda.synchronize()

    def run(out_rs):
        return S.waveaug_shim_run(ctypes.byref(c), d_x.data_ptr(), T, 3, T, d_len.data_ptr(), d_bank.data_ptr(), 900, 2, 900,
                                  d_nl.data_ptr(), SEED, 0, d_ids.data_ptr(), d_y.data_ptr(), out_rs, d_draws.data_ptr(),
                                  d_stats.data_ptr(), ctypes.byref(info), extra)

    assert run(T) == 0, S.waveaug_shim_last_error()
    snr, gain = wa.tables(cfg)
    assert extra[2] > 0 and (info.tile, info.draws, info.snr_entries, info.gain_entries) == (TILE, 5, len(snr), len(gain))
    assert (extra[0], extra[1], info.pad_value, info.gain_lo_q8) == (snr[0], gain[0], -1.0, -768)
    hold_to_host((d_y.cpu().numpy(), d_draws.cpu().numpy(), d_stats.cpu().numpy()), want, x, [T, 0, 333], cfg, bank, [900, 1], "mirror",
                 ids=ids, pad_value=-1.0)
    assert run(T - 1) == -6 and b"stride" in S.waveaug_shim_last_error()


# ---- 5. the second launch ------------------------------------------------------------------------------------------------
def test_second_launch_of_the_three_kernels(torch, pkg, sim):
    """N = 2^22 + 4 099 rows of 6 samples, one chunk each, so each of alac_waveaug_partials, alac_waveaug_finish and
    alac_waveaug_apply_dither goes in two launches, the second with first_tile = 2^22 and 4 099 workgroups. Row r has the content,
    the length and the identity of class r % 7 (2^22 = 2 mod 7), so output, draws and stats cycle with period 7 and are held to
    the host build's 7 rows on the device, with sentinels around each: a launch that ignored first_tile would leave the rows
    from 2^22 on unwritten, one that read its inputs from the batch's start would break the cycle"""
    SLICE, LEAD, TAIL, FILL = 1 << 22, 9, 8, -77.0
    N, T = SLICE + 4099, 6
    cfg, dither = (5 * 256, 20 * 256, -6 * 256, 3 * 256, 52429, 0), 0.01
    rng = np.random.default_rng(72)
    x7, lengths7, ids7 = wa.waves(rng, 7, T), [-3, 0, 1, 2, 5, 6, 13], [1000 + k for k in range(7)]
    bank, bl = wa.waves(rng, 3, 40, 0.1), [40, 1, 7]
    want7 = wa.host_values(sim, x7, lengths7, cfg, SEED, bank, bl, ids=ids7, dither=dither, pad_value=-2.0)
    assert len({tuple(d) for d in want7[1].tolist()}) == 7 and 0 < want7[1][:, 0].sum() < 7 and (want7[2][:, 3] != 0).sum() >= 2
    x = to_dev(torch, x7).repeat(-(-N // 7), 1)[:N].contiguous()
    d_len = to_dev(torch, np.asarray(lengths7, np.int32)).repeat(-(-N // 7))[:N].contiguous()
    d_ids = 1000 + torch.arange(N, dtype=torch.int64, device="cuda:0") % 7
    d_bank, d_nl = to_dev(torch, bank), to_dev(torch, np.asarray(bl, np.int32))
    out = torch.full((LEAD + N * T + TAIL,), FILL, dtype=torch.float32, device="cuda:0")
    draws = torch.full((LEAD + N * 5 + TAIL,), -77, dtype=torch.int32, device="cuda:0")
    stats = torch.full((LEAD + N * 4 + TAIL,), FILL, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    with new_waveaug(pkg, cfg, dither, -2.0) as h:
        h.waveaug_device(x.data_ptr(), T, N, T, d_len.data_ptr(), SEED, out.data_ptr() + 4 * LEAD, T, d_bank.data_ptr(), 40, 3, 40,
                         d_nl.data_ptr(), 0, d_ids.data_ptr(), draws.data_ptr() + 4 * LEAD, stats.data_ptr() + 4 * LEAD, sync=True)
    # the device's own 7 classes against the host build, then the cycle against the device's first period
    first = (out[LEAD:LEAD + 7 * T].cpu().numpy().reshape(7, T), draws[LEAD:LEAD + 35].cpu().numpy().reshape(7, 5),
             stats[LEAD:LEAD + 28].cpu().numpy().reshape(7, 4))
    hold_to_host(first, want7, x7, lengths7, cfg, bank, bl, "the first period", ids=ids7, dither=dither, pad_value=-2.0)
    for name, buf, per, fill in (("output", out, T, FILL), ("draws", draws, 5, -77), ("stats", stats, 4, FILL)):
        body = buf[LEAD:LEAD + N * per].view(torch.int32)
        row = body[:7 * per].clone()
        full = N // 7
        bad = torch.nonzero((body[:full * 7 * per].view(full, 7 * per) != row).any(dim=1))[:4].flatten().tolist()
        assert not bad, "%s: periods %s differ from the first" % (name, bad)
        assert torch.equal(body[full * 7 * per:], row[:(N - full * 7) * per]), "%s: the last, short period differs" % name
        assert bool((buf[:LEAD] == fill).all()) and bool((buf[LEAD + N * per:] == fill).all()), "%s: a sentinel is gone" % name


# ---- 6. far rows ---------------------------------------------------------------------------------------------------------
def test_rows_more_than_4_gi_elements_apart(torch, pkg, sim):
    """Two rows whose row stride is 2^32 + 12 345 elements, in the input and in the output, each in one allocation of 16 GiB that
    is touched only around the rows: a row offset narrowed to 32 bits would read and write row 1 at element 12 345, which holds
    canaries. Then in place on the input"""
    cfg, dither = wa.PARAMS["all"]
    rs, guard, T = (1 << 32) + 12345, 4096, TILE + 1
    try:
        big_in = torch.empty(rs + T + guard, dtype=torch.float32, device="cuda:0")
        big_out = torch.empty(rs + T + guard, dtype=torch.float32, device="cuda:0")
    except RuntimeError as e:
        pytest.skip("no two allocations of %.1f GiB: %s" % ((rs + T + guard) * 4 / 2.0 ** 30, str(e).splitlines()[0]))
    rng = np.random.default_rng(4)
    x = wa.waves(rng, 2, T)
    bank, bl = wa.waves(rng, 2, 3000, 0.1), [3000, 257]
    d_bank = to_dev(torch, bank)
    lengths = [T - 3, T]
    for big in (big_in, big_out):
        big[:12345 + T + guard] = float(CANARY)
        big[rs - guard:rs + T + guard] = float(CANARY)
    big_in[:T] = to_dev(torch, x[0])
    big_in[rs:rs + T] = to_dev(torch, x[1])
    rows_in = torch.as_strided(big_in, (2, T), (rs, 1))
    rows_out = torch.as_strided(big_out, (2, T), (rs, 1))

    def rows_of(big):
        return np.stack([big[:T].cpu().numpy(), big[rs:rs + T].cpu().numpy()])

    def guards_intact(big):
        return all(bool((big[a:b] == float(CANARY)).all()) for a, b in ((T, 12345 + T + guard), (rs - guard, rs), (rs + T, rs + T + guard)))

    want = wa.host_values(sim, x, lengths, cfg, SEED, bank, bl, row_base=5, dither=dither, pad_value=-2.0)
    assert (want[2][:, 3] != 0).all(), "both rows get noise"
    with new_waveaug(pkg, cfg, dither, -2.0) as h:
        out, draws, stats = h(rows_in, lengths, SEED, noise=d_bank, noise_lengths=bl, row_base=5, out=rows_out, return_draws=True,
                              return_stats=True)
        assert out is rows_out
        hold_to_host((rows_of(big_out), draws.cpu().numpy(), stats.cpu().numpy()), want, x, lengths, cfg, bank, bl, "far rows",
                     row_base=5, dither=dither, pad_value=-2.0)
        assert guards_intact(big_out), "an element outside the two rows was written"
        assert wa.same_bits(rows_of(big_in), x) and guards_intact(big_in), "the input changed"
        out, draws, stats = h(rows_in, lengths, SEED, noise=d_bank, noise_lengths=bl, row_base=5, out=rows_in, return_draws=True,
                              return_stats=True)
    assert out is rows_in
    hold_to_host((rows_of(big_in), draws.cpu().numpy(), stats.cpu().numpy()), want, x, lengths, cfg, bank, bl, "far rows in place",
                 row_base=5, dither=dither, pad_value=-2.0)
    assert guards_intact(big_in), "an element outside the two rows was written"
    del big_in, big_out, rows_in, rows_out, out
    torch.cuda.empty_cache()
