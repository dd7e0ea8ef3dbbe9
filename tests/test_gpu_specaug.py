"""The SpecAugment pass on the MI355X (k_specaug.hip), held to the host build of the same header (tests/host_sim/specaug_sim.cpp,
which tests/test_specaug_host.py holds to numpy, to the definition's properties and to float64). The draws are integer arithmetic,
fmaf is correctly rounded on both sides and nothing else rounds but one subtraction, so every comparison is bit for bit, output
and draws:

* the parameter sets of sa.PARAMS at the bins 1, 23, 80, 129 and the frames 1, tile_out, tile_out + 1, 3 tile_out + 5, five rows
  with the lengths 0, 1, 2 W + 1, frames and frames + 9, both layouts in and both out, with gaps between rows and lines, odd base
  offsets, NaN / Inf in padding and gaps, canaries around the output and the draws; the same at the wide bins 193, 257, 513, 1025
  and 4096 (sa.WIDE_BINS), where tile_out is 31, 23, 11, 5 and 1 and there are more bins than work items;
* in place without a warp; a strided view; ids against row_base; spec_augment against the handle, and the cache;
* load_features with augment over three synthesised .m4a files against the pass applied to load_features without it, and
  augment=None against the chain as it was, byte for byte;
* the lifecycle of the handle, the C++ mirror;
* two rows more than 2^32 elements apart, in and out, and in place.

No test provokes a fault: every refusal happens on the host, and every buffer has the size the entry asks for."""
import ctypes

import numpy as np
import pytest

from tests import specaug_ref as sa

pytestmark = pytest.mark.gpu

F32 = np.float32
CANARY = F32(-12345.5)
SEED = 0x1234_5678_9ABC_DEF1
CASES = [(name, bins) for name in sa.PARAMS for bins in sa.BINS]
CASES += [(name, bins) for bins in sa.WIDE_BINS for name in sa.PARAMS]  # tile_out 31, 23, 11, 5 and 1
IDS = ["%s-%d" % c for c in CASES]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture(scope="module")
def sim():
    return sa.build_specaug_sim()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def new_specaug(pkg, ps, bins, mask_value=0.0, pad_value=0.0):
    h = pkg.NewSpecAugment(bins, ps[0], ps[1], ps[2], ps[3], ps[4] / 65536.0, ps[5], mask_value, pad_value)
    assert h.config.time_ratio_q16 == ps[4]
    return h


def device_run(torch, h, ps, x, lengths, in_layout, out_layout, row_gap=0, inner_gap=0, lead=0, poison=None, row_base=0, ids=None):
    """The pass over x laid out in a buffer with gaps, through specaug_device -> (y [rows, frames, bins], draws) as numpy; asserts
    that nothing but the output's elements and the rows' draws changed"""
    rows, frames, bins = x.shape
    P = 2 + 2 * ps[0] + 2 * ps[2]
    xin = x.copy()
    if poison is not None:
        for r, n in enumerate(sa.clamp_lengths(lengths, rows, frames)):
            xin[r, n:] = poison
    buf, _, st = sa.lay_out(xin, in_layout, row_gap, inner_gap, lead, fill=CANARY if poison is None else poison)
    olead = (lead + 1) % 4
    obuf, _, ost = sa.lay_out(np.zeros_like(x), out_layout, row_gap + 1, inner_gap + 2, olead, fill=CANARY)
    d_in, d_out = to_dev(torch, buf), to_dev(torch, obuf)
    d_len = None if lengths is None else to_dev(torch, np.asarray(lengths, np.int32))
    d_ids = None if ids is None else to_dev(torch, np.asarray(ids, np.int64))
    d_draws = torch.full((rows + 2, P), -77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    h.specaug_device(d_in.data_ptr() + 4 * lead, st, rows, frames, 0 if d_len is None else d_len.data_ptr(), SEED,
                     d_out.data_ptr() + 4 * olead, ost, row_base, 0 if d_ids is None else d_ids.data_ptr(), d_draws.data_ptr() + 4 * P,
                     sync=True)
    assert h.last_ms() > 0
    got, draws = d_out.cpu().numpy(), d_draws.cpu().numpy()
    rest = sa.outside(got, lambda b: sa.view_like(b, olead, x.shape, ost))
    assert rest.size and (rest.view(np.uint32) == CANARY.view(np.uint32)).all(), "an element outside the output was written"
    assert np.array_equal(d_in.cpu().numpy().view(np.uint32), buf.view(np.uint32)), "the input changed"
    assert (draws[0] == -77).all() and (draws[-1] == -77).all(), "a draw outside the rows' was written"
    return sa.view_like(got, olead, x.shape, ost).copy(), draws[1:-1]


# ---- 1. the CPU suite's cases against the host build ---------------------------------------------------------------------
@pytest.mark.parametrize("name,bins", CASES, ids=IDS)
def test_the_host_cases_on_the_device(torch, pkg, sim, name, bins):
    ps = sa.for_bins(sa.PARAMS[name], bins)
    rng = np.random.default_rng(1000 + bins)
    T = sa.tile_out_of(bins)
    k = 0
    with new_specaug(pkg, ps, bins, -7.0, -3.5) as h:
        pl = h.plan()
        assert {key: pl[key] for key in ("draws", "tile_out", "lds_bytes")} == sa.plan_of(ps, bins)
        for frames in sorted({1, T, T + 1, 3 * T + 5}):
            lengths = [0, 1, 2 * ps[5] + 1, frames, frames + 9]
            x = sa.features(rng, 5, frames, bins)
            want, want_draws = sa.host_values(sim, x, lengths, ps, SEED, row_base=11, mask_value=-7.0, pad_value=-3.5)
            for in_layout in ("frames", "bins"):
                for out_layout in ("frames", "bins"):
                    lead = (k % 4) | (1 if k % 3 else 0)
                    poison = (F32(np.nan), F32(np.inf), None, F32(-np.inf))[(k // 4) % 4]
                    k += 1
                    y, draws = device_run(torch, h, ps, x, lengths, in_layout, out_layout, row_gap=(0, 5, 1, 7)[lead],
                                          inner_gap=(0, 3, 1, 2)[lead], lead=lead, poison=poison, row_base=11)
                    assert sa.same_bits(y, want), "%d frames, %s -> %s, lead %d" % (frames, in_layout, out_layout, lead)
                    assert np.array_equal(draws, want_draws), "draws"
        # no lengths: every frame is valid; ids in place of the row base
        ids = [2 ** 63 - 1, -1, 13]
        y, draws = device_run(torch, h, ps, x[:3], None, "bins", "frames", ids=ids)
        want, want_draws = sa.host_values(sim, x[:3], None, ps, SEED, ids=ids, mask_value=-7.0, pad_value=-3.5)
        assert sa.same_bits(y, want) and np.array_equal(draws, want_draws)


# ---- 2. the tensor interface ---------------------------------------------------------------------------------------------
def test_in_place_views_ids_and_the_functional_entry(torch, pkg, sim):
    rng = np.random.default_rng(7)
    F, bins = 151, 24
    x = sa.features(rng, 4, F, bins)
    lengths = [F, 7, 0, 99]
    feats = to_dev(torch, x)  # [4, F, 24]
    masks, warp = (2, 6, 2, 30, 65536, 0), (2, 6, 2, 30, 32768, 4)
    # in place without a warp, both layouts
    want, want_draws = sa.host_values(sim, x, lengths, masks, SEED, mask_value=1.5, pad_value=-1.0)
    with new_specaug(pkg, masks, bins, 1.5, -1.0) as h:
        work = feats.clone()
        y, draws = h(work, lengths, SEED, out=work, return_draws=True)
        assert y is work and sa.same_bits(work.cpu().numpy(), want) and draws.dtype is torch.int32
        assert np.array_equal(draws.cpu().numpy(), want_draws)
        tb = feats.transpose(1, 2).contiguous()  # [4, 24, F]: the bins layout
        assert h(tb, lengths, SEED, layout="bins", out=tb) is tb and sa.same_bits(tb.transpose(1, 2).cpu().numpy(), want)
        with pytest.raises(ValueError):
            h(work, lengths, SEED, out=work, out_layout="bins")
    # a strided view: 23 bins at a frame stride of 24, with a warp
    view = feats[..., :-1]
    assert view.stride() == (F * bins, bins, 1)
    want, want_draws = sa.host_values(sim, x[..., :-1], lengths, warp, SEED, row_base=40)
    before = feats.clone()
    with new_specaug(pkg, warp, 23) as h:
        y, draws = h(view, lengths, SEED, row_base=40, return_draws=True)
        assert tuple(y.shape) == want.shape and y.is_contiguous() and torch.equal(feats, before)
        assert sa.same_bits(y.cpu().numpy(), want) and np.array_equal(draws.cpu().numpy(), want_draws)
        yb = h(view, lengths, SEED, row_base=40, out_layout="bins")
        assert tuple(yb.shape) == (4, 23, F) and torch.equal(yb.transpose(1, 2), y)
        # ids against row_base: a row's augmentation is its identity's, wherever it stands in the batch
        order = [2, 0, 3, 1]
        shuffled = h(view[order], [lengths[j] for j in order], SEED, ids=[40 + j for j in order])
        assert torch.equal(shuffled, y[order])
        alone = h(view[3:4], lengths[3:4], SEED, ids=torch.tensor([43], device="cuda:0"))
        assert torch.equal(alone[0], y[3])
        assert not torch.equal(h(view, lengths, SEED, row_base=41)[0], y[0])
        assert not torch.equal(h(view, lengths, SEED + 1, row_base=40)[0], y[0])
        # leading dimensions, an out tensor, lengths on the device
        out = torch.full((2, 2, F, 23), 5.0, device="cuda:0")
        y2, d2 = h(view.reshape(2, 2, F, 23), torch.tensor(lengths, device="cuda:0").reshape(2, 2), SEED, row_base=40, out=out,
                   return_draws=True)
        assert y2 is out and torch.equal(out.reshape(y.shape), y) and tuple(d2.shape) == (2, 2, 10)
        # in place with a warp, and what the class refuses
        own = view.contiguous()
        for call in (lambda: h(own, lengths, SEED, out=own), lambda: h(view.double(), lengths, SEED), lambda: h(feats, lengths, SEED),
                     lambda: h(view, [1, 2, 3], SEED), lambda: h(view, lengths, SEED, ids=[1, 2, 3]), lambda: h(view, lengths, -1),
                     lambda: h(view, lengths, SEED, ids=[1.0, 2.0, 3.0, 4.0]),
                     lambda: h(view, lengths, SEED, out=torch.zeros(4, 3, 3, device="cuda:0")),
                     lambda: h.specaug_device(own.data_ptr(), (F * 23, 23, 1), 4, F, 0, SEED, own.data_ptr(), (F * 23, 23, 1))):
            with pytest.raises(ValueError):
                call()
        assert torch.equal(own, view)
    # the functional entry against the handle, and the cache
    before = set(pkg._SPECAUGS)
    kw = dict(freq_masks=2, freq_width=6, time_masks=2, time_width=30, time_ratio=0.5, warp=4)
    a, a_draws = pkg.spec_augment(view, lengths, SEED, row_base=40, return_draws=True, **kw)
    assert torch.equal(a, y) and torch.equal(a_draws, draws) and len(set(pkg._SPECAUGS) - before) == 1
    pkg.spec_augment(view, lengths, seed=SEED + 1, **kw)
    assert len(set(pkg._SPECAUGS) - before) == 1
    # a CPU tensor is uploaded; without masks and warp the pass only masks the padding
    plain = pkg.spec_augment(torch.from_numpy(x), lengths, seed=1, freq_masks=0, time_masks=0, freq_width=0, pad_value=-2.0)
    assert plain.is_cuda and torch.equal(plain[0], feats[0]) and torch.equal(plain[1, :7], feats[1, :7]) and float(plain[2].max()) == -2.0


# ---- 3. raggedness, end to end -------------------------------------------------------------------------------------------
def test_load_features_with_augment(torch, pkg, tmp_path):
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
    n_frames = flen.cpu().tolist()
    assert tuple(base.shape) == (3, 48, 23) and n_frames[0] == n_frames[1] == 48 and 1 < n_frames[2] < 48
    # augment=None runs the chain as it was: byte for byte normalize_features of the same steps
    clips, lengths, _ = pkg.load_clips(paths, offsets, L, sample_rate=16000)
    counts = pkg.kaldi_frame_counts(lengths, 400, 160)
    chain = pkg.normalize_features(pkg.kaldi_fbank(clips[:, 0], sample_frequency=16000, **kw), counts, stat="mean")
    none, nlen, _ = pkg.load_features(paths, offsets, L, sample_rate=16000, augment=None, **kw)
    assert torch.equal(none.view(torch.int32), chain.view(torch.int32)) and torch.equal(base.view(torch.int32), chain.view(torch.int32))
    assert torch.equal(nlen.cpu(), counts.cpu())
    aug = dict(seed=77, ids=[900, 5, 31], freq_masks=2, freq_width=5, time_masks=2, time_width=10, time_ratio=0.5, warp=3)
    feats, alen, _ = pkg.load_features(paths, offsets, L, sample_rate=16000, augment=aug, **kw)
    want, draws = pkg.spec_augment(base, flen, return_draws=True, **aug)
    assert torch.equal(feats.view(torch.int32), want.view(torch.int32)) and torch.equal(alen, flen)
    assert not torch.equal(feats, base) and bool((draws[:, 1] > 0).all()), "every row is long enough for a warp of 3"
    for j, n in enumerate(n_frames):  # masks inside the row's own frames, +0.0 behind them
        d = draws[j].cpu().tolist()
        assert all(0 <= d[6 + 2 * i] and d[6 + 2 * i] + d[7 + 2 * i] <= n and d[7 + 2 * i] <= n // 2 for i in range(2))
        assert not bool(feats[j, n:].view(torch.int32).any())
    # in front of the stacking: the stacked features are the stacking of the augmented ones
    stacked, slen, _ = pkg.load_features(paths, offsets, L, sample_rate=16000, augment=aug, deltas=1, subsample=2, **kw)
    ws, wl = pkg.stack_frames(want, flen, order=1, window=2, stride=2)
    assert torch.equal(stacked.view(torch.int32), ws.view(torch.int32)) and torch.equal(slen, wl)


# ---- 4. the handle -------------------------------------------------------------------------------------------------------
def test_lifecycle_and_the_cpp_mirror(torch, pkg, sim):
    rng = np.random.default_rng(9)
    x = sa.features(rng, 3, 70, 23)
    d_x = to_dev(torch, x)
    ps = (1, 5, 1, 12, 65536, 2)
    h = new_specaug(pkg, ps, 23)
    with pytest.raises(ValueError):
        h.last_ms()  # no pass yet on this handle
    h.specaug_device(0, (1, 1, 1), 0, 70, 0, 1, 0, (1, 1, 1))
    h.specaug_device(0, (1, 1, 1), 3, 0, 0, 1, 0, (1, 1, 1))
    with pytest.raises(ValueError):
        h.last_ms()  # nothing was launched
    d_y = torch.zeros(3, 70, 23, device="cuda:0")
    good = (70 * 23, 23, 1)
    for bad_in, bad_out in (((70 * 23, 23, 2), good), (good, (70 * 23, 22, 1)), ((70 * 23 - 1, 23, 1), good), (good, (70 * 23 - 1, 23, 1))):
        with pytest.raises(ValueError):
            h.specaug_device(d_x.data_ptr(), bad_in, 3, 70, 0, 1, d_y.data_ptr(), bad_out)
    for ptr_in, ptr_out in ((0, d_y.data_ptr()), (d_x.data_ptr(), 0), (d_x.data_ptr() + 2, d_y.data_ptr()),
                            (d_x.data_ptr(), d_x.data_ptr()), (d_x.data_ptr(), d_x.data_ptr() + 4 * (3 * 70 * 23 - 1))):
        with pytest.raises(ValueError):
            h.specaug_device(ptr_in, good, 3, 70, 0, 1, ptr_out, good)
    with pytest.raises(ValueError):
        h.last_ms()
    assert not bool(d_y.any()) and h.out_frames(70) == 70
    pl = h.plan()
    assert [pl[k] for k in ("bins", "freq_masks", "freq_width", "time_masks", "time_width", "time_ratio_q16", "warp", "draws")] == [
        23, 1, 5, 1, 12, 65536, 2, 6]
    y, draws = h(d_x, [70, 0, 33], SEED, return_draws=True)
    want, want_draws = sa.host_values(sim, x, [70, 0, 33], ps, SEED)
    assert sa.same_bits(y.cpu().numpy(), want) and np.array_equal(draws.cpu().numpy(), want_draws) and h.last_ms() > 0
    h.synchronize()
    h.close()
    h.close()
    assert h.out_frames(70) == 0
    for call in (h.synchronize, h.last_ms, h.plan, lambda: h(d_x)):
        with pytest.raises(ValueError):
            call()
    # host/spec_augment.hpp through the ctypes shim
    S = sa.build_specaug_shim(pkg)
    cfg = pkg.SpecAugConfig(23, 1, 5, 1, 12, 65536, 2, 2.5, -1.0)
    ids = [7, -9, 2 ** 40]
    want, want_draws = sa.host_values(sim, x, [70, 0, 33], ps, SEED, ids=ids, mask_value=2.5, pad_value=-1.0)
    d_len, d_ids = to_dev(torch, np.asarray([70, 0, 33], np.int32)), to_dev(torch, np.asarray(ids, np.int64))
    d_draws = torch.zeros((3, 6), dtype=torch.int32, device="cuda:0")
    info, ms = pkg.SpecAugInfo(), ctypes.c_float()
    torch.cuda.synchronize()

    def run(strides):
        st = np.asarray(strides, np.uint64)
        return S.specaug_shim_run(ctypes.byref(cfg), d_x.data_ptr(), st.ctypes.data, 3, 70, d_len.data_ptr(), SEED, 0, d_ids.data_ptr(),
                                  d_y.data_ptr(), d_draws.data_ptr(), ctypes.byref(info), ctypes.byref(ms))

    assert run(good + good) == 0, S.specaug_shim_last_error()
    p = sa.plan_of(ps, 23)
    assert ms.value > 0 and (info.draws, info.tile_out, info.lds_bytes) == (6, p["tile_out"], p["lds_bytes"])
    assert (info.mask_value, info.pad_value, info.warp) == (2.5, -1.0, 2)
    assert sa.same_bits(d_y.cpu().numpy(), want) and np.array_equal(d_draws.cpu().numpy(), want_draws)
    assert run(good + (70 * 23, 22, 1)) == -6 and b"stride" in S.specaug_shim_last_error()


# ---- 5. far rows ---------------------------------------------------------------------------------------------------------
def test_rows_more_than_4_gi_elements_apart(torch, pkg, sim):
    """Two rows whose row stride is 2^32 + 12 345 elements, in the input and in the output, each in one allocation of 16 GiB that
    is touched only around the rows: a row offset narrowed to 32 bits would read and write row 1 at element 12 345, which holds
    canaries. The warp reads two source frames per output frame through the row's offset. Then masks only, in place on the input"""
    bins = 23
    ps, masks = sa.for_bins(sa.PARAMS["all"], bins), sa.for_bins(sa.PARAMS["masks"], bins)
    rs, guard = (1 << 32) + 12345, 4096
    with new_specaug(pkg, ps, bins, -7.0, -2.0) as h:
        frames = h.plan()["tile_out"] + 1
    ext = frames * bins
    try:
        big_in = torch.empty(rs + ext + guard, dtype=torch.float32, device="cuda:0")
        big_out = torch.empty(rs + ext + guard, dtype=torch.float32, device="cuda:0")
    except RuntimeError as e:
        pytest.skip("no two allocations of %.1f GiB: %s" % ((rs + ext + guard) * 4 / 2.0 ** 30, str(e).splitlines()[0]))
    x = sa.features(np.random.default_rng(4), 2, frames, bins)
    lengths = [frames - 3, frames]
    for big in (big_in, big_out):
        big[:12345 + ext + guard] = float(CANARY)
        big[rs - guard:rs + ext + guard] = float(CANARY)
    big_in[:ext] = to_dev(torch, x[0].reshape(-1))
    big_in[rs:rs + ext] = to_dev(torch, x[1].reshape(-1))
    rows_in = torch.as_strided(big_in, (2, frames, bins), (rs, bins, 1))
    rows_out = torch.as_strided(big_out, (2, frames, bins), (rs, bins, 1))

    def rows_of(big):
        return np.stack([big[:ext].cpu().numpy(), big[rs:rs + ext].cpu().numpy()]).reshape(2, frames, bins)

    def guards_intact(big):
        return all(bool((big[a:b] == float(CANARY)).all()) for a, b in ((ext, 12345 + ext + guard), (rs - guard, rs),
                                                                        (rs + ext, rs + ext + guard)))

    with new_specaug(pkg, ps, bins, -7.0, -2.0) as h:
        out, draws = h(rows_in, lengths, SEED, row_base=5, out=rows_out, return_draws=True)
    assert out is rows_out
    want, want_draws = sa.host_values(sim, x, lengths, ps, SEED, row_base=5, mask_value=-7.0, pad_value=-2.0)
    assert (want_draws[:, 1] > 0).all(), "both rows are warped"
    assert sa.same_bits(rows_of(big_out), want) and np.array_equal(draws.cpu().numpy(), want_draws)
    assert guards_intact(big_out), "an element outside the two rows was written"
    assert sa.same_bits(rows_of(big_in), x) and guards_intact(big_in), "the input changed"
    # masks only, in place on the input view
    with new_specaug(pkg, masks, bins, -7.0, -2.0) as h:
        out, draws = h(rows_in, lengths, SEED, row_base=5, out=rows_in, return_draws=True)
    assert out is rows_in
    want, want_draws = sa.host_values(sim, x, lengths, masks, SEED, row_base=5, mask_value=-7.0, pad_value=-2.0)
    assert sa.same_bits(rows_of(big_in), want) and np.array_equal(draws.cpu().numpy(), want_draws) and not sa.same_bits(want, x)
    assert guards_intact(big_in), "an element outside the two rows was written"
    del big_in, big_out, rows_in, rows_out, out
    torch.cuda.empty_cache()
