"""The feature normalisation pass on the MI355X (k_featnorm.hip), held to the host build of the same header
(tests/host_sim/featnorm_sim.cpp, which tests/test_featnorm_host.py holds to numpy and float64):

* the CPU suite's cases (fr.MODES at the bins 1, 23, 80, 129, five frame counts around tile_frames, six rows with the lengths 0,
  1, a middle value, frames, -5 and frames + 7, both layouts): output and stats bit for bit the host build's for none, mean, max
  and the affine; for mean_var the mean bit for bit, rstd within 2 float32 ulp (the device's sqrtf is specified to 1 ulp, the
  division rounds once more), and the output bit for bit numpy's (x - mean) * rstd over the device's own stats;
* gaps between rows and lines, base offsets, one layout in and the other out, in place, NaN / Inf in padding and gaps, canaries;
* both of these at the wide bins 193, 257, 513, 1025 and 4096 as well (fr.WIDE_BINS), where tile_frames is 32, 32, 16, 8 and 2
  and the finishing kernel runs 1, 2, 3, 5 and 16 workgroups per row; the statistics of 257 and 4096 bins on their own; the
  max-clamp of a 513-bin spectrogram view through normalize_features;
* whisper_post and amplitude_to_DB's clamp against the torch ops, on the strided view logmel[..., :-1];
* load_features over three synthesised .m4a files of two sample rates, one shorter than the clip, against the pass applied to
  kaldi_fbank of each clip cut to its length;
* the lifecycle of the handle, the cache of normalize_features, kaldi_frame_counts against a handle's out_frames, the C++ mirror;
* two rows more than 2^32 elements apart.

No test provokes a fault: every refusal happens on the host, and every buffer has the size the entry asks for."""
import ctypes

import numpy as np
import pytest

from tests import featnorm_ref as fr

pytestmark = pytest.mark.gpu

F32 = np.float32
ROWS = 6
CANARY = F32(-12345.5)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture(scope="module")
def sim():
    return fr.build_featnorm_sim()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def new_norm(pkg, bins, stat="mean", shift=None, scale=None, var_floor=1e-20, range_=None, pad=0.0):
    return pkg.NewFeatureNorm(bins, stat, shift, scale, var_floor, range_, pad)


def device_run(torch, pkg, x, lengths, in_layout, out_layout, args, row_gap=0, inner_gap=0, lead=0, poison=None, in_place=False):
    """The pass over x laid out in a buffer with gaps, through norm_device -> (y [rows, frames, bins], stats) as numpy; asserts that
    nothing but the output's elements changed"""
    rows, frames, bins = x.shape
    xin = x.copy()
    if poison is not None:
        for r, n in enumerate(fr.clamp_lengths(lengths, rows, frames)):
            xin[r, n:] = poison
    buf, view, st = fr.lay_out(xin, in_layout, row_gap, inner_gap, lead, fill=CANARY if in_place or poison is None else poison)
    if in_place:
        obuf, ost, olead = buf, st, lead
    else:
        olead = (lead + 1) % 4
        obuf, _, ost = fr.lay_out(np.zeros_like(x), out_layout, row_gap + 1, inner_gap + 2, olead, fill=CANARY)
    d_in = to_dev(torch, buf)
    d_out = d_in if in_place else to_dev(torch, obuf)
    d_len = None if lengths is None else to_dev(torch, np.asarray(lengths, np.int32))
    d_stats = torch.full((rows, 2, bins), float(CANARY), dtype=torch.float32, device="cuda:0")
    with new_norm(pkg, bins, **args) as h:
        torch.cuda.synchronize()
        h.norm_device(d_in.data_ptr() + 4 * lead, st, rows, frames, 0 if d_len is None else d_len.data_ptr(),
                      d_out.data_ptr() + 4 * olead, ost, d_stats.data_ptr(), sync=True)
        assert h.last_ms() > 0
    got = d_out.cpu().numpy()
    rest = fr.outside(got, lambda b: fr.view_like(b, olead, x.shape, ost))
    assert rest.size and (rest.view(np.uint32) == CANARY.view(np.uint32)).all(), "an element outside the output was written"
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy().view(np.uint32), buf.view(np.uint32)), "the input changed"
    return fr.view_like(got, olead, x.shape, ost).copy(), d_stats.cpu().numpy()


def ulps(a, b):
    """The distance of two positive float32 arrays in units in the last place"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_against_host(sim, x, lengths, args, y, stats, what):
    want, want_stats = fr.host_values(sim, x, lengths, "frames", **args)
    if args.get("stat") != "mean_var":
        assert fr.same_bits(y, want), what + ": output"
        assert fr.same_bits(stats, want_stats), what + ": stats"
        return 0
    rows, frames, bins = x.shape
    assert fr.same_bits(stats[:, 0], want_stats[:, 0]), what + ": mean"
    valid = np.array(fr.clamp_lengths(lengths, rows, frames)) > 0
    assert not stats[~valid].view(np.uint32).any()
    d = ulps(stats[valid, 1], want_stats[valid, 1])
    print("%s: rstd at most %d ulp from the host build's" % (what, d.max() if d.size else 0))
    assert (d <= 2).all(), what + ": rstd %d ulp off" % d.max()
    # the apply step on its own: numpy over the device's own stats
    exp = np.full(x.shape, F32(args.get("pad", 0.0)), F32)
    for r, n in enumerate(fr.clamp_lengths(lengths, rows, frames)):
        s = (x[r, :n] - stats[r, 0]) * stats[r, 1]
        if args.get("shift") is not None:
            s = s - args["shift"]
        if args.get("scale") is not None:
            s = s * args["scale"]
        exp[r, :n] = s
    assert fr.same_bits(y, exp), what + ": output over the device's own stats"
    return int(d.max()) if d.size else 0


# ---- 1. the CPU suite's cases against the host build ---------------------------------------------------------------------
@pytest.mark.parametrize("bins", fr.BINS + fr.WIDE_BINS)
@pytest.mark.parametrize("mode", list(fr.MODES))
def test_the_host_cases_on_the_device(torch, pkg, sim, mode, bins):
    tf = fr.tile_frames_of(bins)
    args = fr.mode_args(mode, bins)
    with new_norm(pkg, bins, **args) as h:
        assert h.plan()["tile_frames"] == tf and (tf == 64) == (bins <= 192)
    rng = np.random.default_rng(1000 + bins)
    for k, frames in enumerate(fr.frames_of(tf)):
        if frames < 1:
            continue
        x = fr.features(rng, ROWS, frames, bins)
        lengths = fr.lengths_of(frames)
        got = {}
        for layout in ("frames", "bins"):
            y, stats = device_run(torch, pkg, x, lengths, layout, layout, args, lead=k % 4)
            check_against_host(sim, x, lengths, args, y, stats, "%s, %d bins, %d frames, %s" % (mode, bins, frames, layout))
            got[layout] = (y, stats)
        assert fr.same_bits(got["frames"][0], got["bins"][0]) and fr.same_bits(got["frames"][1], got["bins"][1]), "the layouts differ"


@pytest.mark.parametrize("bins", fr.BINS + fr.WIDE_BINS)
@pytest.mark.parametrize("mode", ["mean_var", "whisper", "mean_affine"])
def test_gaps_offsets_poisoned_padding_and_in_place(torch, pkg, sim, mode, bins):
    tf = fr.tile_frames_of(bins)
    args = fr.mode_args(mode, bins)
    rng = np.random.default_rng(3000 + bins)
    frames = 2 * tf + 3
    x = fr.features(rng, ROWS, frames, bins)
    lengths = fr.lengths_of(frames)
    k = 0
    for in_layout in ("frames", "bins"):
        for out_layout in ("frames", "bins"):
            lead = k % 4
            poison = (F32(np.nan), F32(np.inf), F32(-np.inf), None)[k % 4]
            y, stats = device_run(torch, pkg, x, lengths, in_layout, out_layout, args, row_gap=(0, 5, 1, 7)[lead],
                                  inner_gap=(0, 3, 1, 2)[lead], lead=lead, poison=poison)
            check_against_host(sim, x, lengths, args, y, stats, "%s -> %s, lead %d" % (in_layout, out_layout, lead))
            k += 1
        y, stats = device_run(torch, pkg, x, lengths, in_layout, in_layout, args, row_gap=5, inner_gap=3, lead=3, in_place=True)
        check_against_host(sim, x, lengths, args, y, stats, "%s in place" % in_layout)


@pytest.mark.parametrize("bins", [257, 4096])
@pytest.mark.parametrize("mode", ["mean_var", "max"])
def test_statistics_of_more_than_one_finishing_block(torch, pkg, sim, mode, bins):
    """The returned stats [rows][2][bins] where alac_featnorm_finish runs ceil(bins / 256) > 1 workgroups per row for the sums (at
    257 bins the second holds one bin) and one per row, which writes all 2 bins values, for the maximum: the host build calls
    finish_bin per bin and knows no blocks, so this is the only observer of row = b / blocks and bin = (b - row * blocks) * 256 +
    tid. mean_var: the mean bit for bit, rstd within the 2 ulp of this file (the device's sqrtf and one division), rows without a
    frame +0.0; max: M in [r][0][0] bit for bit and every other value +0.0."""
    args = fr.mode_args(mode, bins)
    with new_norm(pkg, bins, **args) as h:
        pl = h.plan()
    tf, blocks = pl["tile_frames"], -(-pl["bins"] // 256)
    assert tf == fr.tile_frames_of(bins) and blocks >= 2
    frames = 2 * tf + 3
    x = fr.features(np.random.default_rng(7000 + bins), ROWS, frames, bins)
    lengths = fr.lengths_of(frames)
    valid = np.array(fr.clamp_lengths(lengths, ROWS, frames)) > 0
    want, want_stats = fr.host_values(sim, x, lengths, "frames", **args)
    assert want_stats[valid].any(axis=(1, 2)).all() and not want_stats[~valid].view(np.uint32).any()
    for layout in ("frames", "bins"):
        y, stats = device_run(torch, pkg, x, lengths, layout, layout, args, row_gap=3, inner_gap=1, lead=1)
        assert stats.shape == (ROWS, 2, bins)
        if mode == "max":
            assert fr.same_bits(stats, want_stats) and fr.same_bits(y, want)
            assert fr.same_bits(stats[valid, 0, 0], np.array([fr.largest(x[r, :n]) for r, n in
                                                              enumerate(fr.clamp_lengths(lengths, ROWS, frames)) if n], F32))
            rest = stats.reshape(ROWS, -1)[:, 1:]
            assert rest.shape[1] == 2 * bins - 1 and not rest.view(np.uint32).any(), "a value behind the maximum is not +0.0"
        else:
            assert fr.same_bits(stats[:, 0], want_stats[:, 0]), "mean"
            assert not stats[~valid].view(np.uint32).any()
            assert (ulps(stats[valid, 1], want_stats[valid, 1]) <= 2).all(), "rstd"
            assert (stats[valid, 1] > 0).all()
            check_against_host(sim, x, lengths, args, y, stats, "%s, %d bins, %s" % (mode, bins, layout))


# ---- 2. against the torch ops --------------------------------------------------------------------------------------------
def test_max_clamp_of_a_513_bin_spectrogram_view(torch, pkg, sim):
    """normalize_features on a spectrogram of n_fft 1024 in the bins layout: the view spec[..., :-1] of a [2, 513, F] tensor (bin
    stride F, F - 1 frames at frame stride 1), stat max, against the host build of the same view, output and statistics; the
    largest value of row 1 lies in the frame that the view drops"""
    bins = 513
    tf = fr.tile_frames_of(bins)
    F = 2 * tf + 4
    rng = np.random.default_rng(513)
    x = rng.uniform(-10.0, 1.5, (2, bins, F)).astype(F32)
    x[1, 300, F - 1] = 9.0
    spec = to_dev(torch, x)
    view = spec[..., :-1]
    assert view.stride() == (bins * F, F, 1) and tuple(view.shape) == (2, bins, F - 1)
    before = spec.clone()
    lengths = [F - 1, tf + 1]
    logical = np.ascontiguousarray(x[..., :-1].transpose(0, 2, 1))  # [rows, frames, bins]
    want, want_stats = fr.host_values(sim, logical, lengths, "bins", stat="max", range_=8.0, pad=-1.0)
    got, stats = pkg.normalize_features(view, lengths, stat="max", layout="bins", range=8.0, pad_value=-1.0, return_stats=True)
    assert tuple(got.shape) == (2, bins, F - 1) and got.is_contiguous() and torch.equal(spec, before)
    assert fr.same_bits(got.cpu().numpy().transpose(0, 2, 1), want)
    assert fr.same_bits(stats.cpu().numpy(), want_stats) and float(stats[1, 0, 0]) < 9.0
    assert not fr.same_bits(want, logical), "the clamp changed nothing"


def test_whisper_post_and_the_db_clamp(torch, pkg):
    """whisper_post(logmel) == FeatureNorm(max, range 8, shift -4, scale 0.25) on the view logmel[..., :-1] (bin stride F, F - 1
    frames), bit for bit; and amplitude_to_DB's clamp at top_db 80 on dB values"""
    tf = fr.tile_frames_of(80)
    rng = np.random.default_rng(80)
    F = 2 * tf + 4
    logmel = to_dev(torch, rng.uniform(-10.0, 1.5, (3, 80, F)).astype(F32))
    logmel[1, 40, F - 1] = 9.0  # the largest value of row 1 is in the frame that is dropped
    want = pkg.whisper_post(logmel)
    view = logmel[..., :-1]
    assert view.stride() == (80 * F, F, 1)
    before = logmel.clone()
    with pkg.NewFeatureNorm(80, "max", shift=-4.0, scale=0.25, range=8.0) as h:
        got = h(view, layout="bins")
        assert tuple(got.shape) == (3, 80, F - 1) and got.is_contiguous() and torch.equal(logmel, before)
        assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    again = pkg.normalize_features(view, stat="max", layout="bins", range=8.0, shift=-4.0, scale=0.25)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    db = to_dev(torch, rng.uniform(-140.0, 30.0, (3, 80, F)).astype(F32))
    want = torch.maximum(db, db.amax(dim=(-2, -1), keepdim=True) - 80.0)
    got = pkg.normalize_features(db, stat="max", layout="bins", range=80.0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not torch.equal(got, db)


# ---- 3. raggedness, end to end -------------------------------------------------------------------------------------------
def test_load_features_over_ragged_files(torch, pkg, tmp_path):
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
    for norm in ("mean", "mean_var", None):
        feats, flen, rate = pkg.load_features(paths, offsets, L, sample_rate=16000, norm=norm, **kw)
        clips, lengths, _ = pkg.load_clips(paths, offsets, L, sample_rate=16000)
        n_samples = lengths.cpu().tolist()
        assert rate == 16000 and n_samples[0] == L and n_samples[1] == L and 400 < n_samples[2] < L
        counts = pkg.kaldi_frame_counts(lengths, 400, 160)
        assert flen.dtype is torch.int32 and torch.equal(flen.cpu(), counts.cpu())
        F = 1 + (L - 400) // 160
        assert tuple(feats.shape) == (3, F, 23)
        with pkg.NewFeatureNorm(23, norm) as h:
            for j in range(3):
                n = int(flen[j])
                assert n == 1 + (n_samples[j] - 400) // 160
                cut = clips[j, 0, :n_samples[j]].contiguous()
                want = h(pkg.kaldi_fbank(cut[None], 16000, **kw))[0]
                assert tuple(want.shape) == (n, 23)
                assert torch.equal(feats[j, :n].view(torch.int32), want.view(torch.int32)), "row %d, norm %s" % (j, norm)
                assert not bool(feats[j, n:].view(torch.int32).any()), "the frames behind row %d's are not +0.0" % j
        if norm == "mean":
            assert float(feats[2, :int(flen[2])].mean(dim=0).abs().max()) < 1e-4
    mf, _, _ = pkg.load_features(paths, offsets, L, sample_rate=16000, kind="mfcc", norm="mean")
    assert tuple(mf.shape) == (3, F, 13)
    for bad in (dict(kind="plp"), dict(norm="max"), dict(channel=1), dict(layout="bins")):
        with pytest.raises(ValueError):
            pkg.load_features(paths, offsets, L, sample_rate=16000, **bad)


# ---- 4. the handle -------------------------------------------------------------------------------------------------------
def test_lifecycle_scratch_and_cache(torch, pkg):
    x = to_dev(torch, fr.features(np.random.default_rng(9), 4, 150, 23))
    h = pkg.NewFeatureNorm(23, "mean_var")
    with pytest.raises(ValueError):
        h.last_ms()  # no pass yet on this handle
    h.norm_device(0, (1, 1, 1), 0, 150, 0, 0, (1, 1, 1))
    h.norm_device(0, (1, 1, 1), 4, 0, 0, 0, (1, 1, 1))
    with pytest.raises(ValueError):
        h.last_ms()  # nothing was launched
    for bad_in, bad_out in (((150 * 23, 23, 2), (150 * 23, 23, 1)), ((150 * 23, 23, 1), (150 * 23, 22, 1)),
                            ((150 * 23 - 1, 23, 1), (150 * 23, 23, 1))):
        with pytest.raises(ValueError):
            h.norm_device(x.data_ptr(), bad_in, 4, 150, 0, x.data_ptr(), bad_out)
    with pytest.raises(ValueError):
        h.norm_device(0, (150 * 23, 23, 1), 4, 150, 0, x.data_ptr(), (150 * 23, 23, 1))
    with pytest.raises(ValueError):
        h.last_ms()
    assert h.out_frames(150) == 150
    p0 = h.plan()
    first = h(x, lengths=[150, 7, 0, 99])
    p1 = h.plan()
    second = h(x, lengths=[150, 7, 0, 99])
    p2 = h.plan()
    assert p1["scratch_bytes"] >= 4 * (4 * 3 * 23 + 4 * 2 * 23) and p1["scratch_bytes"] >= p0["scratch_bytes"]
    assert (p2["scratch_bytes"], p2["scratch_address"]) == (p1["scratch_bytes"], p1["scratch_address"]), "the second pass allocated"
    assert p1["tile_frames"] == 64 and p1["bins"] == 23 and p1["stat"] == 2 and p1["shift"] is None and p1["scale"] is None
    assert torch.equal(first.view(torch.int32), second.view(torch.int32)) and h.last_ms() > 0
    h(x[:2], lengths=[5, 5])
    assert h.plan()["scratch_address"] == p1["scratch_address"], "a smaller pass allocated"
    out, stats = h(x, lengths=torch.tensor([150, 7, 0, 99], device="cuda:0"), return_stats=True)
    assert tuple(stats.shape) == (4, 2, 23) and torch.equal(out, first) and not bool(stats[2].any()) and bool((stats[0, 1] > 0).all())
    y = x.clone()
    assert h(y, lengths=[150, 7, 0, 99], out=y) is y and torch.equal(y, first)
    t = x.transpose(1, 2).contiguous()  # [4, 23, 150]
    assert torch.equal(h(t, lengths=[150, 7, 0, 99], layout="bins").transpose(1, 2), first)
    for bad in (x.double(), x[..., :22], x.cpu().numpy()):
        with pytest.raises(ValueError):
            h(bad)
    with pytest.raises(ValueError):
        h(x, lengths=[1, 2, 3])
    h.synchronize()
    h.close()
    h.close()
    assert h.out_frames(150) == 0
    for call in (h.synchronize, h.last_ms, h.plan, lambda: h(x)):
        with pytest.raises(ValueError):
            call()
    with pkg.NewFeatureNorm(23, shift=np.arange(23), scale=2.0) as g:
        pl = g.plan()
        assert np.array_equal(pl["shift"], np.arange(23, dtype=F32)) and np.array_equal(pl["scale"], np.full(23, 2, F32))
    assert g.out_frames(3) == 0
    before = set(pkg._NORMS)
    floor = 1.5e-20  # a parameter set no other test of this process has used; the variances here are far above it
    a = pkg.normalize_features(x, [150, 7, 0, 99], stat="mean_var", var_floor=floor)
    added = set(pkg._NORMS) - before
    assert len(added) == 1 and torch.equal(a, first)
    pkg.normalize_features(x, [150, 7, 0, 99], stat="mean_var", var_floor=floor)
    assert set(pkg._NORMS) - before == added
    pkg.normalize_features(x, stat="mean_var", var_floor=floor, shift=np.zeros(23, F32))
    pkg.normalize_features(x, stat="mean_var", var_floor=floor, shift=np.zeros(23, F32))
    pkg.normalize_features(x, stat="mean_var", var_floor=floor, shift=np.ones(23, F32))
    assert len(set(pkg._NORMS) - before) == 3, "shift enters the key by its bytes"


def test_frame_counts_are_a_handles(torch, pkg):
    for W, h in ((400, 160), (1200, 480)):
        for snip in (True, False):
            with pkg.NewKaldiFeatures(W * 40, W, h, snip_edges=snip) as kf:
                T = list(range(0, 3 * W + 1))
                want = [kf.out_frames(t) for t in T]
            assert pkg.kaldi_frame_counts(torch.tensor(T, dtype=torch.int32, device="cuda:0"), W, h, snip).cpu().tolist() == want


def test_cpp_mirror(torch, pkg, sim):
    """host/feature_norm.hpp through the ctypes shim: the bits are the host build's, the plan's numbers, what it refuses"""
    S = fr.build_featnorm_shim(pkg)
    rng = np.random.default_rng(77)
    x = fr.features(rng, 3, 70, 23)
    lengths = [70, 0, 33]
    shift, scale = rng.uniform(-1, 1, 23).astype(F32), rng.uniform(0.5, 2, 23).astype(F32)
    want, want_stats = fr.host_values(sim, x, lengths, "frames", stat="mean", shift=shift, scale=scale, pad=-1.0)
    d_in, d_len = to_dev(torch, x), to_dev(torch, np.asarray(lengths, np.int32))
    d_out, d_stats = torch.zeros_like(d_in), torch.zeros((3, 2, 23), dtype=torch.float32, device="cuda:0")
    cfg = pkg.NormConfig(23, 1, 1e-20, 0.0, -1.0)
    of, info, sizes, ms = ctypes.c_uint64(), np.zeros(6, np.uint32), np.zeros(2, np.uint64), ctypes.c_float()
    torch.cuda.synchronize()

    def run(strides):
        st = np.asarray(strides, np.uint64)
        return S.featnorm_shim_run(ctypes.byref(cfg), shift.ctypes.data, scale.ctypes.data, d_in.data_ptr(), st.ctypes.data, 3, 70,
                                   d_len.data_ptr(), d_out.data_ptr(), d_stats.data_ptr(), ctypes.byref(of), info.ctypes.data,
                                   sizes.ctypes.data, ctypes.byref(ms))

    assert run([70 * 23, 23, 1] * 2) == 0, S.featnorm_shim_last_error()
    assert of.value == 70 and info.tolist() == [23, 1, 64, 4 * (((23 * 65 + 3) & ~3) + 256), 23, 23] and sizes.tolist() == [23, 23]
    assert ms.value > 0 and fr.same_bits(d_out.cpu().numpy(), want) and fr.same_bits(d_stats.cpu().numpy(), want_stats)
    assert run([70 * 23, 23, 1, 70 * 23, 22, 1]) == -6 and b"stride" in S.featnorm_shim_last_error()


# ---- 5. far rows ---------------------------------------------------------------------------------------------------------
def test_rows_more_than_4_gi_elements_apart(torch, pkg, sim):
    """Two rows of [tile_frames + 1, 23] whose row stride is 2^32 + 12 345 elements, in place in one allocation of 16 GiB that is
    touched only around the rows: a row offset narrowed to 32 bits would put row 1 at element 12 345, which holds canaries"""
    bins, tf = 23, fr.tile_frames_of(23)
    frames = tf + 1
    rs, extent, guard = (1 << 32) + 12345, frames * bins, 4096
    try:
        big = torch.empty(rs + extent + guard, dtype=torch.float32, device="cuda:0")
    except RuntimeError as e:
        pytest.skip("no allocation of %.1f GiB: %s" % ((rs + extent + guard) * 4 / 2.0 ** 30, str(e).splitlines()[0]))
    x = fr.features(np.random.default_rng(4), 2, frames, bins)
    lengths = [frames - 3, frames]
    zones = [(0, 12345 + extent + guard), (rs - guard, rs + extent + guard)]
    for a, b in zones:
        big[a:b] = float(CANARY)
    big[:extent] = to_dev(torch, x[0].reshape(-1))
    big[rs:rs + extent] = to_dev(torch, x[1].reshape(-1))
    rows = torch.as_strided(big, (2, frames, bins), (rs, bins, 1))
    with pkg.NewFeatureNorm(bins, "mean_var", pad_value=-2.0) as h:
        out, stats = h(rows, lengths=lengths, out=rows, return_stats=True)
    assert out is rows
    want, want_stats = fr.host_values(sim, x, lengths, "frames", stat="mean_var", pad=-2.0)
    got = np.stack([big[:extent].cpu().numpy(), big[rs:rs + extent].cpu().numpy()]).reshape(2, frames, bins)
    st = stats.cpu().numpy()
    assert fr.same_bits(st[:, 0], want_stats[:, 0]) and (ulps(st[:, 1], want_stats[:, 1]) <= 2).all()
    exp = np.full(x.shape, F32(-2.0), F32)
    for r, n in enumerate(lengths):
        exp[r, :n] = (x[r, :n] - st[r, 0]) * st[r, 1]
    assert fr.same_bits(got, exp)
    assert np.abs(got - want).max() < 1e-5
    for a, b in ((extent, zones[0][1]), (rs - guard, rs), (rs + extent, rs + extent + guard)):
        assert bool((big[a:b] == float(CANARY)).all()), "an element outside the two rows was written"
    del big, rows, out
    torch.cuda.empty_cache()
