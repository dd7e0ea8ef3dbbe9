"""The frame stacking pass on the MI355X (k_stack.hip), held to the host build of the same header (tests/host_sim/stack_sim.cpp,
which tests/test_stack_host.py holds to numpy, to the sources' definitions and to float64). There is no root, division or
logarithm in this pass and fmaf is correctly rounded on both sides, so every comparison is bit for bit:

* the CPU suite's cases (sr.PARAMS at the bins 1, 23, 80, 129 and the slab case, five frame counts around tile_in, six rows with
  the lengths 0, 1, a middle value, frames, -5 and frames + 7, both layouts in and both out) with gaps between rows and lines,
  base offsets, NaN / Inf in padding and gaps, canaries around the output and the out lengths; the same at the wide bins 193, 257,
  513, 1025 and 4096 (sr.WIDE_BINS) with every parameter set that create takes there;
* strided views through FrameStack's __call__; lfr, add_deltas and stack_frames against FrameStack; the cache;
* load_features with deltas, and with context and subsampling, over three synthesised .m4a files against the pass applied to each
  clip cut to its own frame count; with the defaults against normalize_features of the same chain;
* the lifecycle of the handle, the C++ mirror;
* two rows more than 2^32 elements apart, in and out.

No test provokes a fault: every refusal happens on the host, and every buffer has the size the entry asks for."""
import ctypes

import numpy as np
import pytest

from tests import stack_ref as sr

pytestmark = pytest.mark.gpu

F32 = np.float32
ROWS = 6
CANARY = F32(-12345.5)
SLABS = (2, 8, 0, 0, 1)
CASES = [(ps, bins) for ps in sr.PARAMS for bins in sr.BINS if sr.accepted(ps, bins)] + [(SLABS, 700)]
CASES += [(ps, bins) for bins in sr.WIDE_BINS for ps in sr.PARAMS if sr.accepted(ps, bins)]  # at 4096 bins the plain copy alone
IDS = ["%s-%d" % (sr.param_id(ps), bins) for ps, bins in CASES]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return t


@pytest.fixture(scope="module")
def sim():
    return sr.build_stack_sim()


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def new_stack(pkg, ps, bins, pad=0.0):
    return pkg.NewFrameStack(bins, ps[0], ps[1], ps[2], ps[3], ps[4], pad)


def device_run(torch, h, ps, x, lengths, in_layout, out_layout, row_gap=0, inner_gap=0, lead=0, poison=None):
    """The pass over x laid out in a buffer with gaps, through stack_device -> (y [rows, G, D], out_lengths) as numpy; asserts that
    nothing but the output's elements and the rows out lengths changed"""
    rows, frames, bins = x.shape
    G, D = -(-frames // ps[4]), sr.columns_of(ps, bins)
    xin = x.copy()
    if poison is not None:
        for r, n in enumerate(sr.clamp_lengths(lengths, rows, frames)):
            xin[r, n:] = poison
    buf, _, st = sr.lay_out(xin, in_layout, row_gap, inner_gap, lead, fill=CANARY if poison is None else poison)
    olead = (lead + 1) % 4
    obuf, _, ost = sr.lay_out(np.zeros((rows, G, D), F32), out_layout, row_gap + 1, inner_gap + 2, olead, fill=CANARY)
    d_in, d_out = to_dev(torch, buf), to_dev(torch, obuf)
    d_len = None if lengths is None else to_dev(torch, np.asarray(lengths, np.int32))
    d_olen = torch.full((rows + 2,), -77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    h.stack_device(d_in.data_ptr() + 4 * lead, st, rows, frames, 0 if d_len is None else d_len.data_ptr(), d_out.data_ptr() + 4 * olead,
                   ost, d_olen.data_ptr() + 4, sync=True)
    assert h.last_ms() > 0
    got, olen = d_out.cpu().numpy(), d_olen.cpu().numpy()
    rest = sr.outside(got, lambda b: sr.view_like(b, olead, (rows, G, D), ost))
    assert rest.size and (rest.view(np.uint32) == CANARY.view(np.uint32)).all(), "an element outside the output was written"
    assert np.array_equal(d_in.cpu().numpy().view(np.uint32), buf.view(np.uint32)), "the input changed"
    assert olen[0] == olen[-1] == -77, "an out length outside the rows' was written"
    return sr.view_like(got, olead, (rows, G, D), ost).copy(), olen[1:-1]


# ---- 1. the CPU suite's cases against the host build ---------------------------------------------------------------------
@pytest.mark.parametrize("ps,bins", CASES, ids=IDS)
def test_the_host_cases_on_the_device(torch, pkg, sim, ps, bins):
    rng = np.random.default_rng(1000 + bins)
    k = 0
    with new_stack(pkg, ps, bins, pad=-3.5) as h:
        pl = h.plan()
        assert {key: pl[key] for key in sr.INFO[:5]} == {key: sr.plan_of(ps, bins)[key] for key in sr.INFO[:5]}
        for frames in sr.frames_of(ps, bins):
            x = sr.features(rng, ROWS, frames, bins)
            lengths = sr.lengths_of(frames)
            want, want_len = sr.host_values(sim, x, lengths, ps, pad=-3.5)
            assert h.out_frames(frames) == want.shape[1]
            for in_layout in ("frames", "bins"):
                for out_layout in ("frames", "bins"):
                    lead = k % 4
                    poison = (F32(np.nan), F32(np.inf), None, F32(-np.inf))[(k // 4) % 4]
                    k += 1
                    y, out_len = device_run(torch, h, ps, x, lengths, in_layout, out_layout, row_gap=(0, 5, 1, 7)[lead],
                                            inner_gap=(0, 3, 1, 2)[lead], lead=lead, poison=poison)
                    assert sr.same_bits(y, want), "%d frames, %s -> %s, lead %d" % (frames, in_layout, out_layout, lead)
                    assert np.array_equal(out_len, want_len), "out_lengths"
        # no lengths: every frame is valid
        y, out_len = device_run(torch, h, ps, x[:2], None, "bins", "frames")
        want, want_len = sr.host_values(sim, x[:2], None, ps, pad=-3.5)
        assert sr.same_bits(y, want) and np.array_equal(out_len, want_len)


# ---- 2. the tensor interface ---------------------------------------------------------------------------------------------
def test_strided_views_and_the_functional_entries(torch, pkg, sim):
    rng = np.random.default_rng(7)
    F, bins = 151, 24
    x = sr.features(rng, 4, F, bins)
    lengths = [F, 7, 0, 99]
    feats = to_dev(torch, x)  # [4, F, 24]
    ps = (2, 2, 1, 2, 3)
    view = feats[..., :-1]  # 23 bins at a frame stride of 24
    assert view.stride() == (F * bins, bins, 1)
    want, want_len = sr.host_values(sim, x[..., :-1], lengths, ps, pad=0.0)
    before = feats.clone()
    with pkg.NewFrameStack(23, *ps) as h:
        y, out_len = h(view, lengths)
        assert tuple(y.shape) == want.shape and y.is_contiguous() and torch.equal(feats, before)
        assert sr.same_bits(y.cpu().numpy(), want) and out_len.dtype is torch.int32 and np.array_equal(out_len.cpu().numpy(), want_len)
        yb, _ = h(view, lengths, out_layout="bins")
        assert tuple(yb.shape) == (4, want.shape[2], want.shape[1]) and torch.equal(yb.transpose(1, 2), y)
        t = feats.transpose(1, 2).contiguous()  # [4, 24, F]: the bins layout; its view has F - 1 frames at a bin stride of F
        tv = t[..., :-1]
        assert tv.stride() == (F * bins, F, 1)
        with pkg.NewFrameStack(bins, *ps) as hb:
            got, got_len = hb(tv, [F - 1, 7, 0, 99], layout="bins", out_layout="frames")
            w2, w2_len = sr.host_values(sim, x[:, :-1], [F - 1, 7, 0, 99], ps)
            assert sr.same_bits(got.cpu().numpy(), w2) and np.array_equal(got_len.cpu().numpy(), w2_len)
        # leading dimensions, an out tensor, lengths on the device
        out = torch.full((2, 2) + want.shape[1:], 5.0, device="cuda:0")
        y2, len2 = h(view.reshape(2, 2, F, 23), torch.tensor(lengths, device="cuda:0").reshape(2, 2), out=out)
        assert y2 is out and torch.equal(out.reshape(y.shape), y) and tuple(len2.shape) == (2, 2)
        for bad in (view.double(), feats, view.cpu().numpy()):
            with pytest.raises(ValueError):
                h(bad)
        with pytest.raises(ValueError):
            h(view, [1, 2, 3])
        with pytest.raises(ValueError):
            h(view, out=torch.zeros(4, 3, 3, device="cuda:0"))
    # in place is refused: the output of a plain copy has the input's shape
    with pkg.NewFrameStack(bins) as c:
        with pytest.raises(ValueError):
            c(feats, out=feats)
        same, _ = c(feats)
        assert torch.equal(same, feats)
    # the functional entries against the handle
    before = set(pkg._STACKS)
    a, a_len = pkg.stack_frames(view, lengths, order=2, window=2, left=1, right=2, stride=3)
    assert torch.equal(a, y) and torch.equal(a_len, out_len) and len(set(pkg._STACKS) - before) == 1
    pkg.stack_frames(view, lengths, order=2, window=2, left=1, right=2, stride=3)
    assert len(set(pkg._STACKS) - before) == 1
    with pkg.NewFrameStack(bins, 2, 2) as h:
        want, want_len = h(feats, lengths)
    got, got_len = pkg.add_deltas(feats, lengths)
    assert tuple(got.shape) == (4, F, 3 * bins) and torch.equal(got, want) and got_len.cpu().tolist() == [F, 7, 0, 99]
    with pkg.NewFrameStack(bins, 0, 2, 3, 3, 6) as h:
        want, want_len = h(feats, lengths)
    got, got_len = pkg.lfr(feats, lengths)
    assert tuple(got.shape) == (4, 26, 7 * bins) and torch.equal(got, want) and got_len.cpu().tolist() == [26, 2, 0, 17]
    with pkg.NewFrameStack(bins, 0, 2, 1, 2, 4, -1.0) as h:
        want, _ = h(feats, lengths)
    got, _ = pkg.lfr(feats, lengths, m=4, n=4, pad_value=-1.0)
    assert torch.equal(got, want) and float(got[2].max()) == -1.0
    # a CPU tensor is uploaded; order 1 is compute_deltas' replicate mode on a full row, to float32 rounding
    d1, _ = pkg.add_deltas(torch.from_numpy(x), order=1, window=2)
    pad = torch.nn.functional.pad(feats.transpose(1, 2), (2, 2), mode="replicate")
    kern = torch.arange(-2, 3, dtype=torch.float32, device="cuda:0").repeat(bins, 1, 1)
    ref = (torch.nn.functional.conv1d(pad, kern, groups=bins) / 10.0).transpose(1, 2)
    assert d1.is_cuda and float((d1[..., bins:] - ref).abs().max()) < 1e-5 and torch.equal(d1[..., :bins], feats)


# ---- 3. raggedness, end to end -------------------------------------------------------------------------------------------
def test_load_features_with_deltas_context_and_subsampling(torch, pkg, tmp_path):
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
    F = 1 + (L - 400) // 160
    n_frames = flen.cpu().tolist()
    assert tuple(base.shape) == (3, F, 23) and n_frames[0] == n_frames[1] == F and 1 < n_frames[2] < F
    # the defaults run the chain as it was: byte for byte normalize_features of the same steps
    clips, lengths, _ = pkg.load_clips(paths, offsets, L, sample_rate=16000)
    counts = pkg.kaldi_frame_counts(lengths, 400, 160)
    chain = pkg.normalize_features(pkg.kaldi_fbank(clips[:, 0], sample_frequency=16000, **kw), counts, stat="mean")
    assert torch.equal(base.view(torch.int32), chain.view(torch.int32)) and torch.equal(flen.cpu(), counts.cpu())
    for args, ps in ((dict(deltas=2), (2, 2, 0, 0, 1)), (dict(context=(3, 3), subsample=6), (0, 2, 3, 3, 6)),
                     (dict(deltas=1, delta_window=3, context=(1, 0), subsample=2), (1, 3, 1, 0, 2))):
        feats, out_len, _ = pkg.load_features(paths, offsets, L, sample_rate=16000, **args, **kw)
        G, D = -(-F // ps[4]), sr.columns_of(ps, 23)
        assert tuple(feats.shape) == (3, G, D) and out_len.dtype is torch.int32
        with pkg.NewFrameStack(23, *ps) as h:
            for j in range(3):
                n = n_frames[j]
                want, m = h(base[j:j + 1, :n].contiguous())  # the clip cut to its own frame count
                m = int(m[0])
                assert m == -(-n // ps[4]) == int(out_len[j]) and tuple(want.shape) == (1, m, D)
                assert torch.equal(feats[j, :m].view(torch.int32), want[0].view(torch.int32)), "row %d, %r" % (j, args)
                assert not bool(feats[j, m:].view(torch.int32).any()), "the frames behind row %d's are not +0.0" % j


# ---- 4. the handle -------------------------------------------------------------------------------------------------------
def test_lifecycle_and_the_cpp_mirror(torch, pkg, sim):
    rng = np.random.default_rng(9)
    x = sr.features(rng, 3, 70, 23)
    d_x = to_dev(torch, x)
    h = pkg.NewFrameStack(23, 1, 2, 1, 1, 2)
    with pytest.raises(ValueError):
        h.last_ms()  # no pass yet on this handle
    h.stack_device(0, (1, 1, 1), 0, 70, 0, 0, (1, 1, 1))
    h.stack_device(0, (1, 1, 1), 3, 0, 0, 0, (1, 1, 1))
    with pytest.raises(ValueError):
        h.last_ms()  # nothing was launched
    d_y = torch.zeros(3, 35, 138, device="cuda:0")
    good_in, good_out = (70 * 23, 23, 1), (35 * 138, 138, 1)
    for bad_in, bad_out in (((70 * 23, 23, 2), good_out), (good_in, (35 * 138, 137, 1)), ((70 * 23 - 1, 23, 1), good_out),
                            (good_in, (35 * 138 - 1, 138, 1))):
        with pytest.raises(ValueError):
            h.stack_device(d_x.data_ptr(), bad_in, 3, 70, 0, d_y.data_ptr(), bad_out)
    for ptr_in, ptr_out in ((0, d_y.data_ptr()), (d_x.data_ptr(), 0), (d_x.data_ptr() + 2, d_y.data_ptr()),
                            (d_x.data_ptr(), d_x.data_ptr()), (d_x.data_ptr(), d_x.data_ptr() + 4 * (3 * 70 * 23 - 1))):
        with pytest.raises(ValueError):
            h.stack_device(ptr_in, good_in, 3, 70, 0, ptr_out, good_out)
    with pytest.raises(ValueError):
        h.last_ms()
    assert not bool(d_y.any()) and h.out_frames(70) == 35 and h.out_frames(71) == 36 and h.out_frames(0) == 0
    pl = h.plan()
    assert (pl["bins"], pl["order"], pl["window"], pl["left"], pl["right"], pl["stride"], pl["columns"]) == (23, 1, 2, 1, 1, 2, 138)
    assert sr.same_bits(pl["w1"], sr.weights(1, 2)[0]) and pl["w2"] is None
    y, out_len = h(d_x, [70, 0, 33])
    want, want_len = sr.host_values(sim, x, [70, 0, 33], (1, 2, 1, 1, 2))
    assert sr.same_bits(y.cpu().numpy(), want) and np.array_equal(out_len.cpu().numpy(), want_len) and h.last_ms() > 0
    h.synchronize()
    h.close()
    h.close()
    assert h.out_frames(70) == 0
    for call in (h.synchronize, h.last_ms, h.plan, lambda: h(d_x)):
        with pytest.raises(ValueError):
            call()
    # host/frame_stack.hpp through the ctypes shim
    S = sr.build_stack_shim(pkg)
    cfg = pkg.StackConfig(23, 1, 2, 1, 1, 2, -1.0)
    want, want_len = sr.host_values(sim, x, [70, 0, 33], (1, 2, 1, 1, 2), pad=-1.0)
    d_len, d_olen = to_dev(torch, np.asarray([70, 0, 33], np.int32)), torch.zeros(3, dtype=torch.int32, device="cuda:0")
    of, info, sizes, ms = ctypes.c_uint64(), np.zeros(13, np.uint32), np.zeros(2, np.uint64), ctypes.c_float()
    torch.cuda.synchronize()

    def run(strides):
        st = np.asarray(strides, np.uint64)
        return S.stack_shim_run(ctypes.byref(cfg), d_x.data_ptr(), st.ctypes.data, 3, 70, d_len.data_ptr(), d_y.data_ptr(),
                                d_olen.data_ptr(), ctypes.byref(of), info.ctypes.data, sizes.ctypes.data, ctypes.byref(ms))

    assert run(good_in + good_out) == 0, S.stack_shim_last_error()
    p = sr.plan_of((1, 2, 1, 1, 2), 23)
    assert of.value == 35 and sizes.tolist() == [5, 0] and ms.value > 0
    assert info.tolist() == [23, 1, 2, 1, 1, 2, 138, p["tile_out"], p["tile_in"], 23, p["lds_bytes"], 5, 0]
    assert sr.same_bits(d_y.cpu().numpy(), want) and np.array_equal(d_olen.cpu().numpy(), want_len)
    assert run(good_in + (35 * 138, 137, 1)) == -6 and b"stride" in S.stack_shim_last_error()


# ---- 5. far rows ---------------------------------------------------------------------------------------------------------
def test_rows_more_than_4_gi_elements_apart(torch, pkg, sim):
    """Two rows whose row stride is 2^32 + 12 345 elements, in the input and in the output, each in one allocation of 16 GiB that
    is touched only around the rows: a row offset narrowed to 32 bits would read and write row 1 at element 12 345, which holds
    canaries"""
    bins, ps = 23, (2, 2, 1, 1, 2)
    frames = sr.plan_of(ps, bins)["tile_in"] + 1
    G, D = -(-frames // 2), sr.columns_of(ps, bins)
    rs, guard = (1 << 32) + 12345, 4096
    ext_in, ext_out = frames * bins, G * D
    try:
        big_in = torch.empty(rs + ext_in + guard, dtype=torch.float32, device="cuda:0")
        big_out = torch.empty(rs + ext_out + guard, dtype=torch.float32, device="cuda:0")
    except RuntimeError as e:
        pytest.skip("no two allocations of %.1f GiB: %s" % ((rs + ext_out + guard) * 4 / 2.0 ** 30, str(e).splitlines()[0]))
    x = sr.features(np.random.default_rng(4), 2, frames, bins)
    lengths = [frames - 3, frames]
    for big, ext in ((big_in, ext_in), (big_out, ext_out)):
        big[:12345 + ext + guard] = float(CANARY)
        big[rs - guard:rs + ext + guard] = float(CANARY)
    big_in[:ext_in] = to_dev(torch, x[0].reshape(-1))
    big_in[rs:rs + ext_in] = to_dev(torch, x[1].reshape(-1))
    rows_in = torch.as_strided(big_in, (2, frames, bins), (rs, bins, 1))
    rows_out = torch.as_strided(big_out, (2, G, D), (rs, D, 1))
    with new_stack(pkg, ps, bins, pad=-2.0) as h:
        out, out_len = h(rows_in, lengths, out=rows_out)
    assert out is rows_out
    want, want_len = sr.host_values(sim, x, lengths, ps, pad=-2.0)
    got = np.stack([big_out[:ext_out].cpu().numpy(), big_out[rs:rs + ext_out].cpu().numpy()]).reshape(2, G, D)
    assert sr.same_bits(got, want) and np.array_equal(out_len.cpu().numpy(), want_len)
    for a, b in ((ext_out, 12345 + ext_out + guard), (rs - guard, rs), (rs + ext_out, rs + ext_out + guard)):
        assert bool((big_out[a:b] == float(CANARY)).all()), "an element outside the two rows was written"
    del big_in, big_out, rows_in, rows_out, out
    torch.cuda.empty_cache()
