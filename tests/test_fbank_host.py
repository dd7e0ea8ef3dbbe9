"""The Kaldi feature pass on the CPU: the plan of csrc/alac_fbank.h and the host build of its tile phases
(tests/host_sim/fbank_sim.cpp: g++, contraction off, work item for work item) against the step-by-step float64 restatement of
tests/kaldi_ref.py, which does not fold anything and so tests the folding.

    * the plan's tables within one float32 ulp of the restatement's (folded basis, mel weights, DCT, lifter), zeros exactly +0.0
    * the frame counts of both modes
    * whole sentinel-filled buffers at every base offset, odd strides, a frame stride above cols; rows 1 and 3
    * unlogged values within the derived ceilings (kr.prelog_bounds); logged values and MFCC against the float64 ln (and DCT) of
      the build's own unlogged values
    * impulses bit for bit from the tables alone; the refusals
    * where use_energy and htk_compat put the columns, and sqrt(2) C0, from the build's own outputs alone (kr.check_arrangement)
    * zeros, denormals, huge values, -0.0, an infinity and a NaN; silence through MFCC; a constant row"""
import numpy as np
import pytest

from tests import kaldi_ref as kr
from tests import mel_ref as mr


@pytest.fixture(scope="module")
def sim():
    return kr.build_fbank_sim()


def ulps_or_noise(got32, want64, scale):
    """|got - want| <= one float32 ulp of want, or, for an entry that is what is left of terms of size (1 + 2 c) scale cancelling in
    double, a few of their double roundings: 2^-48 scale"""
    err = np.abs(got32.astype(np.float64) - want64)
    return err <= kr.spacing32(want64) + 2.0 ** -48 * abs(scale)


@pytest.mark.parametrize("name", list(kr.CASES))
def test_plan_is_the_restatement_rounded(sim, name):
    cfg, tf = kr.CASES[name]
    pl = kr.sim_plan(sim, cfg)
    rule_tf, rule_floats = kr.lds_rule(cfg)
    assert pl["tile_frames"] == tf == rule_tf and pl["lds_bytes"] == 4 * rule_floats <= 65536
    assert (pl["frame_length"], pl["frame_shift"], pl["n_fft"], pl["n_freqs"]) == (cfg.W, cfg.h, cfg.N, cfg.K)
    assert (pl["num_mel_bins"], pl["num_ceps"], pl["cols"]) == (cfg.mels, cfg.ceps, cfg.cols)
    assert ulps_or_noise(pl["basis"], kr.folded(cfg), cfg.scale).all()
    fb64 = kr.mel_banks(cfg)
    dense = kr.dense_fb(pl)
    assert (np.abs(dense.astype(np.float64) - fb64) <= kr.spacing32(fb64)).all()
    assert (dense.view(np.uint32)[fb64 == 0.0] == 0).all(), "a weight outside its triangle is not +0.0"
    assert (dense[:, cfg.N // 2:] == 0).all(), "the bins from N / 2 on have no weight"
    first, taps = pl["first"], pl["taps"]
    assert taps >= 1 and (first >= 0).all() and (first + taps <= cfg.K).all()
    if cfg.ceps:
        assert (np.abs(pl["dct"].astype(np.float64) - kr.dct_matrix(cfg)) <= kr.spacing32(kr.dct_matrix(cfg)) + 2.0 ** -52).all()
        assert (np.abs(pl["lifter"].astype(np.float64) - kr.lifter(cfg)) <= kr.spacing32(kr.lifter(cfg))).all()


def test_window_zeros_are_plus_zero(sim):
    """Without pre-emphasis and DC removal an entry is win[n] cos / sin: the Hanning and Blackman end points and every sin at k = 0
    are zero, and +0.0f, never the -0.0f a negative factor would make of them"""
    for window in ("hanning", "blackman", "povey"):
        cfg = kr.W10.with_(window=window, pre=0.0, dc=False)
        b = kr.sim_plan(sim, cfg)["basis"]
        zero = kr.folded(cfg) == 0.0
        assert zero[:, :, 0].all() and zero[1, 0].all()
        assert (b.view(np.uint32)[zero] == 0).all() and not (b.view(np.uint32) == 0x80000000).any()
    assert np.array_equal(kr.sim_plan(sim, kr.Cfg(8000, 1, 1, pre=0.0, dc=False))["basis"][0], np.ones((1, 1), np.float32))  # W = 1 is [1.0]


def test_folding_agrees_with_the_steps_in_float64():
    """The restatement's own two forms: step by step and folded, 1.5e-15 of the largest bin apart at most"""
    rng = np.random.default_rng(5)
    for (W, h), offset in (((400, 160), 0.0), ((10, 4), 0.3), ((1200, 480), 0.3)):
        cfg = kr.Cfg(48000, W, h)
        x = kr.signal(rng, 2, W + 3 * h, offset)
        p, _ = kr.stepwise(cfg, x)
        Fd, fr = kr.folded(cfg), kr.raw_frames(cfg, x)
        q = np.einsum("kn,rfn->rfk", Fd[0], fr) ** 2 + np.einsum("kn,rfn->rfk", Fd[1], fr) ** 2
        assert np.abs(p - q).max() <= 1.5e-15 * p.max()


@pytest.mark.parametrize("snip", [True, False])
def test_frame_counts(sim, snip):
    for W, h in ((10, 4), (9, 5), (16, 37), (400, 160)):
        cfg = kr.Cfg(16000, W, h, snip=snip)
        for T in (W, W + h - 1, W + h, 8 * h * (1 + W // (8 * h)), W - 1, 0):
            want = 0 if T < W else (1 + (T - W) // h if snip else (T + h // 2) // h)
            assert kr.sim_out_frames(sim, cfg, T) == want == kr.out_frames(cfg, T)
            if want:
                kr.frame_index(cfg, T)  # asserts that one reflection brings every index into [0, T)
    assert kr.sim_out_frames(sim, kr.Cfg(16000, 10, 4, snip=snip), 10) == (1 if snip else 3)
    assert kr.sim_out_frames(sim, kr.Cfg(16000, 10, 4, snip=snip), 14) == (2 if snip else 4)


def test_refusals(sim):
    ok = kr.W10
    assert kr.sim_plan(sim, ok) is not None
    for kw in (dict(dither=1.0), dict(vtln=1.1), dict(use_power=0)):
        assert kr.sim_plan(sim, ok, **kw) is None
    assert kr.sim_plan(sim, ok.with_(energy=True), raw_energy=0) is None
    assert kr.sim_plan(sim, ok, raw_energy=0) is not None  # raw_energy is only read with use_energy
    for bad in (ok.with_(W=0), ok.with_(W=2049), ok.with_(W=1025, pow2=True).with_(W=2049), ok.with_(h=0), ok.with_(rate=0),
                ok.with_(mels=0), ok.with_(mels=4097), ok.with_(ceps=24), ok.with_(low=4000.0), ok.with_(low=-1.0),
                ok.with_(high=4001.0), ok.with_(high=-4000.0), ok.with_(low=3000.0, high=2000.0), ok.with_(scale=0.0),
                ok.with_(scale=float("nan")), ok.with_(efloor=-1.0), ok.with_(pre=float("inf"))):
        assert kr.sim_plan(sim, bad) is None
    assert kr.sim_plan(sim, ok.with_(W=2048, h=2048, pow2=False)) is not None
    assert kr.sim_plan(sim, ok.with_(W=1025, h=2048))["n_fft"] == 2048
    assert kr.lds_rule(kr.NO_LDS) == (4, 16516) and kr.sim_plan(sim, kr.NO_LDS) is None  # four frames do not fit LDS
    assert kr.sim_plan(sim, kr.NO_LDS.with_(ceps=2015))["lds_bytes"] == 65536  # and the largest that does
    # what the entry refuses: strides below what they span, misaligned or NULL buffers
    x = mr.aligned(64, 0)
    out = mr.aligned(4096, 0)
    w, d = ok.words()
    F = kr.out_frames(ok, 30)

    def run(in_stride, row_stride, inner, in_ptr=x.ctypes.data, out_ptr=out.ctypes.data, rows=2):
        return sim.fbank_sim_run(w.ctypes.data, d.ctypes.data, in_ptr, in_stride, rows, 30, out_ptr, row_stride, inner, 0)

    assert run(30, F * 23, 23) == 0
    assert run(29, F * 23, 23) == -2 and run(30, F * 23 - 1, 23) == -2 and run(30, F * 23, 22) == -2
    assert run(30, F * 23, 23, in_ptr=x.ctypes.data + 2) == -2 and run(30, F * 23, 23, out_ptr=None) == -2
    assert run(30, 0, 0, rows=0) == 0
    wb, db = ok.with_(layout="bins").words()
    assert sim.fbank_sim_run(wb.ctypes.data, db.ctypes.data, x.ctypes.data, 30, 2, 30, out.ctypes.data, 23 * F, F - 1, 0) == -2
    assert sim.fbank_sim_run(wb.ctypes.data, db.ctypes.data, x.ctypes.data, 30, 2, 30, out.ctypes.data, 23 * F, F, 0) == 0


@pytest.mark.parametrize("name", list(kr.CASES))
def test_host_build_against_the_restatement(sim, name):
    """Every case at F = tile_frames - 1, tile_frames, tile_frames + 1 and 1, rows 1 and 3 (a row on a DC offset of 0.3 among
    them): the unlogged pass within the ceilings; the case's own pass, logs, DCT and all, against the float64 of the build's own
    unlogged values; whole buffers at the four offset pairs, the last three with a frame stride of cols + 3; one run per case over
    an input that ends at an inaccessible page."""
    cfg, tf = kr.CASES[name]
    small = name in kr.SMALL
    rng = np.random.default_rng(len(name) + cfg.W)
    pre_cfg = cfg.prelog()
    plan = kr.sim_plan(sim, pre_cfg)
    worst = worst_log = 0.0
    for k, T in enumerate(kr.case_lengths(cfg, tf)):
        for rows in (1, 3) if small or k == 2 else (1,):
            x = kr.signal(rng, rows, T, 0.3 if rows == 3 else 0.0)
            what = "%s rows %d T %d" % (name, rows, T)
            img, lay = kr.sim_image(sim, pre_cfg, x, guard=1 if k == 2 else 0)
            pre = kr.values_of(img, lay, pre_cfg, rows, T, what)
            ref, lim = kr.prelog_bounds(pre_cfg, plan, x)
            worst = max(worst, kr.assert_within(pre, ref, lim, what))
            img, lay = kr.sim_image(sim, cfg, x)
            got = kr.values_of(img, lay, cfg, rows, T, what)
            worst_log = max(worst_log, kr.check_logged(cfg, got, pre, what))
            if name == "e_scale" and rows == 3:  # its floor lies between the energies of the signal's rows
                assert (pre[..., 0] > cfg.efloor).any() and (pre[..., 0] < cfg.efloor).any() and (pre[..., 0] > kr.EPS).all()
            for j, (out_off, in_off) in enumerate(kr.OFFSETS[1:] if small else kr.OFFSETS[1:2]):
                img, lay = kr.sim_image(sim, cfg, x, in_off, out_off, 3)
                assert np.array_equal(img, kr.image_of(cfg, got, img.size, lay)), "%s offsets %d/%d" % (what, in_off, out_off)
    print("%s: largest error / ceiling %.3f unlogged, %.3f logged" % (name, worst, worst_log))
    assert 0 < worst <= 1


@pytest.mark.parametrize("name", ["w10", "ns9", "h37ns", "e_last_1", "mfcc_e_htk", "asr", "mfcc_htk", "mfcc_c1", "mfcc_many", "m2e",
                                  "e_many_first"])
def test_layout_bins_is_the_transpose(sim, name):
    cfg, tf = kr.CASES[name]
    rng = np.random.default_rng(11)
    x = kr.signal(rng, 3, kr.length_for(cfg, tf + 1))
    want = kr.host_values(sim, cfg, x)
    bins = cfg.with_(layout="bins")
    for k, (out_off, in_off) in enumerate(kr.OFFSETS):
        img, lay = kr.sim_image(sim, bins, x, in_off, out_off, 3 if k else 0)
        assert np.array_equal(img, kr.image_of(bins, want, img.size, lay)), "%s offsets %d/%d" % (name, in_off, out_off)


@pytest.mark.parametrize("name", kr.IMPULSE_CASES)
def test_impulses_are_table_entries(sim, name):
    """remove_dc_offset off, nothing logged: row r is +0.0 with 1.0 at j0 + r, for every position of the first 3 W and the last 2 W
    samples; the whole buffer bit for bit what the tables under the impulse give"""
    cfg, T, js = kr.impulse_batch(name)
    plan = kr.sim_plan(sim, cfg)
    x = np.zeros((len(js), T), np.float32)
    x[np.arange(len(js)), js] = 1.0
    want, twice = zip(*(kr.impulse_expected(cfg, plan, T, j) for j in js))
    want = np.stack(want)
    img, lay = kr.sim_image(sim, cfg, x, 1, 3, 3)
    assert np.array_equal(img, kr.image_of(cfg, want, img.size, lay))
    assert want.any() and (cfg.snip or sum(twice) > 0), "no frame saw its impulse twice through the reflection"


def test_column_arrangement(sim):
    """kr.check_arrangement on the host build: the place of every column and the factor of C0 under htk_compat, without the
    restatement"""
    share = kr.check_arrangement(lambda cfg, x: kr.host_values(sim, cfg, x))
    print("sqrt(2) C0: largest error / bound %.3f" % share)


@pytest.mark.parametrize("name", kr.SPECIAL_CASES)
def test_other_float_values(sim, name):
    """mr.special_rows through the host build. Unlogged: rows 0 and 3 (zeros; a signal with -0.0) within the ceilings of the
    restatement, the denormal row below the normal range (its powers underflow, which the ceilings do not model), and
    kr.check_special_unlogged; the case's own logging pass over the same rows: kr.check_special_logged"""
    cfg, T, x = kr.special_input(name)
    pre_cfg = cfg.prelog()
    P = kr.host_values(sim, pre_cfg, x)
    kr.check_special_unlogged(pre_cfg, T, x, P)
    ref, lim = kr.prelog_bounds(pre_cfg, kr.sim_plan(sim, pre_cfg), x[[0, 3]])
    kr.assert_within(P[[0, 3]], ref, lim, name + " rows 0 and 3")
    assert (P[1] < 2.0 ** -126).all()
    got = kr.host_values(sim, cfg, x)
    share = kr.check_special_logged(cfg, got, P, name)
    if cfg.energy:
        floor = np.float32(0.0) if cfg.efloor > 0.0 else kr.LOG_EPS32
        assert cfg.efloor in (0.0, 1.0) and (got[0, :, 0].view(np.uint32) == floor.view(np.uint32)).all()
    print("%s: largest error / bound of the logs %.3f" % (name, share))


@pytest.mark.parametrize("name", ["mfcc13", "mfcc_e_htk", "mfcc_htk"])
def test_silence_through_mfcc(sim, name):
    print("%s: %.3f of the bound" % (name, kr.check_silence_mfcc(lambda cfg, x: kr.host_values(sim, cfg, x), name)))


def test_constant_row(sim):
    """What the folded mean removal leaves of a constant 0.5: within the ceilings; the figures are DESIGN.md §15's"""
    left = kr.check_constant(lambda cfg, x: kr.host_values(sim, cfg, x), lambda cfg: kr.sim_plan(sim, cfg))
    print("constant 0.5: largest mel value %s" % ", ".join("%.3g at scale %g" % (v, s) for s, v in left.items()))


def test_restatement_is_torchaudio():
    """Where torchaudio is installed: the restatement against kaldi.fbank / kaldi.mfcc within 1e-5 relative of the largest value,
    over snip_edges x use_energy x htk_compat, the five windows, remove_dc_offset off and round_to_power_of_two off"""
    kaldi = pytest.importorskip("torchaudio.compliance.kaldi")
    import torch
    rng = np.random.default_rng(3)
    x = kr.signal(rng, 1, 4000)
    base = kr.Cfg(16000, 400, 160, mels=40)
    sets = [base.with_(snip=snip, energy=energy, htk=htk) for snip in (True, False) for energy in (False, True) for htk in (False, True)]
    sets += [base.with_(window=w) for w in kr.WINDOWS] + [base.with_(window=w, htk=True, snip=False) for w in kr.WINDOWS]
    sets += [base.with_(dc=False), base.with_(dc=False, energy=True), base.with_(pow2=False), base.with_(pow2=False, htk=True)]
    for c in sets:
        kw = dict(num_mel_bins=40, snip_edges=c.snip, use_energy=c.energy, htk_compat=c.htk, window_type=c.window,
                  remove_dc_offset=c.dc, round_to_power_of_two=c.pow2, dither=0.0)
        for cfg, fn in ((c, kaldi.fbank), (c.with_(ceps=13), kaldi.mfcc)):
            want = fn(torch.from_numpy(x), **kw).double().numpy()
            got = kr.features64(cfg, x, kr.mel_banks(cfg))[0]
            assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), kw
