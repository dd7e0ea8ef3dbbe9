"""The waveform augmentation pass on the CPU, second look: the paths of csrc/alac_waveaug.h that tests/test_waveaug_host.py's grid
does not value-check, host build (tests/host_sim/waveaug_sim.cpp) against the numpy restatement (tests/waveaug_ref.py) bit for
bit. tests/test_gpu_waveaug_paths.py runs the same cases on the MI355X against the host build.

* the apply kernel alone (no bank, no stats block: reduce == 0): its output and the draws it writes itself, over the five
  parameter sets and the eight sample counts; a bank without a stats block (the handle's own block behind the partials);
* rows of more than 256 chunks: the finish kernel's second and third block of partials, positions beyond 2^21;
* clips shorter than a chunk: the walk in steps of 256 mod m at m = 3, 5, 100, 255, 256, 300, 1000 and tile - 1;
* edge values inside the valid samples: subnormal squares and energies, an overflowing energy, NaN, +Inf, -0.0, +-1 and their
  neighbours, in the rows and in the bank. Where the expected value is a NaN the test asks for a NaN, everywhere else for the bits.
  Not tested, on purpose: an ordinary row under a clip of amplitude around 1e-20, where sqrt(Ex / En) overflows and the header
  yields b = +Inf by its own definition (wa.edge_cases)."""
import numpy as np
import pytest

from tests import waveaug_ref as wa
from tests.test_waveaug_host import run_over_buffers, sim  # noqa: F401 (sim is the module's fixture)

F32 = np.float32
SEED = wa.SEED
TILE = wa.TILE


def agree(got, want, what):
    assert wa.same_bits(got[0], want[0]), "output: " + what
    assert np.array_equal(got[1], want[1]), "draws: " + what
    assert got[2] is None or wa.same_bits(got[2], want[2]), "stats: " + what


# ---- 1. the apply kernel alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(wa.PARAMS))
def test_apply_alone_writes_output_and_draws(sim, name):
    """No bank and no stats block, so the partials and the finish kernel do not run: the output with b = 0, and the draws by
    put_draws out of the apply kernel's chunk 0, canaries around them. Then a bank without a stats block: the same draws and
    output as with one"""
    cfg, dither = wa.PARAMS[name]
    rng = np.random.default_rng(5000 + len(name))
    bank, bl = wa.waves(rng, 3, 5000, 0.1), [257, 5000, TILE + 1]
    k = 0
    for T in wa.SAMPLES:
        lengths = wa.lengths_of(T)
        x = wa.waves(rng, len(lengths), T)
        want = wa.reference(x, lengths, cfg, SEED, row_base=11, dither=dither, pad_value=-3.5)
        for in_place in (False, True):
            got = run_over_buffers(sim, x, lengths, cfg, dither, None, None, k, in_place, want_stats=False)
            agree(got, want, "T %d, case %d" % (T, k))
            bare = run_over_buffers(sim, x, lengths, cfg, dither, None, None, k, in_place, want_draws=False, want_stats=False)
            assert wa.same_bits(bare[0], want[0]) and bare[1] is None, "neither draws nor stats, T %d" % T
            k += 1
        own = run_over_buffers(sim, x, lengths, cfg, dither, bank, bl, k, k % 2 == 1, want_stats=False)
        kept = run_over_buffers(sim, x, lengths, cfg, dither, bank, bl, k, k % 2 == 1)
        assert wa.same_bits(own[0], kept[0]) and np.array_equal(own[1], kept[1]), "the handle's own stats block, T %d" % T
        if T in (257, 2 * TILE + 3):
            agree(own, wa.reference(x, lengths, cfg, SEED, bank, bl, row_base=11, dither=dither, pad_value=-3.5), "own stats, T %d" % T)
        k += 1


# ---- 2. long rows ------------------------------------------------------------------------------------------------------------
def test_rows_of_more_than_256_chunks(sim):
    """wa.long_rows_case: lengths of 256 tiles, one sample more, 257 tiles - 1, 512 tiles + 1 and 513 tiles + 5, so the finish
    kernel's loop ends after its first, second and third block; output, draws and stats bit for bit"""
    case = wa.long_rows_case()
    want = wa.reference(case["x"], case["lengths"], case["cfg"], SEED, case["bank"], case["bl"], **wa.case_kw(case))
    assert (want[1][[0, 1, 2, 4, 5], 0] == 1).all() and set(want[1][:, 1]) == {0, 1} and (want[2][[0, 1, 2, 4, 5], 3] != 0).all()
    got = wa.host_values(sim, case["x"], case["lengths"], case["cfg"], SEED, case["bank"], case["bl"], **wa.case_kw(case))
    agree(got, want, "long rows")


# ---- 3. clip lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", wa.CLIP_LENGTHS)
def test_clips_shorter_than_a_chunk(sim, m):
    case = wa.clip_case(m)
    x, lengths, cfg, bank, bl = (case[k] for k in ("x", "lengths", "cfg", "bank", "bl"))
    want = wa.reference(x, lengths, cfg, SEED, bank, bl, pad_value=-3.5, **wa.case_kw(case))
    assert (want[1][2:, 0] == 1).all() and (want[1][:, 2] < m).all() and (want[2][3:, 3] != 0).all()
    for k, in_place in ((m, False), (m + 1, True)):
        got = run_over_buffers(sim, x, lengths, cfg, case["dither"], bank, bl, k, in_place)
        agree(got, want, "m %d, in place %d" % (m, in_place))


# ---- 4. edge values inside the valid samples -----------------------------------------------------------------------------------
def b_is_zero_or_normal(stats):
    """The condition under which the GPU suite's relative tolerance on b means something; no b is infinite (the case left out)"""
    b = np.abs(stats[:, 3].astype(np.float64))
    return bool(((b == 0) | ((b >= 2.0 ** -126) & np.isfinite(b))).all())


@pytest.mark.parametrize("clamp", (0, 1))
def test_edge_values_inside_the_valid_samples(sim, clamp):
    cases, wants = wa.edge_cases(clamp), {}
    for name, case in cases.items():
        x, lengths, cfg, bank, bl = (case[k] for k in ("x", "lengths", "cfg", "bank", "bl"))
        want = wa.reference(x, lengths, cfg, SEED, bank, bl, **wa.case_kw(case))
        got = wa.host_values(sim, x, lengths, cfg, SEED, bank, bl, **wa.case_kw(case))
        wants[name] = want
        assert b_is_zero_or_normal(want[2]), name
        assert np.array_equal(got[1], want[1]) and (want[1][:, 0] == 1).all(), "draws: " + name
        assert wa.same_or_nan(got[2], want[2]), "stats: " + name
        assert wa.same_or_nan(got[0], want[0]), "output: " + name
        assert not np.isnan(want[2][:, 2:]).any(), "a and b are never NaN: " + name
    # the cases are what they claim to be
    y, _, st = wants["rows"]
    tiny = float(np.finfo(F32).tiny)
    assert st[0, 0] >= tiny and 0 < st[1, 0] < tiny and st[2, 0] == np.inf and np.isnan(st[3, 0]) and st[4, 0] == np.inf
    assert (st[:2, 3] > 0).all() and not st[2:5, 3].any() and st[5, 3] > 0
    assert np.isnan(y[3, 1234]) and np.isnan(y[3]).sum() == 1 and y[4, TILE + 4] == (1.0 if clamp else np.inf)
    assert (np.abs(y[2]).max() <= 1) == bool(clamp) and not np.isnan(y[[0, 1, 2, 4, 5]]).any()
    for name, ex in (("bank 3e19", np.inf), ("bank inf", np.inf), ("bank nan", np.nan)):
        st = wants[name][2]
        full = [r for r, n in enumerate(cases[name]["lengths"]) if n >= 700]  # those rows read every sample of the clip
        assert full and all(same_value(st[r, 1], ex) for r in full) and not st[full, 3].any(), name
    for scale in (1e-20, 1e-23):
        st = wants["tiny %g" % scale][2]
        assert (st[:, 1] > 0).all() and ((st[:, 1] < tiny).all() if scale < 1e-21 else (st[:, 1] >= tiny).all()), scale


def same_value(v, want):
    return bool(np.isnan(v)) if np.isnan(want) else bool(v == want)

