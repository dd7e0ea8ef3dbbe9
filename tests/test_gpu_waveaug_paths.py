"""The waveform augmentation pass on the MI355X, second look: the paths of k_waveaug.hip that tests/test_gpu_waveaug.py's grid
never launches, held to the host build by that file's rule (hold_to_host: draws, Ex, En and a bit for bit, b within B_TOL, the
output bit for bit against the formula over the device's own stats). tests/test_waveaug_paths_host.py holds the host build to
numpy over the same cases (wa.long_rows_case, wa.clip_case, wa.edge_cases).

* the apply kernel alone, alac_waveaug_apply and alac_waveaug_apply_dither without the partials and the finish kernel: d_stats = 0
  and no bank, the draws written by the apply kernel, no growth of the scratch block; a bank with d_stats = 0 (the handle's
  own stats block); the same through WaveAugment.__call__ and augment_waveform;
* rows of up to 513 chunks: the finish kernel's second and third block, noise and dither positions beyond 2^21;
* clips of 3, 5, 100, 255, 256, 300, 1000 and tile - 1 samples under rows of two chunks and three samples;
* NaN, +Inf, overflowing and subnormal energies, -0.0, +-1 and their neighbours inside the valid samples, in rows and bank. Where
  the host build has a NaN the device must have one; everything else bit for bit. Not tested, on purpose: sqrt(Ex / En) = +Inf
  (wa.edge_cases);
* two clips 2^32 + 12 345 elements apart in the bank;
* the tensor interface: inputs that do not flatten, strided and host banks, ids of other types and places, a clip [T];
* three passes in flight on one handle (sync=False), the second of which grows the scratch block.

No test provokes a fault: every buffer has the size the entry asks for."""
import numpy as np
import pytest

from tests import waveaug_ref as wa
from tests.test_gpu_waveaug import CANARY, device_run, hold_to_host, new_waveaug, sim, to_dev, torch  # noqa: F401 (two fixtures)

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED = wa.SEED
TILE = wa.TILE


def of(case):
    return tuple(case[k] for k in ("x", "lengths", "cfg", "bank", "bl"))


# ---- 1. the apply kernel alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(wa.PARAMS))
def test_apply_alone_on_the_device(torch, pkg, sim, name):
    """No bank and d_stats = 0: one launch, alac_waveaug_apply for the sets without dither and alac_waveaug_apply_dither for
    "dither" and "all". b is 0 and a is a table entry, so the output is the host build's bit for bit, and so are the draws,
    which the apply kernel's chunk 0 writes. The scratch block stays as create left it. Then a bank with d_stats = 0: the
    handle's own stats block behind the partials gives the draws and the output of the pass with the caller's"""
    cfg, dither = wa.PARAMS[name]
    rng = np.random.default_rng(5000 + len(name))
    bank, bl = wa.waves(rng, 3, 5000, 0.1), [257, 5000, TILE + 1]
    k = 0
    with new_waveaug(pkg, cfg, dither, -3.5) as h:
        first = h.plan()
        for T in wa.SAMPLES:
            lengths = wa.lengths_of(T)
            x = wa.waves(rng, len(lengths), T)
            want = wa.host_values(sim, x, lengths, cfg, SEED, want_stats=False, row_base=11, dither=dither, pad_value=-3.5)
            for in_place in (False, True):
                y, draws, _ = device_run(torch, h, x, lengths, None, None, k, in_place, row_base=11, want_stats=False)
                assert np.array_equal(draws, want[1]) and wa.same_bits(y, want[0]), "T %d, case %d" % (T, k)
                y, _, _ = device_run(torch, h, x, lengths, None, None, k, in_place, row_base=11, want_draws=False, want_stats=False)
                assert wa.same_bits(y, want[0]), "neither draws nor stats, T %d, case %d" % (T, k)
                k += 1
        now = h.plan()
        assert (now["scratch_bytes"], now["scratch_address"]) == (first["scratch_bytes"], first["scratch_address"])
        for T in (257, 2 * TILE + 3):
            lengths = wa.lengths_of(T)
            x = wa.waves(rng, len(lengths), T)
            own = device_run(torch, h, x, lengths, bank, bl, k, k % 2 == 1, row_base=11, want_stats=False)
            kept = device_run(torch, h, x, lengths, bank, bl, k, k % 2 == 1, row_base=11)
            want = wa.host_values(sim, x, lengths, cfg, SEED, bank, bl, row_base=11, dither=dither, pad_value=-3.5)
            hold_to_host(kept, want, x, lengths, cfg, bank, bl, "caller's stats, T %d" % T, row_base=11, dither=dither, pad_value=-3.5)
            assert np.array_equal(own[1], kept[1]) and wa.same_bits(own[0], kept[0]), "the handle's own stats block, T %d" % T
            k += 1


def test_apply_alone_through_the_tensor_interface(torch, pkg, sim):
    rng = np.random.default_rng(31)
    T = TILE + 33
    x = wa.waves(rng, 5, T)
    lengths = [T, 0, 257, T - 1, 4096]
    d_x = to_dev(torch, x)
    cfg = (5 * 256, 20 * 256, -6 * 256, 3 * 256, 65536, 0)
    for dither in (0.0, 0.01):
        want = wa.host_values(sim, x, lengths, cfg, SEED, want_stats=False, row_base=7, dither=dither)
        with new_waveaug(pkg, cfg, dither, 0.0) as h:
            first = h.plan()
            y, draws = h(d_x, lengths, SEED, row_base=7, return_draws=True)
            assert (h.plan()["scratch_address"], h.plan()["scratch_bytes"]) == (first["scratch_address"], first["scratch_bytes"])
        assert wa.same_bits(y.cpu().numpy(), want[0]) and np.array_equal(draws.cpu().numpy(), want[1]), dither
        y, draws = pkg.augment_waveform(d_x, lengths, seed=SEED, gain=(-6, 3), dither=dither, row_base=7, return_draws=True)
        assert wa.same_bits(y.cpu().numpy(), want[0]) and np.array_equal(draws.cpu().numpy(), want[1]), dither
        only = pkg.augment_waveform(d_x, lengths, seed=SEED, gain=(-6, 3), dither=dither, row_base=7)
        assert torch.equal(only.view(torch.int32), y.view(torch.int32))
    assert not want[1][:, :3].any() and len(set(want[1][:, 4])) > 1


# ---- 2. long rows ------------------------------------------------------------------------------------------------------------
def test_rows_of_more_than_256_chunks(torch, pkg, sim):
    """wa.long_rows_case: alac_waveaug_finish adds the partials of a row 256 chunks at a time, and these rows end in its first,
    second and third block, one sample on either side of the edges. Prints whether b is the host build's"""
    case = wa.long_rows_case()
    x, lengths, cfg, bank, bl = of(case)
    want = wa.host_values(sim, x, lengths, cfg, SEED, bank, bl, **wa.case_kw(case))
    assert (want[2][[0, 1, 2, 4, 5], 3] != 0).all()
    with new_waveaug(pkg, cfg, case["dither"], 0.0) as h:
        got = device_run(torch, h, x, lengths, bank, bl, 1, False, row_base=case["row_base"])
    equal = hold_to_host(got, want, x, lengths, cfg, bank, bl, "long rows", host_output=True, **wa.case_kw(case))
    print("b equal to the host build's: %s" % equal)


# ---- 3. clip lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", wa.CLIP_LENGTHS)
def test_clips_shorter_than_a_chunk(torch, pkg, sim, m):
    case = wa.clip_case(m)
    x, lengths, cfg, bank, bl = of(case)
    want = wa.host_values(sim, x, lengths, cfg, SEED, bank, bl, pad_value=-3.5, **wa.case_kw(case))
    assert (want[2][3:, 3] != 0).all()
    equal = []
    with new_waveaug(pkg, cfg, case["dither"], -3.5) as h:
        for k, in_place in ((m, False), (m + 1, True)):
            got = device_run(torch, h, x, lengths, bank, bl, k, in_place, row_base=case["row_base"])
            equal.append(hold_to_host(got, want, x, lengths, cfg, bank, bl, "m %d, in place %d" % (m, in_place), pad_value=-3.5,
                                      **wa.case_kw(case)))
    print("b equal to the host build's in %d of %d passes" % (sum(equal), len(equal)))


# ---- 4. edge values inside the valid samples -----------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", (0, 1))
def test_edge_values_inside_the_valid_samples(torch, pkg, sim, clamp):
    """wa.edge_cases. The clamp is two comparisons, so a NaN sample stays a NaN (a min / max would return the bound); a NaN or
    infinite energy gives b = 0; energies built of subnormal squares are the host build's bit for bit, which a kernel that
    flushed subnormals would miss. tests/test_waveaug_paths_host.py asserts, from the reference alone, that every b here is 0 or
    a normal float, so B_TOL means what it says"""
    equal = []
    for k, (name, case) in enumerate(wa.edge_cases(clamp).items()):
        x, lengths, cfg, bank, bl = of(case)
        want = wa.host_values(sim, x, lengths, cfg, SEED, bank, bl, **wa.case_kw(case))
        with new_waveaug(pkg, cfg, case["dither"], 0.0) as h:
            got = device_run(torch, h, x, lengths, bank, bl, k, k % 2 == 1, row_base=case["row_base"])
        equal.append(hold_to_host(got, want, x, lengths, cfg, bank, bl, name, nan_ok=True, **wa.case_kw(case)))
        if name == "rows":
            y = got[0]
            assert np.isnan(y[3, 1234]) and np.isnan(y).sum() == 1 and y[4, TILE + 4] == (1.0 if clamp else np.inf)
            assert np.isnan(got[2][3, 0]) and got[2][2, 0] == np.inf and 0 < got[2][1, 0] < np.finfo(F32).tiny
    print("b equal to the host build's in %d of %d passes" % (sum(equal), len(equal)))


# ---- 5. a far bank -----------------------------------------------------------------------------------------------------------
def test_clips_more_than_4_gi_elements_apart(torch, pkg, sim):
    """Two clips whose stride is 2^32 + 12 345 elements, in one allocation of 16 GiB that is touched only around the clips: a clip
    offset narrowed to 32 bits would read clip 1 at element 12 345, which holds canaries, and En, b and the output would show it"""
    cfg, dither = (5 * 256, 20 * 256, -6 * 256, 3 * 256, 65536, 1), 0.01
    rs, guard, Tn, T = (1 << 32) + 12345, 4096, 3000, TILE + 1
    rng = np.random.default_rng(41)
    x = wa.waves(rng, 8, T)
    lengths = [T - 3, T, 257, T, 1, T - 1, 3000, T]
    bank, bl = wa.waves(rng, 2, Tn, 0.1), [Tn, 257]
    want = wa.host_values(sim, x, lengths, cfg, SEED, bank, bl, row_base=5, dither=dither, pad_value=-2.0)
    assert set(want[1][:, 1]) == {0, 1} and (want[2][:, 3] != 0).all(), "both clips are drawn, every row gets noise"
    try:
        big = torch.empty(rs + Tn + guard, dtype=torch.float32, device="cuda:0")
    except RuntimeError as e:
        pytest.skip("no allocation of %.1f GiB: %s" % ((rs + Tn + guard) * 4 / 2.0 ** 30, str(e).splitlines()[0]))
    big[:12345 + Tn + guard] = float(CANARY)
    big[rs - guard:rs + Tn + guard] = float(CANARY)
    big[:Tn] = to_dev(torch, bank[0])
    big[rs:rs + Tn] = to_dev(torch, bank[1])
    d_bank = torch.as_strided(big, (2, Tn), (rs, 1))
    before = (big[:12345 + Tn + guard].clone(), big[rs - guard:rs + Tn + guard].clone())
    with new_waveaug(pkg, cfg, dither, -2.0) as h:
        y, draws, stats = h(to_dev(torch, x), lengths, SEED, noise=d_bank, noise_lengths=bl, row_base=5, return_draws=True,
                            return_stats=True)
    hold_to_host((y.cpu().numpy(), draws.cpu().numpy(), stats.cpu().numpy()), want, x, lengths, cfg, bank, bl, "far bank", row_base=5,
                 dither=dither, pad_value=-2.0)
    assert torch.equal(big[:12345 + Tn + guard], before[0]) and torch.equal(big[rs - guard:rs + Tn + guard], before[1]), "the bank changed"
    del big, d_bank, before
    torch.cuda.empty_cache()


# ---- 6. the tensor interface -------------------------------------------------------------------------------------------------
def test_views_banks_ids_and_a_single_clip(torch, pkg, sim):
    rng = np.random.default_rng(51)
    B, C, L = 3, 2, TILE + 151
    clips = wa.waves(rng, B * C, 2 * L).reshape(B, C, 2 * L)
    lengths = [L, 700, 0, 4097, 1, L - 1]
    wide = wa.waves(rng, 3, 5000, 0.1)
    bl = [2500, 257, 1000]
    cfg, dither = (5 * 256, 20 * 256, -6 * 256, 3 * 256, 52429, 1), 0.01
    d_clips, d_wide = to_dev(torch, clips), to_dev(torch, wide)
    ret = dict(return_draws=True, return_stats=True)

    def same(a, b):
        return all(p.shape == q.shape and torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))

    with new_waveaug(pkg, cfg, dither, 0.0) as h:
        # inputs that do not flatten are copied: every other sample, and a transposed tensor; the input stays as it is
        half = d_clips[..., ::2]
        assert tuple(half.shape) == (B, C, L) and not half.is_contiguous()
        before = d_clips.clone()
        base = h(half.contiguous(), lengths, SEED, noise=d_wide, noise_lengths=bl, row_base=40, **ret)
        assert same(h(half, lengths, SEED, noise=d_wide, noise_lengths=bl, row_base=40, **ret), base) and torch.equal(d_clips, before)
        x = clips[..., ::2].reshape(B * C, L)
        want = wa.host_values(sim, x, lengths, cfg, SEED, wide, bl, row_base=40, dither=dither)
        hold_to_host(tuple(t.cpu().numpy().reshape(B * C, -1) for t in base), want, x, lengths, cfg, wide, bl, "every other sample",
                     row_base=40, dither=dither)
        assert tuple(base[0].shape) == (B, C, L) and tuple(base[1].shape) == (B, C, 5) and tuple(base[2].shape) == (B, C, 4)
        turned = to_dev(torch, np.ascontiguousarray(x.T)).t()
        assert tuple(turned.shape) == (B * C, L) and turned.stride() == (1, B * C)
        kept = turned.clone()
        got = h(turned, lengths, SEED, noise=d_wide, noise_lengths=bl, row_base=40, **ret)
        assert same(got, tuple(t.reshape(B * C, -1) for t in base)) and got[0].is_contiguous() and torch.equal(turned, kept)
        # the bank: every other sample (copied), a view on its own stride, a host tensor, a numpy array
        flat = half.contiguous().reshape(B * C, L)
        for view, dense in ((d_wide[:, ::2], wide[:, ::2]), (d_wide[:, :1000], wide[:, :1000])):
            over_copy = h(flat, lengths, SEED, noise=view.contiguous(), noise_lengths=bl, row_base=40, **ret)
            assert same(h(flat, lengths, SEED, noise=view, noise_lengths=bl, row_base=40, **ret), over_copy)
            assert same(h(flat, lengths, SEED, noise=torch.from_numpy(np.ascontiguousarray(dense)), noise_lengths=bl, row_base=40, **ret),
                        over_copy)
            assert same(h(flat, lengths, SEED, noise=dense, noise_lengths=torch.tensor(bl), row_base=40, **ret), over_copy)
            want = wa.host_values(sim, x, lengths, cfg, SEED, np.ascontiguousarray(dense), bl, row_base=40, dither=dither)
            hold_to_host(tuple(t.cpu().numpy() for t in over_copy), want, x, lengths, cfg, np.ascontiguousarray(dense), bl,
                         "bank of %d samples" % dense.shape[1], row_base=40, dither=dither)
            assert (want[1][:, 0] == 1).sum() >= 3 and (want[1][:, 2] > 0).any()
        # ids: an int32 tensor on the device, an int64 tensor on the host, against a list
        ids = [900, -5, 2 ** 31 - 1, 0, 77, 40]
        by_list = h(flat, lengths, SEED, noise=d_wide, noise_lengths=bl, ids=ids, **ret)
        want = wa.host_values(sim, x, lengths, cfg, SEED, wide, bl, ids=ids, dither=dither)
        hold_to_host(tuple(t.cpu().numpy() for t in by_list), want, x, lengths, cfg, wide, bl, "ids", ids=ids, dither=dither)
        assert same(h(flat, lengths, SEED, noise=d_wide, noise_lengths=bl, ids=torch.tensor(ids, dtype=torch.int32, device="cuda:0"), **ret),
                    by_list)
        assert same(h(flat, lengths, SEED, noise=d_wide, noise_lengths=bl, ids=torch.tensor(ids, dtype=torch.int64), **ret), by_list)
        # one clip [T]: the row of identity row_base; draws [5], stats [4]
        r = 3
        one = h(flat[r], lengths[r:r + 1], SEED, noise=d_wide, noise_lengths=bl, row_base=ids[r], **ret)
        assert tuple(one[0].shape) == (L,) and tuple(one[1].shape) == (5,) and tuple(one[2].shape) == (4,)
        assert same(one, tuple(t[r] for t in by_list))
        whole = h(flat[r], None, SEED, row_base=ids[r])
        assert tuple(whole.shape) == (L,) and wa.same_bits(whole.cpu().numpy()[None], wa.host_values(sim, x[r:r + 1], None, cfg, SEED,
                                                                                                     row_base=ids[r], dither=dither)[0])


# ---- 7. passes in flight -----------------------------------------------------------------------------------------------------
def test_three_passes_in_flight_on_one_handle(torch, pkg, sim):
    """Three waveaug_device(..., sync=False) calls and then one synchronize. The first pass (6 floats of partials) fits the block
    the handle is created with; the second (16 rows of 4 chunks, a bank, no stats block of the caller's: 128 + 64 floats) needs
    the block grown while the first may still run, which the entry answers by waiting for its stream first; the third is small
    and finds the grown block. Each pass has buffers of its own, so all three results can be held to the host build afterwards.
    The block, as (address, bytes), changes once: a larger block may get the address of the one just freed, its size tells"""
    cfg, dither = (5 * 256, 20 * 256, -6 * 256, 3 * 256, 65536, 1), 0.01
    rng = np.random.default_rng(61)
    bank, bl = wa.waves(rng, 2, 3000, 0.1), [3000, 257]
    d_bank, d_bl = to_dev(torch, bank), to_dev(torch, np.asarray(bl, np.int32))
    T2 = 3 * TILE + 9
    specs = [(wa.waves(rng, 3, 700), [700, 0, 333], True, True, 100),
             (wa.waves(rng, 16, T2), [T2, 1, 4096, 4097, 0, 3 * TILE, 9000, 257, T2 - 1, T2, 2 * TILE, 5, T2, 8193, 3 * TILE + 1, T2], True, False, 200),
             (wa.waves(rng, 2, 300), [300, 299], False, True, 300)]
    runs = []
    for x, lengths, banked, stats, row_base in specs:
        rows, T = x.shape
        runs.append(dict(d_x=to_dev(torch, x), d_len=to_dev(torch, np.asarray(lengths, np.int32)),
                         d_y=torch.full((rows * T + 8,), float(CANARY), dtype=torch.float32, device="cuda:0"),
                         d_draws=torch.full((rows + 1, 5), -77, dtype=torch.int32, device="cuda:0"),
                         d_stats=torch.full((rows + 1, 4), float(CANARY), dtype=torch.float32, device="cuda:0")))
    torch.cuda.synchronize()
    with new_waveaug(pkg, cfg, dither, -2.0) as h:
        blocks = [(h.plan()["scratch_address"], h.plan()["scratch_bytes"])]
        for (x, lengths, banked, stats, row_base), r in zip(specs, runs):
            rows, T = x.shape
            h.waveaug_device(r["d_x"].data_ptr(), T, rows, T, r["d_len"].data_ptr(), SEED, r["d_y"].data_ptr(), T,
                             d_bank.data_ptr() if banked else 0, 3000, 2 if banked else 0, 3000 if banked else 0,
                             d_bl.data_ptr() if banked else 0, row_base, 0, r["d_draws"].data_ptr(), r["d_stats"].data_ptr() if stats else 0,
                             sync=False)
            blocks.append((h.plan()["scratch_address"], h.plan()["scratch_bytes"]))
        h.synchronize()
        assert h.last_ms() > 0
    assert blocks[0] == blocks[1] and blocks[2] == blocks[3] and 4 * 6 <= blocks[0][1] < 4 * (128 + 64) <= blocks[2][1], blocks
    for k, ((x, lengths, banked, stats, row_base), r) in enumerate(zip(specs, runs)):
        rows, T = x.shape
        want = wa.host_values(sim, x, lengths, cfg, SEED, bank if banked else None, bl if banked else None, row_base=row_base,
                              dither=dither, pad_value=-2.0)
        y, draws, st = r["d_y"].cpu().numpy(), r["d_draws"].cpu().numpy(), r["d_stats"].cpu().numpy()
        assert (y[rows * T:] == CANARY).all() and (draws[rows] == -77).all() and (st[rows] == CANARY).all(), "pass %d wrote past its rows" % k
        y = y[:rows * T].reshape(rows, T)
        if stats:
            hold_to_host((y, draws[:rows], st[:rows]), want, x, lengths, cfg, bank if banked else None, bl if banked else None,
                         "pass %d" % k, row_base=row_base, dither=dither, pad_value=-2.0)
        else:  # its stats stayed in the handle's block: the same pass alone, synchronous and with a stats block, shows them
            with new_waveaug(pkg, cfg, dither, -2.0) as alone:
                again = tuple(t.cpu().numpy() for t in alone(r["d_x"], lengths, SEED, noise=d_bank, noise_lengths=bl, row_base=row_base,
                                                             return_draws=True, return_stats=True))
            hold_to_host(again, want, x, lengths, cfg, bank, bl, "pass %d alone" % k, row_base=row_base, dither=dither, pad_value=-2.0)
            assert (st == CANARY).all() and np.array_equal(draws[:rows], again[1]) and wa.same_bits(y, again[0]), "pass %d" % k
