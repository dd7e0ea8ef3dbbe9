"""The launch plan's scan (saprobe-alac_amd/csrc/alac_plan.h: what the last block of a classify kernel runs, k_sort.hip)
built for the host (tests/host_sim/plan_sim.cpp) against a few lines of numpy: pkt_start, list_key, list_wave0, nk,
total_waves, irr_waves and wide_waves over all 2 050 keys (kKeys: 2 048 regular ones and the two irregular ones), for 16,
32 and 64 packets per wave, joined over 1, 64, 256 and (one position each, and more threads than positions) 2 050 and
4 096 runs."""
import ctypes

import numpy as np
import pytest

from tests import host_build

SENTINEL = 0xDEADBEEF
KEYS = 2050  # alac_plan.h: kKeys


@pytest.fixture(scope="module")
def sim():
    L = host_build.shared("plan_sim.cpp", "libplan_sim.so", host_build.SIM)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    for fn in (L.plan_sim_keys, L.plan_sim_key_wide, L.plan_sim_key_irregular):
        fn.restype, fn.argtypes = u32, []
    L.plan_sim_make.restype, L.plan_sim_make.argtypes = None, [vp, u32, u32, vp, vp, vp, vp, vp]
    return L


def numpy_plan(cnt, ppw, wide, irregular):
    """Dispatch order: highest key first. -> (pkt_start[keys], list_key, list_wave0, (nk, total, irr, wide waves))"""
    keys = len(cnt)
    order = np.arange(keys - 1, -1, -1)
    c = cnt[order].astype(np.int64)
    waves = (c + ppw - 1) // ppw
    start = np.zeros(keys, np.int64)
    start[order] = np.cumsum(c) - c
    present = c > 0
    wave0 = (np.cumsum(waves) - waves)[present]
    return (start, order[present], wave0,
            (int(present.sum()), int(waves.sum()), int(waves[order >= irregular].sum()),
             int(waves[(order >= wide) & (order < irregular)].sum())))


def check(L, cnt, ppw, threads):
    keys, wide, irr = L.plan_sim_keys(), L.plan_sim_key_wide(), L.plan_sim_key_irregular()
    assert len(cnt) == keys == KEYS and ppw & (ppw - 1) == 0
    cnt = np.ascontiguousarray(cnt, np.uint32)
    out = [np.full(keys, SENTINEL, np.uint32) for _ in range(4)]
    totals = np.full(4, SENTINEL, np.uint32)
    L.plan_sim_make(cnt.ctypes.data, ppw.bit_length() - 1, threads, *[a.ctypes.data for a in out], totals.ctypes.data)
    count, pkt_start, list_key, list_wave0 = out
    start, lk, lw, tot = numpy_plan(cnt, ppw, wide, irr)
    what = "ppw %d, %d threads" % (ppw, threads)
    assert np.array_equal(count, cnt), what
    assert np.array_equal(pkt_start, start), what
    nk = tot[0]
    assert tuple(int(x) for x in totals) == tot, what
    assert np.array_equal(list_key[:nk], lk) and np.array_equal(list_wave0[:nk], lw), what
    assert (list_key[nk:] == SENTINEL).all() and (list_wave0[nk:] == SENTINEL).all(), what  # nothing behind the list


THREADS = (1, 64, 256, KEYS, 4096)
PPW = (16, 32, 64)


@pytest.mark.parametrize("ppw", PPW)
def test_random_histograms_over_all_keys(sim, ppw):
    rng = np.random.default_rng(ppw)
    for density in (1.0, 0.3, 0.01):
        cnt = rng.integers(0, 5 * ppw, KEYS) * (rng.random(KEYS) < density)
        for threads in THREADS:
            check(sim, cnt, ppw, threads)
    cnt = np.zeros(KEYS, np.int64)  # a batch as the decoder sees them: a dozen keys, thousands of packets each
    cnt[rng.choice(KEYS, 12, replace=False)] = rng.integers(1, 20000, 12)
    for threads in THREADS:
        check(sim, cnt, ppw, threads)


@pytest.mark.parametrize("ppw", PPW)
def test_empty_histogram_and_single_keys_at_the_ends_of_the_range(sim, ppw):
    for threads in THREADS:
        check(sim, np.zeros(KEYS, np.int64), ppw, threads)
        for key in (0, 1, 1023, 1024, 2047, 2048, KEYS - 1):
            for c in (1, ppw, 3 * ppw + 1):
                cnt = np.zeros(KEYS, np.int64)
                cnt[key] = c
                check(sim, cnt, ppw, threads)


@pytest.mark.parametrize("ppw", PPW)
def test_counts_that_are_multiples_of_the_wave_and_one_more(sim, ppw):
    rng = np.random.default_rng(100 + ppw)
    for extra in (0, 1):
        cnt = rng.integers(0, 9, KEYS) * ppw
        cnt[cnt > 0] += extra
        cnt[[0, 2047, 2048, KEYS - 1]] = 7 * ppw + extra
        for threads in THREADS:
            check(sim, cnt, ppw, threads)
    cnt = np.full(KEYS, ppw - 1, np.int64)  # every key a partly filled wave; and every key ppw + 1
    for threads in THREADS:
        check(sim, cnt, ppw, threads)
        check(sim, cnt + 2, ppw, threads)
