"""The consumption table of CLUSTER's sampling (csrc/sample_core.hpp) on the CPU: for every start s of a window, used(s) = the words of the random.Random(1524)
stream that random.sample(range(n), 100) consumes from s.  The backward sweep (k_sample_sweep; here its host build with plain loops over the 101 states,
svx_sample_used_host method 1) must give the table of the per-start walk (k_sample_tables, method 0) entry for entry, and both what CPython really consumes.
No GPU involved; tests/test_gpu_sample_sweep.py holds the kernels to the same tables through the clusters they lead to."""
import random

import numpy as np
import pytest

from svim_amd import _lib

C = 512                               # SAMPLE_SWEEP_C of csrc/sample_core.hpp (chunk = margin = 0 asks for the kernel's own C and M)
N_WORDS = 6000
SIZES = [101, 127, 128, 129, 255, 256, 257, 1045]      # 101: the bounds 101..2 cross every bit length from 7 to 2; k changes at or near the first draw; the largest pool size


@pytest.fixture(scope="module")
def words():
    _lib.build()
    r = random.Random(1524)
    return np.array([r.getrandbits(32) for _ in range(N_WORDS)], dtype=np.uint32)


def _cpython_used(n, s):
    """words random.sample(range(n), 100) consumes after s words of the stream have gone: found by what the generator hands out next"""
    r = random.Random(1524)
    for _ in range(s):
        r.getrandbits(32)
    r.sample(range(n), 100)
    return r.getrandbits(32)


def _check_window(words, n, lo, width, cap=None, **sweep):
    stream = words if cap is None else words[:cap]
    walk = _lib.sample_used_host(stream, n, lo, width, "walk")
    sweep_tab = _lib.sample_used_host(stream, n, lo, width, "sweep", **sweep)
    bad = np.nonzero(walk != sweep_tab)[0]
    assert bad.size == 0, (n, lo, width, sweep, int(bad[0]), int(walk[bad[0]]), int(sweep_tab[bad[0]]))
    return walk


@pytest.mark.parametrize("n", SIZES)
def test_sweep_equals_walk_equals_cpython(words, n):
    # a window at lo = 0 of C + 1 starts (the chunk seam), one of exactly one chunk, a narrow one further in
    for lo, width in ((0, C + 1), (300, C), (1777, 65)):
        tab = _check_window(words, n, lo, width)
        assert tab.max() < 0xffff and 100 <= tab.min()
        for s in sorted({0, 1, width // 2, C - 1 if width > C else width - 2, width - 1}):
            assert int(words[lo + s + int(tab[s])]) == _cpython_used(n, lo + s), (n, lo, s)


@pytest.mark.parametrize("n", SIZES)
def test_window_running_into_the_end_of_the_stream(words, n):
    """the last starts of the window cannot finish their 100 draws inside the stream: 0xffff from both methods, also where a whole chunk lies beyond the end"""
    lo, width = 900, 2 * C + 40
    for cap in (lo + width + 60, lo + C + 30, lo + 5):
        tab = _check_window(words, n, lo, width, cap=cap)
        assert tab[-1] == 0xffff and (tab == 0xffff).sum() >= 39            # a walk needs at least 100 words: the 39 starts with fewer than 100 left, at the least
        ok = np.nonzero(tab != 0xffff)[0]
        assert (cap > lo + 400) == (ok.size > 0)
        assert all(lo + s + int(tab[s]) <= cap for s in ok)


@pytest.mark.parametrize("n", SIZES)
def test_small_margin_goes_through_the_walk(words, n):
    """M = 8: only the first starts of a chunk see the end of their walk inside the swept words, the rest take the per-start walk - the same table; and other
    chunk lengths, among them one that is no multiple of 64"""
    _check_window(words, n, 0, C + 1, chunk=C, margin=8)
    _check_window(words, n, 411, 700, chunk=C, margin=8)
    _check_window(words, n, 411, 700, chunk=100, margin=150)
    _check_window(words, n, 5, 130, chunk=64, margin=0)


def test_arguments_are_checked(words):
    for n, lo, width in ((100, 0, 10), (1046, 0, 10), (200, -1, 10), (200, 0, 0)):
        with pytest.raises(_lib.SvxError):
            _lib.sample_used_host(words, n, lo, width, "walk")
    assert "svx_sample_used_host" in _lib.SYMBOLS
