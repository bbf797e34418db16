"""The two forms of svx_sort_pairs_u64 (csrc/prims.hip) around the size where one hands over to the other, on a real MI355X (`-m gpu`): the one-workgroup form
(every pass in one launch, passes over a constant digit skipped) up to RADIX_ONE = 16384 pairs, three launches per pass over tiles of 2048 beyond it.
svx_selftest_prims holds the result to std::stable_sort."""
import pytest

pytestmark = pytest.mark.gpu

RADIX_ONE = 16384                      # csrc/prims.hip
SIZES = (RADIX_ONE, RADIX_ONE + 1, 23001, 2 * RADIX_ONE, 2 * RADIX_ONE + 1)      # 23001: no multiple of the tile (2048)
RANGES = ((0, 64), (0, 37), (0, 3))


@pytest.fixture(scope="module")
def eng():
    from svim_amd import _lib
    e = _lib.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("n", SIZES)
def test_sort_forms_agree_with_stable_sort(eng, n):
    for b0, b1 in RANGES:
        eng.selftest_prims(n, b0, b1, seed=(n + b1) & ~0x100)       # wide and narrow keys mixed, many equal keys: ties keep their input order
    # keys & 0xffff00: the digits from bit 24 up are the same in every key, as the upper digits of the cluster keys are (and bits 0..7 too)
    eng.selftest_prims(n, 0, 64, seed=(n + 5) | 0x100)
    eng.selftest_prims(n, 8, 56, seed=(n + 7) | 0x100)
