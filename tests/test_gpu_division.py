"""The kernels' short division sequences (hippt_trace.h div_core, div_rn, avg_div) against hipcc's
IEEE a / b on the GPU (tests/native/div_selftest.hip, which includes the production header).

The combine's running average and every image bit that follows from it rest on these counts being zero; the
oracle keeps plain division.

* The running average's shape is exhaustive in the numerator: all 2^32 bit patterns of a (both zeros, denormals,
  infinities, NaNs) against fc = float(n) for n = 1..128 and 2^k - 1, 2^k, 2^k + 1 for k = 8..31 as float(int)
  rounds them, about 8.6e11 pairs.  The combine's rule (the sequence, or a / fc where a guard fires) equals a / fc
  bit for bit everywhere; the bare sequence equals it on its stated domain, -0 included.
* The general shape: 2^32 hashed pairs over all exponents; every divisor mantissa at three exponents against 64
  numerator mantissas; every pair of biased exponents with eight mantissa pairs and four sign pairs.  div_rn equals
  a / b everywhere and div_core on its domain (counted on its own).
"""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "native", "libdiv_selftest.so")
N_COUNTS = 32


def test_selftest_library_builds():
    assert os.path.exists(LIB), "build() / make -C tests/native -f div.mk builds it"


@pytest.mark.gpu
def test_running_average_every_numerator():
    lib = ctypes.CDLL(LIB)
    counts = (ctypes.c_ulonglong * N_COUNTS)()
    assert lib.div_selftest_average(counts) == 0
    rule, bare, nan_lost, nan_bits, in_domain = list(counts)[:5]
    print(f"average: rule {rule} bare-in-domain {bare} NaN-lost {nan_lost} NaN-other-bits {nan_bits} in-domain {in_domain}")
    assert in_domain > 200 * 2 ** 31  # the domain is most of the floats: the count is not vacuous
    assert (rule, bare, nan_lost) == (0, 0, 0)


@pytest.mark.gpu
def test_general_pairs():
    lib = ctypes.CDLL(LIB)
    counts = (ctypes.c_ulonglong * N_COUNTS)()
    assert lib.div_selftest_general(counts) == 0
    for s, (name, least) in enumerate([("hashed", 2 ** 31), ("grid", 2 ** 29), ("exponents", 2 ** 20)]):
        div_rn, core, _, in_domain = list(counts)[8 + 4 * s: 12 + 4 * s]
        print(f"{name}: div_rn {div_rn} div_core-in-domain {core} in-domain {in_domain}")
        assert in_domain > least, name
        assert (div_rn, core) == (0, 0), name
