"""The short division sequences on the host (DESIGN.md §5 "Exact division"): tests/native/div_model.cpp, a stand-alone
program that restates hippt_trace.h's div_core, div_rn and avg_div with fmaf and 1.0f / b (which rcp_nr
equals on its verified range) and compares them with the compiler's IEEE a / b: every divisor mantissa at three
exponents against 64 numerator mantissas, every pair of biased exponents (zeros, denormals, infinities and NaN
included) with eight mantissa pairs and four sign pairs, 10^7 hashed pairs, and the running average's divisors
against special and hashed numerators and the ties of the denormal quotients.  The guarded functions equal a / b
everywhere, the bare sequences on their stated domains.  A second build with AddressSanitizer and UBSan runs the
short sweeps.  No GPU, nothing loaded into Python; the GPU's own v_rcp_f32 is tests/test_gpu_division.py's affair.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "div_model.cpp")

needs_gpp = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _has_fma():
    try:
        return re.search(r"^flags\s*:.*\bfma\b", open("/proc/cpuinfo").read(), re.M) is not None
    except OSError:
        return False


def _build(exe, extra):
    # -mfma: fmaf as one instruction where the CPU has it (the same value as the library's: fmaf is exact either way)
    flags = ["-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-pthread"] + (["-mfma"] if _has_fma() else [])
    subprocess.run(["g++", *flags, *extra, SRC, "-o", exe], check=True, capture_output=True)
    return exe


def _run(exe, what, timeout):
    r = subprocess.run([exe, what], capture_output=True, text=True, timeout=timeout)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = re.findall(r"^(\w+) pairs (\d+) in_domain (\d+) guarded_mismatch (\d+) core_mismatch (\d+)$",
                      r.stdout, re.M)
    assert rows
    for name, pairs, in_domain, guarded, core in rows:
        assert int(pairs) > 0 and 8 * int(in_domain) > int(pairs), name  # the domain counts are not vacuous
        assert (int(guarded), int(core)) == (0, 0), name
    return {row[0] for row in rows}


@needs_gpp
def test_sequences_equal_division(tmp_path):
    exe = _build(str(tmp_path / "div_model"), ["-O2"])
    assert _run(exe, "all", 1200) == {"grid", "exponents", "random", "average"}


@needs_gpp
def test_model_under_sanitizers(tmp_path):
    exe = _build(str(tmp_path / "div_model_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert _run(exe, "exponents", 300) == {"exponents"}
    assert _run(exe, "average", 600) == {"average"}
