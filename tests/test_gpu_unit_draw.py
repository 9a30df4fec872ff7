"""The kernels' unit-sphere draw (hippt_trace.h rius: vector loop with a wave-uniform escape branch, then a
scalar tail for the last pending lanes) against the oracle's po_random_in_unit_sphere, bit for bit: every
lane's exit state, coordinates and |p|^2.

tests/native/draw_selftest.hip runs the production rius on host-given entry states, four waves per launch,
each under its own lane mask.  The sets:
  random   64 random states per wave, full and partial masks
  late     waves where all lanes but one or two accept at the first try (found by search on the CPU): the
           scalar tail does the remaining tries
  cycles   the late lanes sit on the hash's short cycles (tests/test_rng_cycles.py): the tail crosses try 64
           and must escape exactly as the oracle does
  crowd    more lanes on cycles than the tail takes: the vector loop itself crosses try 64 (the escape's
           wave-uniform branch)
The CPU part asserts the sets' premises on the oracle alone."""
import ctypes
import functools
import os

import numpy as np
import pytest

import pyoracle as po
from hit_ref import fmaf

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "native", "libdraw_selftest.so")
F = np.float32
CYCLES = (0, 3496737362, 160893342, 2247562032)
FULL = (1 << 64) - 1


def oracle_draw(s0):
    """po_random_in_unit_sphere from state s0: (exit state, x, y, z, r2)."""
    st = ctypes.c_uint32(s0)
    p = (ctypes.c_float * 3)()
    po.lib().po_random_in_unit_sphere(ctypes.byref(st), p)
    x, y, z = F(p[0]), F(p[1]), F(p[2])
    return st.value, x, y, z, fmaf(x, x, fmaf(y, y, z * z))


def tries_of(s0):
    """The loop restated with the oracle's po_rand01, counting tries: (tries, exit state)."""
    st = ctypes.c_uint32(s0)
    r = po.lib().po_rand01
    for tries in range(1, 1000):
        x = fmaf(2.0, r(ctypes.byref(st)), -1.0)
        y = fmaf(2.0, r(ctypes.byref(st)), -1.0)
        z = fmaf(2.0, r(ctypes.byref(st)), -1.0)
        if fmaf(x, x, fmaf(y, y, z * z)) < F(1.0):
            return tries, st.value
        if tries % 64 == 0:
            st.value ^= 0x9E3779B9
    raise AssertionError(f"state {s0}: no candidate accepted in 1000 tries")


@functools.lru_cache(maxsize=None)
def pools():
    """(states accepted at the first try, states that need at least 6 tries), from one random sample."""
    rng = np.random.default_rng(5)
    first, late = [], []
    for s in rng.integers(0, 1 << 32, size=6000, dtype=np.uint64).tolist():
        n, _ = tries_of(s)
        if n == 1:
            first.append(s)
        elif 6 <= n <= 64:
            late.append(s)
    return tuple(first), tuple(late)


def wave(base, special=()):
    """64 entry states: `base` states in order, with `special` = ((lane, state), ...) put in."""
    w = list(base[:64])
    for lane, s in special:
        w[lane] = s
    return w


@functools.lru_cache(maxsize=None)
def sets():
    """name -> (states (256,), masks (4,)): computed once."""
    first, late = pools()
    assert len(first) >= 64 * 4 and len(late) >= 8
    rng = np.random.default_rng(9)
    rnd = lambda: rng.integers(0, 1 << 32, size=64, dtype=np.uint64).tolist()  # noqa: E731
    f = lambda k: first[64 * k:64 * k + 64]  # noqa: E731
    odd, low3 = 0xAAAAAAAAAAAAAAAA, 0b111
    out = {
        "random": ([rnd(), rnd(), rnd(), rnd()], [FULL, 0x5555555555555555, 0xFFFF0000FFFF0001, 1 << 63]),
        "late": ([wave(f(0), [(37, late[0])]), wave(f(1), [(0, late[1]), (63, late[2])]),
                  wave(f(2), [(5, late[3]), (6, late[4])]), wave(f(3), [(1, late[5])])],
                 [FULL, FULL, 0x00000000FFFFFFFF, odd]),
        "cycles": ([wave(f(0), [(11, CYCLES[0])]), wave(f(1), [(2, CYCLES[1]), (62, CYCLES[2])]),
                    wave(f(2), [(33, CYCLES[3])]), wave(f(3), [(1, CYCLES[2])])],
                   [FULL, FULL, 0xFFFFFFFF00000000, low3]),
        "crowd": ([wave(rnd(), [(k * 9, CYCLES[k]) for k in range(4)]),
                   wave(f(0), [(k * 7 + 1, CYCLES[k % 4]) for k in range(8)]),
                   [CYCLES[k % 4] for k in range(64)],
                   wave([CYCLES[k % 4] for k in range(64)], [(k, first[k]) for k in range(1, 64, 2) if k > 10])],
                  [FULL, FULL, FULL, odd]),
    }
    return {k: (np.array(sum(w, []), np.uint32), np.array(m, np.uint64)) for k, (w, m) in out.items()}


def active_lanes(masks):
    return [bool((int(masks[i >> 6]) >> (i & 63)) & 1) for i in range(256)]


def test_selftest_library_builds():
    assert os.path.exists(LIB), "build() / make -C tests/native -f draw.mk builds it"


def test_restated_loop_is_the_oracles():
    for s in list(CYCLES) + list(pools()[1][:8]) + [12345, 357741884]:
        assert tries_of(s)[1] == oracle_draw(s)[0]


def test_premises():
    """On the oracle alone: what each set is meant to exercise."""
    first, late = pools()
    assert all(tries_of(s)[0] > 64 for s in CYCLES)  # a lane on a short cycle needs the escape
    S = sets()
    for name in ("late", "cycles"):
        st, masks = S[name]
        act = active_lanes(masks)
        for w in range(4):
            n = [tries_of(int(st[i]))[0] for i in range(64 * w, 64 * w + 64) if act[i]]
            slow = [x for x in n if x > 1]
            assert 1 <= len(slow) <= 2 and len(n) > len(slow), (name, w, n)  # all but one or two at the first try
            assert min(slow) > (64 if name == "cycles" else 5), (name, w, slow)
    st, masks = S["crowd"]
    act = active_lanes(masks)
    for w in range(4):
        n = [tries_of(int(st[i]))[0] for i in range(64 * w, 64 * w + 64) if act[i]]
        assert sum(x > 64 for x in n) >= 4, (w, n)  # more than the tail's K <= 3 lanes cross try 64


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["random", "late", "cycles", "crowd"])
def test_draw_matches_oracle(name):
    st, masks = sets()[name]
    lib = ctypes.CDLL(LIB)
    state = np.zeros(256, np.uint32)
    out = np.zeros((256, 4), np.float32)
    assert lib.draw_selftest(st.ctypes.data_as(ctypes.c_void_p), masks.ctypes.data_as(ctypes.c_void_p),
                             state.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == 0
    act = active_lanes(masks)
    want_state = np.array(st, np.uint32)
    want = np.zeros((256, 4), np.float32)
    want[:, 3] = -1.0
    for i in range(256):
        if act[i]:
            s, x, y, z, r2 = oracle_draw(int(st[i]))
            want_state[i] = s
            want[i] = (x, y, z, r2)
    bad = np.flatnonzero((state != want_state) | (out.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert bad.size == 0, f"{name}: lanes {bad[:8].tolist()} differ: state {state[bad[:4]]} vs {want_state[bad[:4]]}, " \
                          f"{out[bad[:4]]} vs {want[bad[:4]]}"
