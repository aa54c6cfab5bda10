"""Kernel A's item feed (kamd_core.h ItemFeed -- the functions k_match_v3 takes its positions through), driven on the CPU (tests/emu_matchfeed):
W emulated wavefronts against one plain counter in a seeded random interleaving, each asking for its next grant ahead of need as the kernel does.

  exactly once   every position of [0, n) is handed to a lane once, whatever the interleaving
  none beyond    no position at or behind n is handed out, although the cursor itself runs past n (a wavefront learns that it is done from a grant
                 that begins there)
  fixed chunks   the same functions with one grant made at the start and no request: the fixed-chunk form of the kernel
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu_matchfeed")
GRANTS = (64, 256, 1000)
WAVES = (1, 3, 24)
_lib = None


def _emu():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", EMU], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(EMU, "libkamd_matchfeed_emu.so"))
        _lib.emu_match_feed.restype = C.c_int
        _lib.emu_match_feed.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.emu_match_feed_fixed.restype = C.c_int
        _lib.emu_match_feed_fixed.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]
    return _lib


def _sizes(grant):
    return sorted({0, 1, 63, 64, 65, grant - 1, grant, grant + 1, 5000})


def _run(n, grant, waves, seed):
    handed = np.zeros(n + 1, np.uint32)
    beyond, requests, cursor = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = _emu().emu_match_feed(n, grant, waves, seed, handed.ctypes.data_as(C.c_void_p), C.byref(beyond), C.byref(requests), C.byref(cursor))
    return rc, handed[:n], int(beyond.value), int(requests.value), int(cursor.value)


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("grant", GRANTS)
def test_every_position_once_and_none_beyond(grant, waves):
    for n in _sizes(grant):
        for seed in range(1, 9):
            rc, handed, beyond, requests, cursor = _run(n, grant, waves, 1000003 * seed + 31 * n + grant + waves)
            assert rc == 0, (n, grant, waves, seed)
            assert beyond == 0, (n, grant, waves, seed, beyond)
            assert np.array_equal(handed, np.ones(n, np.uint32)), (n, grant, waves, seed, np.flatnonzero(handed != 1)[:8])
            # the cursor moved by whole grants: one request per grant that holds positions, and per wavefront at most one that begins behind n
            assert cursor == requests * grant
            assert max(waves, -(-n // grant)) <= requests <= -(-n // grant) + waves, (n, grant, waves, requests)


@pytest.mark.parametrize("ipw", GRANTS)
def test_fixed_chunks_are_the_same_feed_without_requests(ipw):
    for n in _sizes(ipw):
        handed = np.zeros(n + 1, np.uint32)
        beyond = C.c_uint64(0)
        rc = _emu().emu_match_feed_fixed(n, ipw, 77 + n, handed.ctypes.data_as(C.c_void_p), C.byref(beyond))
        assert rc == 0, (n, ipw, rc)   # (-2: the fixed form asked for a grant)
        assert beyond.value == 0
        assert np.array_equal(handed[:n], np.ones(n, np.uint32)), (n, ipw)


def test_stand_alone_program_agrees():
    """the same cases as a program with its own main (the form a sanitizer build of this code runs in: `make -C tests/emu_matchfeed san`)"""
    _emu()
    out = subprocess.run([os.path.join(EMU, "matchfeed_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout
