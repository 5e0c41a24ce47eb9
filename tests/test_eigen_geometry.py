"""CPU: the geometry cf_debug_eigen_geometry reports for the full-LDS Jacobi kernel (cf_eigen.hip,
DESIGN 3.1) -- which instantiation a cf_set_eigen_lanes setting launches, since the outputs cannot tell.

Expected values are worked out here, not read back from the library:
  - threads = lanes x lane groups, the groups being what the recursive-halving ordering needs
    (64 for n <= 128, 32 for n <= 64, 16 below), checked against the ordering's own budget
    2^L * ceil(ceil(n / 2^L) / 2) over every level L of every n of the bucket;
  - LD = the smallest value >= NR that is 16 or 48 (mod 64);
  - LDS bytes = 4 NR LD + 28 NR + 16 (B, items, five float rows, perm, flags), and the users per CU the
    block is sized for must fit the CU's 160 KiB.
"""
import ctypes

import pytest

from collaborative_filtering_amd import _native

LDS_PER_CU = 163840
DEFAULT_LANES = {1: 8, 2: 8, 3: 8, 4: 8, 5: 4, 6: 4, 7: 4, 8: 8}   # the measured best per bucket
GROUPS = {1: 16, 2: 16, 3: 32, 4: 32, 5: 64, 6: 64, 7: 64, 8: 64}
# users per CU the 4-lane blocks are sized for (LDS-bound from bucket 4 up)
USERS_4 = {4: 7, 5: 5, 6: 3, 7: 3, 8: 2}
USERS_8 = {4: 6, 5: 3, 6: 2, 7: 2, 8: 2}


def geometry(emax, setting):
    lib = _native.load()
    out = [ctypes.c_int(-1) for _ in range(5)]
    rc = lib.cf_debug_eigen_geometry(emax, setting, *[ctypes.byref(x) for x in out])
    assert rc == 0, (emax, setting, rc)
    return dict(zip(("lanes", "threads", "ld", "lds_bytes", "users"), (x.value for x in out)))


def expected_ld(nr):
    ld = nr
    while ld % 64 not in (16, 48):
        ld += 1
    return ld


@pytest.mark.parametrize("emax", range(1, 9))
@pytest.mark.parametrize("setting", [0, 4, 8])
def test_buckets_1_to_8(emax, setting):
    g = geometry(emax, setting)
    lanes = DEFAULT_LANES[emax] if setting == 0 else setting
    nr = 16 * emax
    assert g["lanes"] == lanes
    assert g["threads"] == lanes * GROUPS[emax]
    assert g["threads"] >= nr and g["threads"] >= 64 and g["threads"] % 64 == 0
    assert g["ld"] == expected_ld(nr) and g["ld"] % 4 == 0
    assert g["lds_bytes"] == 4 * nr * g["ld"] + 28 * nr + 16
    users = (USERS_4 if lanes == 4 else USERS_8).get(emax)
    if users is not None:
        assert g["users"] == users
    assert g["users"] >= 1 and g["lds_bytes"] * g["users"] <= LDS_PER_CU
    # the register budget follows the wave slots: users x waves per block within 8 waves per SIMD
    assert g["users"] * (g["threads"] // 64) <= 32


@pytest.mark.parametrize("emax", range(1, 9))
@pytest.mark.parametrize("setting", [4, 8])
def test_lane_groups_cover_the_ordering(emax, setting):
    g = geometry(emax, setting)
    groups = g["threads"] // g["lanes"]
    for k in range(max(2, 16 * (emax - 1) + 1), 16 * emax + 1):
        n = (k + 1) & ~1
        level = 0
        while True:
            segmax = (n + (1 << level) - 1) >> level
            if segmax < 2:
                break
            assert (1 << level) * ((segmax + 1) >> 1) <= groups, (emax, setting, k, level)
            level += 1


@pytest.mark.parametrize("emax", range(9, 13))
def test_buckets_9_to_12_keep_their_geometry(emax):
    ld = {9: 144, 10: 208, 11: 208, 12: 200}[emax]
    for setting in (0, 4, 8):
        g = geometry(emax, setting)
        assert (g["lanes"], g["threads"], g["ld"], g["users"]) == (8, 1024, ld, 1)
        assert g["lds_bytes"] == 4 * 16 * emax * ld + 28 * 16 * emax + 16 <= LDS_PER_CU


def test_rejects_bad_arguments():
    lib = _native.load()
    for emax, setting in [(0, 0), (13, 0), (4, 2), (4, 16), (4, -1)]:
        assert lib.cf_debug_eigen_geometry(emax, setting, None, None, None, None, None) != 0
    assert lib.cf_debug_eigen_geometry(4, 0, None, None, None, None, None) == 0
