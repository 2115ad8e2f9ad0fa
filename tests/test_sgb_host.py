"""The batched G2 subgroup test (charon_amd/csrc/k_sgb.hip) on the host:
the kernels' math compiled for the CPU (tests/hostcheck, lane pairs
emulated) against the oracle's exact subgroup decisions.

A group of decoded signatures passes iff all 18 random combinations
sum c_i s_i (c_i uniform mod 13, bls_rlc.h sgb_digits) satisfy
psi(Q) == [x] Q.  Checked here: the digits' range and distribution, a group
of G2 points passes, and every crafted non-subgroup kind of
tests/golden/sgb_points.json (13- and 23-torsion components, a bare torsion
point, a pair whose components cancel in a plain sum) fails the group at any
position, with decode failures left out of the sums.  The twin folds the
bucket slices and forms the running sums with the kernels' own templates
(bls_sgb.h), so the sums that meet two equal operands -- short groups, whose
empty buckets add the running sum to itself, and groups of duplicated
signatures -- are checked here too: they are redone with the complete formulas
and never fail a group of G2 points (`redo=False` is the control that shows
each such case does reach the exceptional path).  The per-item verdicts
(k_subgroup_sigs after a failed group) are checked on the GPU against
oracle/c (tests/test_gpu_sgb.py).
"""
import ctypes
import json
import os
import random

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def hc():
    from tests.hostcheck import lib
    h = lib()
    h.hc_sgb_group.restype = ctypes.c_int
    h.hc_sgb_group.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32]
    h.hc_sgb_digits.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    h.hc_sgb_group_ex.restype = ctypes.c_int
    h.hc_sgb_group_ex.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return h


@pytest.fixture(scope="module")
def crafted():
    with open(os.path.join(HERE, "golden", "sgb_points.json")) as f:
        return {k: [bytes.fromhex(h) for h in v] for k, v in json.load(f)["points"].items()}


@pytest.fixture(scope="module")
def g2_points():
    from oracle import bls12_381 as bls
    rng = random.Random(0x5B)
    return [bls.g2_compress(bls.g2_mul(bls.G2_GEN, rng.randrange(1, bls.R))) for _ in range(48)]


SEED = np.array([0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0x4B5A6978, 0x11111111, 0x22222222, 0x33333333, 0x44444444],
                dtype=np.uint32)


def group_mask(hc, sigs, i0=0, seed=SEED):
    buf = b"".join(sigs)
    return hc.hc_sgb_group(buf, len(sigs), seed.ctypes.data_as(ctypes.c_void_p), i0)


def test_digits_uniform_mod_13(hc):
    out = np.zeros(18, dtype=np.int32)
    counts = np.zeros(13, dtype=np.int64)
    n = 4000
    for i in range(n):
        hc.hc_sgb_digits(SEED.ctypes.data_as(ctypes.c_void_p), i, out.ctypes.data_as(ctypes.c_void_p))
        assert out.min() >= -6 and out.max() <= 6
        np.add.at(counts, out + 6, 1)
    exp = n * 18 / 13
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    assert chi2 < 40, counts  # 12 degrees of freedom: p ~ 1e-4 at 40


def test_digits_depend_on_seed_and_index(hc):
    a, b, c = (np.zeros(18, dtype=np.int32) for _ in range(3))
    other = SEED.copy()
    other[7] ^= 1
    hc.hc_sgb_digits(SEED.ctypes.data_as(ctypes.c_void_p), 5, a.ctypes.data_as(ctypes.c_void_p))
    hc.hc_sgb_digits(SEED.ctypes.data_as(ctypes.c_void_p), 6, b.ctypes.data_as(ctypes.c_void_p))
    hc.hc_sgb_digits(other.ctypes.data_as(ctypes.c_void_p), 5, c.ctypes.data_as(ctypes.c_void_p))
    assert not np.array_equal(a, b) and not np.array_equal(a, c)


def test_group_of_g2_points_passes(hc, g2_points):
    assert group_mask(hc, g2_points) == 0
    assert group_mask(hc, g2_points, i0=512 * 7) == 0


@pytest.mark.parametrize("kind", ["t13", "t23", "torsion13"])
@pytest.mark.parametrize("pos", [0, 17, 47])
def test_crafted_point_fails_the_group(hc, g2_points, crafted, kind, pos):
    from oracle import bls12_381 as bls
    sigs = list(g2_points)
    sigs[pos] = crafted[kind][pos % len(crafted[kind])]
    with pytest.raises(bls.DecodeError):
        bls.g2_decompress(sigs[pos])  # the oracle's exact decision: outside G2
    assert group_mask(hc, sigs) != 0


def test_cancelling_pair_fails_the_group(hc, g2_points, crafted):
    from oracle import bls12_381 as bls
    a, b = crafted["pair_a"][0], crafted["pair_b"][0]
    # their torsion components cancel in a plain sum: both decode outside G2,
    # their sum is in G2 -- only the random coefficients separate them
    pa, pb = bls.g2_decompress(a, subgroup_check=False), bls.g2_decompress(b, subgroup_check=False)
    assert bls.g2_in_subgroup(bls.g2_add(pa, pb))
    sigs = list(g2_points)
    sigs[3], sigs[40] = a, b
    assert group_mask(hc, sigs) != 0
    for seed_word in range(1, 6):  # every seed separates them (13^-18 per seed)
        seed = SEED.copy()
        seed[0] = seed_word
        assert group_mask(hc, sigs, seed=seed) != 0


def test_two_bad_points_in_one_group(hc, g2_points, crafted):
    sigs = list(g2_points)
    sigs[1], sigs[2] = crafted["t13"][1], crafted["t13"][2]
    assert group_mask(hc, sigs) != 0


def test_decode_failures_are_left_out(hc, g2_points):
    sigs = list(g2_points)
    bad = bytearray(sigs[5])
    bad[0] &= 0x7F  # no compression flag: a decode error, not a member of any sum
    sigs[5] = bytes(bad)
    assert group_mask(hc, sigs) == 0


# ---- sums that meet two equal operands (bls_sgb.h) -------------------------
SPLITS = (1, 4)  # slices per bucket: none, and k_sgb_fold's at groups of 1,024
SHORT_I0 = (0, 2048, 5120, 7777)


def group_mask_ex(hc, sigs, i0=0, split=1, redo=True, seed=SEED):
    """(mask of failed combinations, sums redone with the complete formulas)."""
    n_redo = ctypes.c_int(-1)
    mask = hc.hc_sgb_group_ex(b"".join(sigs), len(sigs), seed.ctypes.data_as(ctypes.c_void_p), i0, split,
                              1 if redo else 0, ctypes.byref(n_redo))
    return mask, n_redo.value


@pytest.mark.parametrize("i0", SHORT_I0)
@pytest.mark.parametrize("members", [1, 2, 3, 4, 8, 16])
def test_short_group_of_g2_points_passes(hc, g2_points, members, i0):
    for split in SPLITS:
        mask, _ = group_mask_ex(hc, g2_points[:members], i0=i0, split=split)
        assert mask == 0, (split, bin(mask))
    assert group_mask(hc, g2_points[:members], i0=i0) == 0


def test_short_groups_reach_the_exceptional_path(hc, g2_points):
    """Without the redo (the running sums' additions alone, no doubling
    branch) groups of 1 .. 8 clean members fail at every i0: a combination
    whose highest non-empty bucket has an empty one below it adds the running
    sum to itself.  One member: a digit d fails unless d is 0 or 1, and a
    digit is 0, 1 or -1 with probability 3/13, so about 14 of 18 fail."""
    failed = {}
    for members in (1, 2, 4, 8):
        for i0 in SHORT_I0:
            mask, n_redo = group_mask_ex(hc, g2_points[:members], i0=i0, redo=False)
            assert n_redo == 0
            failed[members, i0] = bin(mask).count("1")
            ok_mask, n_redo = group_mask_ex(hc, g2_points[:members], i0=i0, redo=True)
            assert ok_mask == 0 and n_redo >= failed[members, i0]
    print("failed combinations of 18 without the redo:", failed)
    assert all(v > 0 for v in failed.values()), failed
    assert all(failed[1, i0] >= 9 for i0 in SHORT_I0), failed


@pytest.mark.parametrize("split", SPLITS)
def test_duplicated_signatures_pass(hc, g2_points, split):
    one = [g2_points[0]] * 48
    four = [g2_points[k % 4] for k in range(48)]
    grouped = [g2_points[k // 12] for k in range(48)]
    for sigs in (one, four, grouped):
        for i0 in (0, 2048):
            mask, n_redo = group_mask_ex(hc, sigs, i0=i0, split=split)
            assert mask == 0, bin(mask)


def test_duplicated_signatures_reach_the_exceptional_path(hc, g2_points):
    """48 copies of one signature s: every bucket and slice sum is a small
    multiple of s, so equal operands are certain in the fold (split 4) and in
    the running sums."""
    for split in SPLITS:
        mask, _ = group_mask_ex(hc, [g2_points[0]] * 48, split=split, redo=False)
        assert mask != 0
        mask, n_redo = group_mask_ex(hc, [g2_points[0]] * 48, split=split, redo=True)
        assert mask == 0 and n_redo > 0


@pytest.mark.parametrize("kind", ["t13", "t23", "torsion13"])
def test_crafted_point_alone_fails_its_group(hc, crafted, kind):
    for i0 in SHORT_I0:
        for split in SPLITS:
            mask, _ = group_mask_ex(hc, [crafted[kind][0]], i0=i0, split=split)
            assert mask != 0, (i0, split)


@pytest.mark.parametrize("kind", ["t13", "t23", "torsion13"])
def test_crafted_point_last_of_four_fails_the_group(hc, g2_points, crafted, kind):
    for i0 in SHORT_I0:
        for split in SPLITS:
            mask, _ = group_mask_ex(hc, g2_points[:3] + [crafted[kind][0]], i0=i0, split=split)
            assert mask != 0, (i0, split)
