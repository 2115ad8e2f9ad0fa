"""The batched subgroup test's triple schedule (charon_amd/csrc/k_sgb.hip:
buckets over three combinations' digits at once) on the host: a twin built
from the kernels' own templates (bls_sgb.h sgb_tri_code / sgb_tri_sum1_g /
sgb_tri_sum2_g / sgb_running_sums_g, lane pairs emulated, tests/sgbtri) against

  * Q_k = sum_i c_ik s_i formed member by member with the complete additions
    (no buckets): every one of the 18 sums must be the same affine point, and
  * the classic schedule's twin (tests/hostcheck hc_sgb_group): the same
    18-bit mask of failed combinations.

A triple has 1,098 buckets, so in small groups nearly every operand of the
two folding passes is infinity; 2,300 members are more than one triple's
buckets, so some buckets hold two or more.  Equal operands come from replayed
signatures and from the running sums of short groups.  Such a sum is redone
with the complete formulas and never fails a group of G2 points;
`redo=False` is the control that shows the cases do reach that path.
"""
import ctypes

import numpy as np
import pytest

SEED = np.array([0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0x4B5A6978, 0x11111111, 0x22222222, 0x33333333, 0x44444444],
                dtype=np.uint32)
I0S = (0, 16384, 7777)


@pytest.fixture(scope="module")
def st():
    from tests.sgbtri import lib
    return lib()


@pytest.fixture(scope="module")
def hc():
    from tests.hostcheck import lib
    h = lib()
    h.hc_sgb_group.restype = ctypes.c_int
    h.hc_sgb_group.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32]
    return h


@pytest.fixture(scope="module")
def g2_points():
    """2,304 distinct points of G2: small multiples of a few random ones (one
    scalar multiplication each would dominate the module's time)."""
    import random
    from oracle import bls12_381 as bls
    rng = random.Random(0x5B3)
    out = []
    for _ in range(9):
        base = bls.g2_mul(bls.G2_GEN, rng.randrange(1, bls.R))
        p = base
        for _ in range(256):
            out.append(bls.g2_compress(p))
            p = bls.g2_add(p, base)
    rng.shuffle(out)
    assert len(set(out)) == 2304
    return out


@pytest.fixture(scope="module")
def crafted():
    """The non-subgroup kinds of tests/edge_points.py, compressed."""
    from oracle import bls12_381 as bls
    from tests import edge_points as ep
    b = ep.bank()
    return {k: bls.g2_compress(b[k]) for k in ("t13", "t23", "tor", "ns")}


def triple(st, sigs, i0=0, redo=True, seed=SEED):
    """(mask of failed combinations, sums redone, the 18 sums compressed, members of the fullest bucket)."""
    q = ctypes.create_string_buffer(18 * 96)
    n_redo, fullest = ctypes.c_int(-1), ctypes.c_int(-1)
    mask = st.st_group(b"".join(sigs), len(sigs), seed.ctypes.data_as(ctypes.c_void_p), i0, 1 if redo else 0,
                       ctypes.byref(n_redo), q, ctypes.byref(fullest))
    assert mask >= 0
    return mask, n_redo.value, [q.raw[96 * k:96 * (k + 1)] for k in range(18)], fullest.value


def reference(st, sigs, i0=0, seed=SEED):
    q = ctypes.create_string_buffer(18 * 96)
    assert st.st_reference(b"".join(sigs), len(sigs), seed.ctypes.data_as(ctypes.c_void_p), i0, q) == 0
    return [q.raw[96 * k:96 * (k + 1)] for k in range(18)]


def classic_mask(hc, sigs, i0=0, seed=SEED):
    return hc.hc_sgb_group(b"".join(sigs), len(sigs), seed.ctypes.data_as(ctypes.c_void_p), i0)


def test_triple_codes_cover_the_1098_buckets(st):
    seen = {}
    for c0 in range(-6, 7):
        for c1 in range(-6, 7):
            for c2 in range(-6, 7):
                cd = st.st_code(c0, c1, c2)
                if (c0, c1, c2) == (0, 0, 0):
                    assert cd == 0xFFFFFFFF
                    continue
                idx, neg = cd & 0x7FF, cd >> 11
                first = next(c for c in (c0, c1, c2) if c)
                assert idx < 1098 and neg == int(first < 0)
                key = (-c0, -c1, -c2) if neg else (c0, c1, c2)
                assert seen.setdefault(idx, key) == key  # a triple and its negative share a bucket, nothing else does
    assert sorted(seen) == list(range(1098))
    assert [seen[i] for i in range(6)] == [(0, 0, c) for c in range(1, 7)]
    # the plane a = 0 is a pair's 84 buckets in the pair's order; the planes a >= 1 follow, c fastest
    assert seen[6] == (0, 1, -6) and seen[83] == (0, 6, 6)
    assert seen[84] == (1, -6, -6) and seen[85] == (1, -6, -5) and seen[1097] == (6, 6, 6)


@pytest.mark.parametrize("i0", I0S)
@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_every_sum_is_the_same_point(st, hc, g2_points, n, i0):
    sigs = g2_points[:n]
    mask, _, q, _ = triple(st, sigs, i0=i0)
    assert q == reference(st, sigs, i0=i0)
    assert mask == 0 == classic_mask(hc, sigs, i0=i0)


@pytest.mark.parametrize("n,i0", [(1100, 0), (1100, 16384), (2300, 32768)])
def test_every_sum_is_the_same_point_large(st, g2_points, n, i0):
    sigs = g2_points[:n]
    mask, _, q, fullest = triple(st, sigs, i0=i0)
    assert q == reference(st, sigs, i0=i0)
    assert mask == 0
    if n > 1098:
        assert fullest >= 2  # more members than a triple's buckets


def test_48_copies_of_one_signature(st, hc, g2_points):
    sigs = [g2_points[0]] * 48
    for i0 in I0S:
        mask, n_redo, q, _ = triple(st, sigs, i0=i0)
        assert q == reference(st, sigs, i0=i0)
        assert mask == 0 == classic_mask(hc, sigs, i0=i0)
        assert n_redo > 0


def test_group_with_a_signature_and_its_negative(st, hc, g2_points):
    from oracle import bls12_381 as bls
    s = bls.g2_decompress(g2_points[3])
    for n in (2, 7, 64):
        sigs = list(g2_points[:n])
        sigs[0], sigs[n - 1] = g2_points[3], bls.g2_compress(bls.g2_neg(s))
        for i0 in I0S:
            mask, _, q, _ = triple(st, sigs, i0=i0)
            assert q == reference(st, sigs, i0=i0)
            assert mask == 0 == classic_mask(hc, sigs, i0=i0)


def test_decode_failures_are_left_out(st, hc, g2_points):
    sigs = list(g2_points[:64])
    for pos in (0, 5, 63):
        bad = bytearray(sigs[pos])
        bad[0] &= 0x7F  # no compression flag: a decode error, not a member of any sum
        sigs[pos] = bytes(bad)
    kept = [s for i, s in enumerate(sigs) if i not in (0, 5, 63)]
    mask, _, q, _ = triple(st, sigs, i0=16384)
    assert q == reference(st, sigs, i0=16384)
    assert mask == 0 == classic_mask(hc, sigs, i0=16384)
    # the sums are those of the 61 decodable members at THEIR indices: not of a group closed up
    assert q != triple(st, kept, i0=16384)[2]


@pytest.mark.parametrize("kind", ["t13", "t23", "tor", "ns"])
@pytest.mark.parametrize("pos", [0, 31, 63])
def test_crafted_point_gives_the_classic_failure_mask(st, hc, g2_points, crafted, kind, pos):
    from oracle import bls12_381 as bls
    sigs = list(g2_points[:64])
    sigs[pos] = crafted[kind]
    with pytest.raises(bls.DecodeError):
        bls.g2_decompress(sigs[pos])  # the oracle's exact decision: outside G2
    for i0 in (0, 16384):
        mask, _, q, _ = triple(st, sigs, i0=i0)
        assert q == reference(st, sigs, i0=i0)
        assert mask != 0 and mask == classic_mask(hc, sigs, i0=i0), (bin(mask), i0)


def test_short_and_duplicate_groups_reach_the_exceptional_path(st, g2_points):
    """Control, redo disabled: the additions without a doubling branch alone
    fail combinations of clean groups -- a short group's running sums add a sum
    to itself across empty buckets, and 48 copies of one signature make equal
    bucket sums -- and with the redo every such group passes, having redone at
    least one sum."""
    failed = {}
    for name, sigs in (("1", g2_points[:1]), ("2", g2_points[:2]), ("7", g2_points[:7]),
                       ("48 copies", [g2_points[0]] * 48)):
        for i0 in I0S:
            mask, n_redo, _, _ = triple(st, sigs, i0=i0, redo=False)
            assert n_redo == 0
            failed[name, i0] = bin(mask).count("1")
            ok_mask, n_redo, _, _ = triple(st, sigs, i0=i0, redo=True)
            assert ok_mask == 0 and n_redo > 0 and failed[name, i0] > 0, (name, i0, failed[name, i0], n_redo)
    print("failed combinations of 18 without the redo:", failed)
