"""The batched subgroup test's paired schedule (charon_amd/csrc/k_sgb.hip:
buckets over two combinations' digits at once) on the host: a twin built from
the kernels' own templates (bls_sgb.h sgb_pair_code / sgb_pair_sum_g /
sgb_running_sums_g, lane pairs emulated, tests/sgbpair) against

  * Q_k = sum_i c_ik s_i formed member by member with the complete additions
    (no buckets): every one of the 18 sums must be the same affine point, and
  * the classic schedule's twin (tests/hostcheck hc_sgb_group): the same
    18-bit mask of failed combinations.

Empty buckets (infinity operands) are the rule in the paired schedule's 13-term
sums; equal operands come from replayed signatures and from the running sums
of short groups.  Such a sum is redone with the complete formulas and never
fails a group of G2 points; `redo=False` is the control that shows the cases
do reach that path.
"""
import ctypes

import numpy as np
import pytest

SEED = np.array([0x01234567, 0x89ABCDEF, 0x0F1E2D3C, 0x4B5A6978, 0x11111111, 0x22222222, 0x33333333, 0x44444444],
                dtype=np.uint32)
I0S = (0, 2048, 7777)


@pytest.fixture(scope="module")
def sp():
    from tests.sgbpair import lib
    return lib()


@pytest.fixture(scope="module")
def hc():
    from tests.hostcheck import lib
    h = lib()
    h.hc_sgb_group.restype = ctypes.c_int
    h.hc_sgb_group.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32]
    h.hc_sgb_digits.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    return h


@pytest.fixture(scope="module")
def g2_points():
    """512 points of G2: small multiples of a few random ones (one scalar
    multiplication each would dominate the module's time)."""
    import random
    from oracle import bls12_381 as bls
    rng = random.Random(0x5B2)
    out = []
    for _ in range(8):
        base = bls.g2_mul(bls.G2_GEN, rng.randrange(1, bls.R))
        p = base
        for _ in range(64):
            out.append(bls.g2_compress(p))
            p = bls.g2_add(p, base)
    rng.shuffle(out)
    assert len(set(out)) == 512
    return out


@pytest.fixture(scope="module")
def crafted():
    """The non-subgroup kinds of tests/edge_points.py, compressed."""
    from oracle import bls12_381 as bls
    from tests import edge_points as ep
    b = ep.bank()
    return {k: bls.g2_compress(b[k]) for k in ("t13", "t23", "tor", "ns")}


def paired(sp, sigs, i0=0, redo=True, seed=SEED):
    """(mask of failed combinations, sums redone, the 18 sums compressed)."""
    q = ctypes.create_string_buffer(18 * 96)
    n_redo = ctypes.c_int(-1)
    mask = sp.sp_group(b"".join(sigs), len(sigs), seed.ctypes.data_as(ctypes.c_void_p), i0, 1 if redo else 0,
                       ctypes.byref(n_redo), q)
    assert mask >= 0
    return mask, n_redo.value, [q.raw[96 * k:96 * (k + 1)] for k in range(18)]


def reference(sp, sigs, i0=0, seed=SEED):
    q = ctypes.create_string_buffer(18 * 96)
    assert sp.sp_reference(b"".join(sigs), len(sigs), seed.ctypes.data_as(ctypes.c_void_p), i0, q) == 0
    return [q.raw[96 * k:96 * (k + 1)] for k in range(18)]


def classic_mask(hc, sigs, i0=0, seed=SEED):
    return hc.hc_sgb_group(b"".join(sigs), len(sigs), seed.ctypes.data_as(ctypes.c_void_p), i0)


def test_pair_codes_cover_the_84_buckets(sp):
    seen = {}
    for c0 in range(-6, 7):
        for c1 in range(-6, 7):
            cd = sp.sp_code(c0, c1)
            if (c0, c1) == (0, 0):
                assert cd == 0xFF
                continue
            idx, neg = cd & 0x7F, cd >> 7
            assert idx < 84 and neg == int(c0 < 0 or (c0 == 0 and c1 < 0))
            a, b = (-c0, -c1) if neg else (c0, c1)
            assert seen.setdefault(idx, (a, b)) == (a, b)  # (c0, c1) and (-c0, -c1) share a bucket, nothing else does
    assert sorted(seen) == list(range(84))
    assert [seen[i] for i in range(6)] == [(0, b) for b in range(1, 7)]
    assert seen[6] == (1, -6) and seen[83] == (6, 6)


def test_sums_match_the_oracle_for_one_and_two_members(sp, hc, g2_points):
    """An independent reference for the reference: Python integers."""
    from oracle import bls12_381 as bls
    for n in (1, 2):
        sigs = g2_points[:n]
        pts = [bls.g2_decompress(s) for s in sigs]
        digits = np.zeros(18, dtype=np.int32)
        want = [None] * 18
        for i, p in enumerate(pts):
            hc.hc_sgb_digits(SEED.ctypes.data_as(ctypes.c_void_p), 2048 + i, digits.ctypes.data_as(ctypes.c_void_p))
            for k in range(18):
                c = int(digits[k])
                if c:
                    t = bls.g2_mul_raw(p, abs(c))
                    want[k] = bls.g2_add(want[k], bls.g2_neg(t) if c < 0 else t)
        ref = reference(sp, sigs, i0=2048)
        assert ref == [bls.g2_compress(w) for w in want]
        assert paired(sp, sigs, i0=2048)[2] == ref


@pytest.mark.parametrize("i0", I0S)
@pytest.mark.parametrize("n", [1, 2, 7, 64])
def test_every_sum_is_the_same_point(sp, hc, g2_points, n, i0):
    sigs = g2_points[:n]
    mask, _, q = paired(sp, sigs, i0=i0)
    assert q == reference(sp, sigs, i0=i0)
    assert mask == 0 == classic_mask(hc, sigs, i0=i0)


@pytest.mark.parametrize("i0", [0, 5120])
def test_every_sum_is_the_same_point_512(sp, hc, g2_points, i0):
    mask, _, q = paired(sp, g2_points, i0=i0)
    assert q == reference(sp, g2_points, i0=i0)
    assert mask == 0 == classic_mask(hc, g2_points, i0=i0)


def test_48_copies_of_one_signature(sp, hc, g2_points):
    sigs = [g2_points[0]] * 48
    for i0 in I0S:
        mask, n_redo, q = paired(sp, sigs, i0=i0)
        assert q == reference(sp, sigs, i0=i0)
        assert mask == 0 == classic_mask(hc, sigs, i0=i0)
        assert n_redo > 0


def test_group_with_a_signature_and_its_negative(sp, hc, g2_points):
    from oracle import bls12_381 as bls
    s = bls.g2_decompress(g2_points[3])
    for n in (2, 7, 64):
        sigs = list(g2_points[:n])
        sigs[0], sigs[n - 1] = g2_points[3], bls.g2_compress(bls.g2_neg(s))
        for i0 in I0S:
            mask, _, q = paired(sp, sigs, i0=i0)
            assert q == reference(sp, sigs, i0=i0)
            assert mask == 0 == classic_mask(hc, sigs, i0=i0)


def test_decode_failures_are_left_out(sp, hc, g2_points):
    sigs = list(g2_points[:64])
    for pos in (0, 5, 63):
        bad = bytearray(sigs[pos])
        bad[0] &= 0x7F  # no compression flag: a decode error, not a member of any sum
        sigs[pos] = bytes(bad)
    kept = [s for i, s in enumerate(sigs) if i not in (0, 5, 63)]
    mask, _, q = paired(sp, sigs, i0=2048)
    assert q == reference(sp, sigs, i0=2048)
    assert mask == 0 == classic_mask(hc, sigs, i0=2048)
    # the sums are those of the 61 decodable members at THEIR indices: not of a group closed up
    assert q != paired(sp, kept, i0=2048)[2]


@pytest.mark.parametrize("kind", ["t13", "t23", "tor", "ns"])
@pytest.mark.parametrize("pos", [0, 31, 63])
def test_crafted_point_gives_the_classic_failure_mask(sp, hc, g2_points, crafted, kind, pos):
    from oracle import bls12_381 as bls
    sigs = list(g2_points[:64])
    sigs[pos] = crafted[kind]
    with pytest.raises(bls.DecodeError):
        bls.g2_decompress(sigs[pos])  # the oracle's exact decision: outside G2
    for i0 in (0, 2048):
        mask, _, q = paired(sp, sigs, i0=i0)
        assert q == reference(sp, sigs, i0=i0)
        assert mask != 0 and mask == classic_mask(hc, sigs, i0=i0), (bin(mask), i0)


def test_short_and_duplicate_groups_reach_the_exceptional_path(sp, g2_points):
    """Control, redo disabled: the additions without a doubling branch alone
    fail combinations of clean groups -- a short group's running sums add a sum
    to itself across empty buckets, and 48 copies of one signature make equal
    bucket sums -- and with the redo every such group passes, having redone at
    least as many sums as combinations failed without it."""
    failed = {}
    for name, sigs in (("1", g2_points[:1]), ("2", g2_points[:2]), ("7", g2_points[:7]),
                       ("48 copies", [g2_points[0]] * 48)):
        for i0 in I0S:
            mask, n_redo, _ = paired(sp, sigs, i0=i0, redo=False)
            assert n_redo == 0
            failed[name, i0] = bin(mask).count("1")
            ok_mask, n_redo, _ = paired(sp, sigs, i0=i0, redo=True)
            assert ok_mask == 0 and n_redo >= failed[name, i0] > 0, (name, i0, failed[name, i0], n_redo)
    print("failed combinations of 18 without the redo:", failed)
