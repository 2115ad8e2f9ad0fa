"""CPU tests of the key side of the tss.go mirror in charon_amd/tbls.py
(SplitSecret / CombineShares on host integers) and of its argument
validation: nothing here needs a device."""
import itertools
import random

import pytest


def test_split_combine_round_trips():
    from charon_amd import tbls
    rng = random.Random(11)
    for t, n in ((2, 3), (3, 4), (4, 4), (3, 6)):
        secret = rng.randrange(1, tbls.R)
        shares, poly = tbls._split_host(secret, t, n, rng)
        assert [s.identifier for s in shares] == list(range(1, n + 1)) and poly[0] == secret and len(poly) == t
        for sub in itertools.combinations(shares, t):  # any t of n recover the secret
            assert tbls.combine_shares(sub, t, n) == secret
        assert tbls.combine_shares(shares, t, n) == secret  # more than t shares
        with pytest.raises(tbls.TblsError, match="fewer shares"):
            tbls.combine_shares(shares[:t - 1], t, n)
        with pytest.raises(tbls.TblsError, match="duplicate"):
            tbls.combine_shares([shares[0]] * t, t, n)
        if t > 2:  # t - 1 shares interpolate another polynomial
            assert tbls.combine_shares(shares[:t - 1], t - 1, n) != secret


def test_split_matches_the_oracle_polynomial():
    from charon_amd import tbls
    from oracle import tbls_oracle as orc
    assert tbls.R == orc.R
    rng = random.Random(5)
    shares, poly = tbls._split_host(1234567, 3, 5, rng)
    want, _ = orc.split_secret(1234567, 3, 5, poly[1:])
    assert {s.identifier: s.value for s in shares} == want
    assert tbls.combine_shares(shares[2:], 3, 5) == 1234567


def test_python_layer_validates_without_a_device():
    from charon_amd import dkg, tbls
    rng = random.Random(1)
    for t, n in ((1, 3), (4, 3), (2, 256)):
        with pytest.raises(tbls.TblsError, match="new Feldman VSS"):
            tbls.split_secret(5, t, n, rng)
        with pytest.raises(tbls.TblsError, match="generate secret shares: new Feldman VSS"):
            tbls.generate_tss(t, n, rng)
        with pytest.raises(tbls.TblsError, match="new Feldman VSS"):
            tbls.combine_shares([], t, n)
        with pytest.raises(tbls.TblsError, match="new Feldman VSS"):
            dkg.create_cluster_tss([5], t, n, rng, engine=object())
    with pytest.raises(tbls.TblsError, match="zero secret"):
        tbls.split_secret(tbls.R, 2, 3, rng)
    for ident in (0, 256):
        with pytest.raises(tbls.TblsError):
            tbls.SecretKeyShare(ident, 1)
    with pytest.raises(tbls.TblsError, match="invalid share identifier"):
        tbls.combine_shares([tbls.SecretKeyShare(1, 1), tbls.SecretKeyShare(9, 1)], 2, 3)
    assert dkg.create_cluster_tss([], 2, 3, rng, engine=object()) == ([], [])
    assert tbls._sk32(tbls.R + 5) == (5).to_bytes(32, "big")
