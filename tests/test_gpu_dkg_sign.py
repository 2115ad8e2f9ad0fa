"""A whole ceremony through the hardened signer: 3 DVs, 3-of-4.

create_cluster_tss(hardened=True) makes the keys; every peer produces its
deposit-data and lock-hash partials with dkg.sign_deposit_data /
sign_lock_hash (tbg_sign_ct); the existing consuming halves
(agg_and_verify_deposit_data, agg_lock_hash_sig, verify_multi_signature) take
them unchanged.
"""
import random

import pytest

from charon_amd import dkg
from charon_amd import engine as eng
from charon_amd import tbls
from oracle import c as oc

pytestmark = pytest.mark.gpu

N_DV, T, N = 3, 3, 4
LOCK_HASH = bytes(range(32))


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(0, slots=2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ceremony(engine):
    rng = random.Random(0xD4)
    secrets = [rng.randrange(1, tbls.R) for _ in range(N_DV)]
    dvs, splits = dkg.create_cluster_tss(secrets, T, N, random.Random(0xD5), engine=engine, hardened=True)
    dv_keys = [tss.public_key.raw for tss in dvs]
    roots = {dv: b"deposit root of " + dv[:8] + bytes(8) for dv in dv_keys}
    pubshares = {dv: {i: tss.public_share(i).raw for i in range(1, N + 1)} for dv, tss in zip(dv_keys, dvs)}
    return dict(secrets=secrets, dvs=dvs, splits=splits, dv_keys=dv_keys, roots=roots, pubshares=pubshares)


def peer_shares(c, peer):
    return {dv: c["splits"][d][peer - 1] for d, dv in enumerate(c["dv_keys"])}


def exchanged(per_peer):
    """{dv: [every peer's DKGPartial]} from the peers' own sets."""
    data = {}
    for parts in per_peer:
        for dv, p in parts.items():
            data.setdefault(dv, []).append(p)
    return data


def test_hardened_cluster_keys_equal_the_plain_ones(engine, ceremony):
    dvs, splits = dkg.create_cluster_tss(ceremony["secrets"], T, N, random.Random(0xD5), engine=engine)
    assert splits == ceremony["splits"]
    for a, b in zip(dvs, ceremony["dvs"]):
        assert a.public_key == b.public_key and a.commitments == b.commitments and a.pubshares == b.pubshares
    for tss, s in zip(ceremony["dvs"], ceremony["secrets"]):
        assert tss.public_key.raw == oc.sk_to_pk(s)


def test_generate_tss_hardened_equals_plain(engine):
    plain = tbls.generate_tss(T, N, random.Random(0xD6), engine=engine)
    hard = tbls.generate_tss(T, N, random.Random(0xD6), engine=engine, hardened=True)
    assert hard == plain
    tss, shares, secret = hard
    assert tss.public_key.raw == oc.sk_to_pk(secret)
    assert [tss.public_share(s.identifier).raw for s in shares] == [oc.sk_to_pk(s.value) for s in shares]
    with pytest.raises(tbls.TblsError, match="unmarshal secret: secret key cannot be zero"):
        tbls.tss_from_shares([tbls.SecretKeyShare(1, 0)], tss.commitments, engine=engine, hardened=True)


def test_ceremony_accepts_and_matches_the_group_signatures(engine, ceremony):
    c = ceremony
    deposit = exchanged(dkg.sign_deposit_data(peer_shares(c, p), p, c["roots"], engine=engine) for p in range(1, N + 1))
    lock = exchanged(dkg.sign_lock_hash(peer_shares(c, p), p, LOCK_HASH, engine=engine) for p in range(1, N + 1))
    assert all([p.share_idx for p in deposit[dv]] == [1, 2, 3, 4] for dv in c["dv_keys"])
    aggs = dkg.agg_and_verify_deposit_data(deposit, c["pubshares"], c["roots"], engine=engine)
    for dv, s in zip(c["dv_keys"], c["secrets"]):
        assert aggs[dv] == oc.sign(s, c["roots"][dv])
    agg_sig, agg_pk = dkg.agg_lock_hash_sig(lock, c["pubshares"], LOCK_HASH, engine=engine)
    assert dkg.verify_multi_signature(agg_pk, LOCK_HASH, agg_sig, engine=engine)
    assert dkg.agg_sign_lock_hash(c["splits"], LOCK_HASH, engine=engine) == agg_sig


def test_create_cluster_deposit_signatures(engine, ceremony):
    c = ceremony
    pks = tbls.secret_to_public_key_batch(c["secrets"], engine=engine)
    assert [p.raw for p in pks] == c["dv_keys"]
    sigs = dkg.create_cluster_sign_deposit_data(c["secrets"], [c["roots"][dv] for dv in c["dv_keys"]], engine=engine)
    assert sigs == [oc.sign(s, c["roots"][dv]) for s, dv in zip(c["secrets"], c["dv_keys"])]


def test_a_wrong_share_is_refused_by_the_existing_verifier(engine, ceremony):
    c = ceremony
    sets = []
    for p in range(1, N + 1):
        shares = peer_shares(c, p)
        if p == 2:  # peer 2 signs the first DV's root with peer 3's share of it
            shares[c["dv_keys"][0]] = c["splits"][0][2]
        sets.append(dkg.sign_deposit_data(shares, p, c["roots"], engine=engine))
    with pytest.raises(dkg.DKGError, match="invalid deposit data partial signature from peer"):
        dkg.agg_and_verify_deposit_data(exchanged(sets), c["pubshares"], c["roots"], engine=engine)


def test_a_zero_or_out_of_range_share_raises(engine, ceremony):
    c = ceremony
    for bad in (0, tbls.R):
        shares = peer_shares(c, 1)
        shares[c["dv_keys"][1]] = bad
        with pytest.raises(dkg.DKGError, match="unmarshal secret"):
            dkg.sign_lock_hash(shares, 1, LOCK_HASH, engine=engine)
        with pytest.raises(dkg.DKGError, match="unmarshal secret"):
            dkg.sign_deposit_data(shares, 1, c["roots"], engine=engine)
