"""GPU tests of the key side of the tss.go mirror (charon_amd/tbls.py:
split_secret, generate_tss, sign, partial_sign, combine_shares) and of
dkg.create_cluster_tss, over the engine's existing entry points (tbg_sk_to_pk,
tbg_sign, tbg_load_pubkeys, the verify / aggregate batches)."""
import random

import pytest

from charon_amd import dkg
from charon_amd import engine as eng
from charon_amd import tbls
from oracle import bls12_381 as bls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(0, slots=2)
    yield e
    e.close()


def test_generate_tss_matches_the_feldman_relation(engine):
    """The commitments are [a_j] g1, the pubshares are sum_j [i^j] C_j (the
    oracle's G1 arithmetic), the group key is C_0 and any t shares recover
    the secret."""
    rng = random.Random(21)
    tss, shares, secret = tbls.generate_tss(3, 4, rng, engine=engine)
    assert tss.threshold == 3 and tss.num_shares == 4 and len(tss.commitments) == 3
    assert tss.public_key.raw == tss.commitments[0] == bls.g1_compress(bls.g1_mul(bls.G1_GEN, secret))
    cs = [bls.g1_decompress(c) for c in tss.commitments]
    for s in shares:
        acc = None
        for j, c in enumerate(cs):
            acc = bls.g1_add(acc, bls.g1_mul(c, pow(s.identifier, j, bls.R)))
        assert tss.public_share(s.identifier).raw == bls.g1_compress(acc)
    assert tbls.combine_shares(shares[1:], 3, 4) == secret


def test_partial_signatures_aggregate_to_the_group_signature(engine):
    rng = random.Random(22)
    msg = b"tss parity"
    for t, n in ((2, 3), (3, 4), (7, 10)):
        tss, shares, secret = tbls.generate_tss(t, n, rng, engine=engine)
        parts = [tbls.partial_sign(s, msg, engine=engine) for s in shares]
        assert [p.identifier for p in parts] == list(range(1, n + 1))
        want = tbls.sign(secret, msg, engine=engine)
        sig, signers = tbls.verify_and_aggregate(tss, parts, msg, engine=engine)
        assert sig == want and signers == list(range(1, n + 1))
        assert tbls.aggregate(parts[n - t:], engine=engine) == want  # exactly t partials
        assert tbls.verify(tss.public_key, msg, sig, engine=engine)
        assert not tbls.verify(tss.public_share(1), msg, parts[1].signature, engine=engine)  # another share's partial
        with pytest.raises(tbls.TblsError, match="insufficient signatures"):
            tbls.verify_and_aggregate(tss, parts[:t - 1], msg, engine=engine)


def test_create_cluster_tss_leaves_the_pubshares_resident(engine):
    rng = random.Random(23)
    secrets = [rng.randrange(1, tbls.R) for _ in range(5)]
    before = engine.pubkey_count
    dvs, splits = dkg.create_cluster_tss(secrets, 3, 4, rng, engine=engine)
    assert engine.pubkey_count == before + 5 * 4 and len(dvs) == len(splits) == 5
    msgs = [b"duty %d" % d for d in range(5)]
    items = []
    for d, (tss, shares) in enumerate(zip(dvs, splits)):
        assert tbls.combine_shares(shares[:3], 3, 4) == secrets[d]
        assert tss.public_key.raw == bytes(engine.sk_to_pk(tbls._sk32(secrets[d]))[0])
        items += [(tss.public_share(s.identifier), msgs[d], tbls.partial_sign(s, msgs[d], engine=engine).signature)
                  for s in shares]
    assert tbls.verify_batch(items, engine=engine) == [True] * 20
    assert engine.pubkey_count == before + 20  # the verifies uploaded no key
