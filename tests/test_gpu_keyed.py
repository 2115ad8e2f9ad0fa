"""The hardened signer on the GPU: Engine.sk_to_pk_ct / sign_ct (tbg_sk_to_pk_ct,
tbg_sign_ct: fixed-schedule [sk]G1 and [sk]H(m), charon_amd/csrc/k_keyed.hip)
against the C oracle, the reference's known answers and the old entry points.

Item counts 1, 63, 64, 65 and 130: a lone lane, a partial wave, a full one, a
wave and one lane, and two waves and two lanes.  Every count of 63 and up
holds the whole list of tests/edge_scalars.py.
"""
import itertools
import random

import pytest

from charon_amd import engine as eng
from charon_amd import tbls
from oracle import c as oc
from tests import edge_scalars as es
from tests.test_oracle_kat import (DEPOSIT_GOLDEN, DEPOSIT_SKS, TEKU_SIG, TEKU_SK, deposit_signing_root,
                                   teku_signing_root)

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(0, slots=2)
    yield e
    e.close()


_PK, _SIG = {}, {}


def want_pk(k):
    if k not in _PK:
        _PK[k] = oc.sk_to_pk(k)
    return _PK[k]


def want_sig(k, msg):
    if (k, msg) not in _SIG:
        _SIG[(k, msg)] = oc.sign(k, msg)
    return _SIG[(k, msg)]


def scalars(n, first=0):
    """n scalars of the list, from position `first`, wrapping round."""
    return list(itertools.islice(itertools.cycle(es.VALID[first:] + es.VALID[:first]), n))


def keys32(ks):
    return b"".join(es.be32(k) for k in ks)


@pytest.mark.parametrize("n", COUNTS)
def test_sk_to_pk_ct_matches_the_oracle(engine, n):
    ks = scalars(n, first=n % len(es.VALID))
    pks, st = engine.sk_to_pk_ct(keys32(ks))
    assert st.tolist() == [es.KS_OK] * n
    for k, pk in zip(ks, pks):
        assert bytes(pk) == want_pk(k), hex(k)


def _messages(shape, n):
    """(distinct messages, item -> message)"""
    if shape == "one":
        return [b"one signing root for the whole ceremony"], [0] * n
    if shape == "each":
        return [b"root %d" % i for i in range(n)], list(range(n))
    msgs = [b"unsorted %d" % i for i in range(min(n, 5))]
    im = [(7 * i + 3) % len(msgs) for i in range(n)]
    random.Random(n).shuffle(im)
    return msgs, im


@pytest.mark.parametrize("shape", ["one", "each", "unsorted"])
@pytest.mark.parametrize("n", COUNTS)
def test_sign_ct_matches_the_oracle(engine, n, shape):
    ks = scalars(n, first=(3 * n) % len(es.VALID))
    msgs, im = _messages(shape, n)
    sigs, st = engine.sign_ct(keys32(ks), msgs, im)
    assert st.tolist() == [es.KS_OK] * n
    for k, m, sig in zip(ks, im, sigs):
        assert bytes(sig) == want_sig(k, msgs[m]), (hex(k), m)


def test_sign_ct_message_lengths(engine):
    """The empty message and the SHA-256 padding boundaries of expand_message
    (55, 56 and 64 bytes), every scalar of the list over each."""
    msgs = [b"", bytes(range(55)), bytes(range(56)), bytes(range(64))]
    ks = es.VALID
    im = [i % 4 for i in range(len(ks))]
    for rot in range(4):
        item_msg = [(m + rot) % 4 for m in im]
        sigs, st = engine.sign_ct(keys32(ks), msgs, item_msg)
        assert st.tolist() == [es.KS_OK] * len(ks)
        for k, m, sig in zip(ks, item_msg, sigs):
            assert bytes(sig) == want_sig(k, msgs[m]), (hex(k), len(msgs[m]))


def test_known_answers_of_the_reference(engine):
    """The four deposit keys and the Teku key of tests/test_oracle_kat.py:
    golden public keys and signatures."""
    sks = [int(s, 16) for s in DEPOSIT_SKS]
    pks, st = engine.sk_to_pk_ct(keys32(sks + [int(TEKU_SK, 16)]))
    assert st.tolist() == [es.KS_OK] * 5
    golden = {g[0]: g for g in DEPOSIT_GOLDEN}
    assert {bytes(pk).hex() for pk in pks[:4]} == set(golden)
    roots = [deposit_signing_root(golden[bytes(pk).hex()][2]) for pk in pks[:4]] + [teku_signing_root()]
    sigs, st = engine.sign_ct(keys32(sks + [int(TEKU_SK, 16)]), roots, list(range(5)))
    assert st.tolist() == [es.KS_OK] * 5
    for pk, sig in zip(pks[:4], sigs[:4]):
        assert bytes(sig).hex() == golden[bytes(pk).hex()][1]
    assert bytes(sigs[4]).hex() == TEKU_SIG


def _with_invalid(n):
    """n keys: the invalid scalars at scattered places of a wave, list scalars around them."""
    ks = scalars(n, first=11)
    want = [es.KS_OK] * n
    for pos, (k, code) in zip((0, 17, 31, n - 1), es.INVALID):
        ks[pos], want[pos] = k, code
    return ks, want


def test_invalid_scalars_are_refused_and_their_neighbours_unaffected(engine):
    n = 64
    ks, want = _with_invalid(n)
    pks, st = engine.sk_to_pk_ct(keys32(ks))
    assert st.tolist() == want
    msgs, im = _messages("unsorted", n)
    sigs, sst = engine.sign_ct(keys32(ks), msgs, im)
    assert sst.tolist() == want
    for i, (k, code) in enumerate(zip(ks, want)):
        if code == es.KS_OK:
            assert bytes(pks[i]) == want_pk(k) and bytes(sigs[i]) == want_sig(k, msgs[im[i]])
        else:
            assert not pks[i].any() and not sigs[i].any()


def test_agrees_with_the_old_entry_points(engine):
    rng = random.Random(0x300)
    ks = [rng.randrange(1, es.R) for _ in range(300)]
    msgs = [b"old and new %d" % i for i in range(7)]
    im = [rng.randrange(7) for _ in range(300)]
    pks, st = engine.sk_to_pk_ct(keys32(ks))
    sigs, sst = engine.sign_ct(keys32(ks), msgs, im)
    assert not st.any() and not sst.any()
    assert (pks == engine.sk_to_pk(keys32(ks))).all()
    assert (sigs == engine.sign(keys32(ks), msgs, im)).all()


def test_tbls_batch_functions(engine):
    k = es.VALID[-1]
    share = tbls.SecretKeyShare(3, es.VALID[-2])
    out = tbls.sign_batch([(k, b"m1"), (0, b"m1"), (es.R, b"m2"), (k, b"m2")], engine=engine)
    assert out[0].raw == want_sig(k, b"m1") and out[3].raw == want_sig(k, b"m2")
    assert isinstance(out[1], tbls.TblsError) and str(out[1]) == "unmarshal secret: secret key cannot be zero"
    assert isinstance(out[2], tbls.TblsError) and str(out[2]).startswith("unmarshal secret: ")
    parts = tbls.partial_sign_batch([(share, b"m1")], engine=engine)
    assert parts == [tbls.PartialSignature(3, tbls.Signature(want_sig(share.value, b"m1")))]
    assert tbls.sign(k, b"m1", engine=engine, hardened=True) == tbls.sign(k, b"m1", engine=engine)
    assert tbls.partial_sign(share, b"m1", engine=engine, hardened=True) == parts[0]
    with pytest.raises(tbls.TblsError, match="unmarshal secret"):
        tbls.sign(es.R + 1, b"m1", engine=engine, hardened=True)
    pks = tbls.secret_to_public_key_batch([k, 0], engine=engine)
    assert pks[0].raw == want_pk(k) and str(pks[1]) == "secret to pubkey: secret key cannot be zero"
    assert tbls.sign_batch([], engine=engine) == [] and tbls.secret_to_public_key_batch([], engine=engine) == []
