"""GPU tests of tbg_split_secret_ct / tbg_combine_shares_ct (k_shares.hip,
bls_frct.h) and of what stands on them: Engine.split_secret_ct /
combine_shares_ct, tbls.split_secret_batch / generate_tss_batch /
combine_shares_batch and dkg.create_cluster_tss(device_split=True).

Every check is exact: bytes equal, statuses equal.  Expected shares come from
tbls._split_host (Python integers), expected points from
oracle/bls12_381.g1_mul, expected secrets from tbls.combine_shares and from
the split's own coefficient 0; the pubshares are checked a second time
against tbg_eval_commitments of the commitments (tbls.new_tss)."""
import ctypes
import itertools
import random

import numpy as np
import pytest

from charon_amd import dkg
from charon_amd import engine as eng
from charon_amd import tbls
from oracle import bls12_381 as bls
from tests import edge_scalars as es

pytestmark = pytest.mark.gpu

R = es.R
POOL = list(es.VALID)  # (1 and r - 1 are among them)
assert 1 in POOL and R - 1 in POOL
ZERO32, ZERO48 = bytes(32), bytes(48)


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(0, slots=2)
    yield e
    e.close()


class Fixed:
    """An rng that hands out a given list (tbls._split_host draws with randrange)."""

    def __init__(self, vals):
        self.vals = list(vals)

    def randrange(self, lo, hi):
        return self.vals.pop(0)


def poly(k, t):
    """Polynomial k of threshold t over the edge scalars."""
    return [POOL[(7 * k + 3 * j + t) % len(POOL)] for j in range(t)]


def first_of(polys):
    return np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.uint32)


def coef_bytes(polys):
    return b"".join(int(c).to_bytes(32, "big") for p in polys for c in p)


def g1(k):
    return bls.g1_compress(bls.g1_mul(bls.G1_GEN, k))


def check_split(engine, polys, n, out, skip=()):
    """The outputs of one call against Python integers and the oracle, for the polynomials not in skip."""
    shares, commits, pub, st = out
    first = first_of(polys)
    for k, p in enumerate(polys):
        if k in skip:
            continue
        assert int(st[k]) == eng.SH_OK, (k, int(st[k]))
        want, _ = tbls._split_host(p[0], len(p), n, Fixed(p[1:]))
        for i, s in enumerate(want):
            assert bytes(shares[k * n + i]) == es.be32(s.value), (k, i)
            if pub is not None:
                assert bytes(pub[k * n + i]) == g1(s.value), (k, i)
        for j, c in enumerate(p):
            assert bytes(commits[first[k] + j]) == g1(c), (k, j)


def test_split_65_polynomials_of_mixed_thresholds(engine):
    n = 10
    polys = [poly(k, (2, 3, 7, 10, 5)[k % 5]) for k in range(65)]
    assert len(polys) * n > 64 * 10 and len({len(p) for p in polys}) == 5
    out = engine.split_secret_ct(coef_bytes(polys), first_of(polys), n)
    check_split(engine, polys, n, out)
    # the pubshares are the commitment polynomials at 1..n (tbg_eval_commitments), and tbls.new_tss agrees
    shares, commits, pub, st = out
    first = first_of(polys)
    ev, est, _ = engine.eval_commitments(commits.tobytes(), first, [k for k in range(65) for _ in range(n)],
                                         [i for _ in range(65) for i in range(1, n + 1)])
    assert (est == eng.FV_OK).all() and (ev == pub).all()
    for k in (0, 3, 64):
        tss = tbls.new_tss([bytes(c) for c in commits[first[k]:first[k + 1]]], n, engine=engine)
        assert [tss.public_share(i).raw for i in range(1, n + 1)] == [bytes(pk) for pk in pub[k * n:(k + 1) * n]]
        assert tss.threshold == len(polys[k]) and tss.public_key.raw == g1(polys[k][0])


@pytest.mark.parametrize("t,n,count", [(2, 2, 3), (3, 4, 3), (7, 10, 2), (255, 255, 1)])
def test_split_shapes(engine, t, n, count):
    polys = [poly(11 * k + t, t) for k in range(count)]
    out = engine.split_secret_ct(coef_bytes(polys), first_of(polys), n)
    check_split(engine, polys, n, out)
    tss = tbls.new_tss([bytes(c) for c in out[1][:t]], n, engine=engine)
    assert [tss.public_share(i).raw for i in range(1, n + 1)] == [bytes(pk) for pk in out[2][:n]]


def failure_launch():
    """Refused polynomials between good ones, n = 4: (polynomials, expected status per polynomial)."""
    a = POOL[25]
    good = [poly(k, t) for k, t in ((1, 3), (2, 2), (3, 4), (4, 3), (5, 2), (6, 3))]
    bad = [([0, POOL[3], POOL[4]], eng.SH_COEF_ZERO),               # the secret is zero
           ([POOL[5], POOL[6], 0], eng.SH_COEF_ZERO),               # coefficient t - 1 is zero
           ([POOL[7], R], eng.SH_COEF_RANGE),
           ([(1 << 256) - 1, POOL[8], POOL[9]], eng.SH_COEF_RANGE),
           ([POOL[10], R + 1, 0], eng.SH_COEF_RANGE),               # the first refusal by index counts
           ([R - a, a], eng.SH_SHARE_ZERO)]                         # f(1) = 0
    polys, want = [], []
    for g, (b, code) in zip(good, bad):
        polys += [g, b]
        want += [eng.SH_OK, code]
    return polys, want


@pytest.mark.parametrize("pubshares", [True, False])
def test_split_directed_failures_beside_good_polynomials(engine, pubshares):
    n = 4
    polys, want = failure_launch()
    first = first_of(polys)
    out = engine.split_secret_ct(coef_bytes(polys), first, n, pubshares=pubshares)
    shares, commits, pub, st = out
    assert st.tolist() == want
    assert (pub is None) == (not pubshares)
    skip = {k for k, w in enumerate(want) if w != eng.SH_OK}
    check_split(engine, polys, n, out, skip=skip)
    for k in skip:  # a failed polynomial has all its outputs zero
        assert not shares[k * n:(k + 1) * n].any() and not commits[first[k]:first[k + 1]].any()
        assert pub is None or not pub[k * n:(k + 1) * n].any()
    if not pubshares:  # the same shares and commitments as with pubshares
        full = engine.split_secret_ct(coef_bytes(polys), first, n)
        assert (full[0] == shares).all() and (full[1] == commits).all() and (full[3] == st).all()


def test_split_argument_errors_launch_nothing(engine):
    lib, h = engine._lib, engine._h
    coef = np.frombuffer(coef_bytes([poly(0, 2), poly(1, 3)]), np.uint8).copy()
    sh, cm, pb = np.zeros((8, 32), np.uint8), np.zeros((5, 48), np.uint8), np.zeros((8, 48), np.uint8)
    st = np.full(2, 77, np.int32)
    p = eng._ptr

    def call(coef_p=p(coef), first=(0, 2, 5), n_polys=2, n=4, sh_p=p(sh), cm_p=p(cm), pb_p=p(pb), st_p=p(st)):
        f = np.array(first, dtype=np.uint32)
        return lib.tbg_split_secret_ct(h, coef_p, p(f), n_polys, n, sh_p, cm_p, pb_p, st_p)

    assert call() == 0 and st.tolist() == [0, 0]
    st[:] = 77
    for kw in (dict(coef_p=None), dict(sh_p=None), dict(cm_p=None), dict(st_p=None), dict(first=(1, 2, 5)),
               dict(first=(0, 3, 2)), dict(n=0), dict(n=256), dict(first=(0, 1, 5)), dict(first=(0, 5, 7), n=4),
               dict(first=(0, 2, 5), n=2)):
        assert call(**kw) == eng.E_INVALID_ARG, kw
    assert lib.tbg_split_secret_ct(None, p(coef), p(np.array([0, 2, 5], np.uint32)), 2, 4, p(sh), p(cm), p(pb), p(st)) == \
        eng.E_INVALID_ARG
    assert st.tolist() == [77, 77]  # (a refused call writes nothing)
    assert call(n_polys=0, coef_p=None, sh_p=None, cm_p=None, st_p=None) == 0  # nothing to do: TBG_OK
    with pytest.raises(eng.EngineError):
        engine.split_secret_ct(coef.tobytes(), [0, 2, 5], 2)  # t = 3 > n = 2 through the binding


# ---- combine ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def splits():
    """Host splits shared by the combine tests: (secret, t, n, shares)."""
    rng = random.Random(0x5A7E)
    out = {}
    for t, n in ((3, 4), (2, 255), (7, 10), (255, 255)):
        secret = POOL[(t + n) % len(POOL)]
        out[(t, n)] = (secret, t, n, tbls._split_host(secret, t, n, rng)[0])
    return out


def combine(engine, sets):
    """sets: lists of SecretKeyShare -> (secrets as int, statuses) of ONE call."""
    first = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.uint32)
    out, st = engine.combine_shares_ct(b"".join(int(x.value).to_bytes(32, "big") for s in sets for x in s),
                                       [x.identifier for s in sets for x in s], first)
    return [int.from_bytes(bytes(o), "big") for o in out], st.tolist()


def test_combine_subsets_and_identifier_orders(engine, splits):
    secret, t, n, shares = splits[(3, 4)]
    sets = [list(c) for c in itertools.combinations(shares, 3)] + [list(shares), list(reversed(shares)),
                                                                   [shares[2], shares[0], shares[3]]]
    s2, _, _, sh2 = splits[(2, 255)]
    sets.append([sh2[253], sh2[254]])   # identifiers {254, 255}
    sets.append([sh2[254], sh2[0]])
    got, st = combine(engine, sets)
    assert st == [eng.SH_OK] * len(sets)
    want = [secret] * 7 + [s2] * 2
    assert got == want
    for s, w in zip(sets, want):
        assert tbls.combine_shares(s, 2, 255) == w


def test_combine_all_255_shares(engine, splits):
    secret, t, n, shares = splits[(255, 255)]
    mixed = list(shares)
    random.Random(3).shuffle(mixed)
    got, st = combine(engine, [shares, mixed])
    assert st == [eng.SH_OK] * 2 and got == [secret, secret]


def test_combine_65_sets_in_one_call_and_the_group_key(engine, splits):
    secret, t, n, shares = splits[(7, 10)]
    rng = random.Random(65)
    polys = [poly(k, 3) for k in range(32)]
    sh, commits, _, st = engine.split_secret_ct(coef_bytes(polys), first_of(polys), 4, pubshares=False)
    assert (st == eng.SH_OK).all()
    sets, want, key = [], [], []
    for k in range(65):
        if k % 2:
            sets.append(rng.sample(shares, 7 + k % 4))
            want.append(secret)
            key.append(None)
        else:  # the device's own split, recombined from three of its four shares
            d = k // 2 % 32
            pick = rng.sample(range(4), 3)
            sets.append([tbls.SecretKeyShare(i + 1, int.from_bytes(bytes(sh[4 * d + i]), "big")) for i in pick])
            want.append(polys[d][0])
            key.append(bytes(commits[3 * d]))
    got, cst = combine(engine, sets)
    assert cst == [eng.SH_OK] * 65 and got == want
    pks, kst = engine.sk_to_pk_ct(b"".join(es.be32(s) for s in got))
    assert (kst == eng.KS_OK).all()
    for pk, c0 in zip(pks, key):  # [secret] G1 == commitment 0
        assert c0 is None or bytes(pk) == c0


def test_combine_directed_failures_beside_good_sets(engine, splits):
    secret, t, n, shares = splits[(3, 4)]
    S = tbls.SecretKeyShare
    a = POOL[30]

    class Raw:  # a share the mirror's class would refuse (identifier 0, value >= r)
        def __init__(self, identifier, value):
            self.identifier, self.value = identifier, value

    good = shares[:3]
    cases = [([shares[0]], eng.SH_TOO_FEW),
             ([], eng.SH_TOO_FEW),
             ([shares[0], Raw(0, shares[1].value), shares[2]], eng.SH_ID),
             ([shares[0], shares[1], S(1, shares[2].value)], eng.SH_DUPLICATE_ID),
             ([shares[0], Raw(2, 0), shares[2]], eng.SH_VALUE_ZERO),
             ([shares[0], shares[1], Raw(3, R)], eng.SH_VALUE_RANGE),
             ([Raw(1, (1 << 256) - 1), Raw(2, 0), shares[2]], eng.SH_VALUE_RANGE),   # the first by index
             ([Raw(0, 0), Raw(0, R)], eng.SH_ID),                                    # public reasons first
             ([S(i, a * i % R) for i in (5, 2, 200)], eng.SH_SECRET_ZERO)]           # f(x) = a x
    sets, want = [good], [eng.SH_OK]
    for c, code in cases:
        sets += [c, good[::-1]]
        want += [code, eng.SH_OK]
    got, st = combine(engine, sets)
    assert st == want
    assert got == [secret if w == eng.SH_OK else 0 for w in want]


def test_combine_argument_errors(engine):
    lib, h, p = engine._lib, engine._h, eng._ptr
    val, ids = np.zeros((2, 32), np.uint8), np.array([1, 2], np.uint8)
    val[:, 31] = 9
    out, st = np.zeros((1, 32), np.uint8), np.full(1, 77, np.int32)
    ok = np.array([0, 2], np.uint32)
    assert lib.tbg_combine_shares_ct(h, p(val), p(ids), p(ok), 1, p(out), p(st)) == 0 and st[0] == eng.SH_OK
    assert int.from_bytes(bytes(out[0]), "big") == 9  # the constant polynomial
    for args in ((None, p(ids), p(ok), 1, p(out), p(st)), (p(val), None, p(ok), 1, p(out), p(st)),
                 (p(val), p(ids), None, 1, p(out), p(st)), (p(val), p(ids), p(ok), 1, None, p(st)),
                 (p(val), p(ids), p(ok), 1, p(out), None), (p(val), p(ids), p(np.array([1, 2], np.uint32)), 1, p(out), p(st)),
                 (p(val), p(ids), p(np.array([0, 2, 1], np.uint32)), 2, p(out), p(st))):
        assert lib.tbg_combine_shares_ct(h, *args) == eng.E_INVALID_ARG
    assert lib.tbg_combine_shares_ct(None, p(val), p(ids), p(ok), 1, p(out), p(st)) == eng.E_INVALID_ARG
    assert lib.tbg_combine_shares_ct(h, None, None, None, 0, None, None) == 0


# ---- the mirror ------------------------------------------------------------------------------

def test_split_secret_batch_equals_sequential_split_secret(engine):
    items = [(POOL[k], t) for k, t in ((20, 3), (21, 2), (22, 4), (23, 3))]
    seq_rng, rng = random.Random(0xBA7C), random.Random(0xBA7C)
    seq = [tbls.split_secret(s, t, 4, seq_rng, engine=engine) for s, t in items]
    got = tbls.split_secret_batch(items + [(5, 1)], 4, rng, engine=engine)
    assert isinstance(got[-1], tbls.TblsError) and "new Feldman VSS" in str(got[-1])
    for (shares, commits), (g_shares, g_commits, g_pub) in zip(seq, got):
        assert g_shares == shares and g_commits == commits
        assert g_pub == [g1(s.value) for s in shares]
    assert seq_rng.random() == rng.random()  # the same draws were consumed
    refused = tbls.split_secret_batch([(0, 2), (R, 2), (POOL[1], 2)], 2, random.Random(1), engine=engine)
    assert str(refused[0]).startswith("split Secret Key: ") and str(refused[1]).startswith("convert to scaler: ")
    assert not isinstance(refused[2], Exception)
    a = POOL[9]
    zero_share = tbls.split_secret_batch([(R - a, 2)], 2, Fixed([a]), engine=engine)[0]
    assert str(zero_share).startswith("unmarshalling shamir share: ")


def test_generate_tss_batch_equals_sequential_generate_tss(engine):
    seq_rng, rng = random.Random(0x6E4), random.Random(0x6E4)
    seq = [tbls.generate_tss(3, 4, seq_rng, engine=engine, hardened=True) for _ in range(5)]
    got = tbls.generate_tss_batch(5, 3, 4, rng, engine=engine)
    assert len(got) == 5
    for (tss, shares, secret), (g_tss, g_shares, g_secret) in zip(seq, got):
        assert g_secret == secret and g_shares == shares and g_tss == tss
    assert seq_rng.random() == rng.random()


def test_combine_shares_batch(engine, splits):
    secret, t, n, shares = splits[(3, 4)]
    s7, _, _, sh7 = splits[(7, 10)]
    line = [tbls.SecretKeyShare(i, 11 * i) for i in (1, 2, 3)]
    got = tbls.combine_shares_batch([(shares[1:], 3, 4), (shares[:2], 3, 4), (sh7[2:], 7, 10), (line, 3, 4),
                                     ([shares[0], tbls.SecretKeyShare(2, 0), shares[2]], 3, 4)], engine=engine)
    assert got[0] == secret == tbls.combine_shares(shares[1:], 3, 4) and got[2] == s7
    assert str(got[1]) == "combine shares: fewer shares than the threshold"
    assert str(got[3]).startswith("unmarshal secret: ") and str(got[4]).startswith("combine shares: ")


def test_device_split_ceremony_equals_the_hardened_one_and_signs(engine):
    rng = random.Random(0xD4)
    secrets = [rng.randrange(1, R) for _ in range(3)]
    dvs_h, splits_h = dkg.create_cluster_tss(secrets, 3, 4, random.Random(0xD5), engine=engine, hardened=True)
    dvs, splits_d = dkg.create_cluster_tss(secrets, 3, 4, random.Random(0xD5), engine=engine, device_split=True)
    assert splits_d == splits_h
    for a, b in zip(dvs, dvs_h):
        assert a.public_key == b.public_key and a.commitments == b.commitments and a.pubshares == b.pubshares
        assert (a.num_shares, a.threshold) == (b.num_shares, b.threshold) == (4, 3)
    # partials signed with the device-split shares verify and aggregate under the group key
    msg = b"signed with device-split shares"
    for tss, shares, secret in zip(dvs, splits_d, secrets):
        parts = tbls.partial_sign_batch([(s, msg) for s in shares[1:]], engine=engine)
        assert not any(isinstance(x, Exception) for x in parts)
        sig, signers = tbls.verify_and_aggregate(tss, parts, msg, engine=engine)
        assert signers == [2, 3, 4]
        assert tbls.verify(tss.public_key, msg, sig, engine=engine)
        assert sig == tbls.sign(secret, msg, engine=engine, hardened=True)
    with pytest.raises(tbls.TblsError):
        dkg.create_cluster_tss([0], 3, 4, random.Random(1), engine=engine, device_split=True)
