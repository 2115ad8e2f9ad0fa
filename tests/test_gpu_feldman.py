"""GPU tests of tbg_eval_commitments (k_feldman.hip, bls_feldman.h) and of what
stands on it: Engine.eval_commitments, tbls.new_tss / new_tss_batch /
pubshares_from_commitments_batch / feldman_verify_batch and
dkg.create_cluster_tss(from_commitments=True).

Expected points come from Python integers: [f(id) mod r] G1 through
oracle/bls12_381.py (tests/edge_feldman.py), and for the larger batches
through Engine.sk_to_pk of the host-computed f(id), the engine's existing and
independent 256-bit ladder."""
import ctypes
import random

import numpy as np
import pytest

from charon_amd import dkg
from charon_amd import engine as eng
from charon_amd import tbls
from tests import edge_decode as ed
from tests import edge_feldman as ef

pytestmark = pytest.mark.gpu

R = ef.R


@pytest.fixture(scope="module")
def engine():
    e = eng.Engine(0, slots=2)
    yield e
    e.close()


def sk_to_pk(engine, scalars):
    return [bytes(k) for k in engine.sk_to_pk(b"".join((v % R).to_bytes(32, "big") for v in scalars))]


def first_of(polys):
    return np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.uint32)


def test_directed_cases_in_one_launch(engine):
    L = ef.launch()
    assert len(L.eval_poly) > 64 and len(L.eval_poly) % 64 != 0
    out, st, cst = engine.eval_commitments(L.commit48, L.poly_first, L.eval_poly, L.eval_id)
    for k, (p, i) in enumerate(zip(L.eval_poly, L.eval_id)):
        assert int(st[k]) == L.want_status[k], (L.case_of_poly[p], i, int(st[k]))
        assert bytes(out[k]) == L.want_out[k], (L.case_of_poly[p], i)
    assert cst.tolist() == [1 if L.commit48[48 * j:48 * j + 48] == ef.IDENT48 else 0 for j in range(len(cst))]


def test_bad_commitment_encodings(engine):
    bad = [e for e in ed.g1_entries() if ed.g1_class(e.data)[0] < 0]
    assert {ed.g1_class(e.data)[0] for e in bad} == {ed.DEC_ERR_FLAGS, ed.DEC_ERR_FIELD, ed.DEC_ERR_NOT_ON_CURVE,
                                                      ed.DEC_ERR_SUBGROUP}
    good = ef.BY_NAME["generic_t3"].coeffs
    cs = ef.commits(good)
    polys, kind = [], []  # kind: None for a good polynomial, else (position, decode code) of its bad commitment
    for e in bad:
        code = ed.g1_class(e.data)[0]
        polys += [[e.data] + cs[1:], cs, [cs[0], e.data] + cs[2:]]
        kind += [(0, code), None, (1, code)]
    ids = [1, 2, 3]
    eval_poly = [p for i in ids for p in range(len(polys))]  # neighbouring lanes: bad, good, bad, ...
    eval_id = [i for i in ids for _ in polys]
    assert len(eval_poly) % 64 != 0
    out, st, cst = engine.eval_commitments(b"".join(c for p in polys for c in p), first_of(polys), eval_poly, eval_id)
    for k, (p, i) in enumerate(zip(eval_poly, eval_id)):
        if kind[p] is None:
            assert (int(st[k]), bytes(out[k])) == ef.expected(good, i), (p, i)
        else:
            assert int(st[k]) == eng.FV_COMMIT and bytes(out[k]) == ef.ZERO48, (p, i, int(st[k]))
    want_c = []
    for k in kind:
        row = [0, 0, 0]
        if k is not None:
            row[k[0]] = k[1]
        want_c += row
    assert cst.tolist() == want_c


def test_ragged_batch(engine):
    polys = ef.random_polys(300, [1, 2, 3, 7], seed=0xFE1D3)
    assert {len(p) for p in polys} == {1, 2, 3, 7}
    flat = sk_to_pk(engine, [a for p in polys for a in p])
    ev = [(p, i) for p in range(len(polys)) for i in range(1, 11)]
    out, st, cst = engine.eval_commitments(b"".join(flat), first_of(polys), [p for p, _ in ev], [i for _, i in ev])
    assert len(ev) == 3000 and not st.any() and not cst.any()
    want = sk_to_pk(engine, [ef.f(polys[p], i) for p, i in ev])
    assert [bytes(o) for o in out] == want
    sample = random.Random(5).sample(range(len(polys)), 48)
    for p in sample:
        assert flat[int(first_of(polys)[p])] == ef.commit(polys[p][0])
        for i in range(1, 11):
            assert bytes(out[10 * p + i - 1]) == ef.expected(polys[p], i)[1], (p, i)


def test_one_170_of_255_verifier(engine):
    coeffs = ef.BY_NAME["long_t170"].coeffs
    ids = list(range(1, 256))
    out, st, cst = engine.eval_commitments(b"".join(sk_to_pk(engine, coeffs)), [0, 170], [0] * 255, ids)
    assert not st.any() and not cst.any()
    assert [bytes(o) for o in out] == sk_to_pk(engine, [ef.f(coeffs, i) for i in ids])
    for i in (1, 2, 255):
        assert bytes(out[i - 1]) == ef.expected(coeffs, i)[1]


def test_new_tss_equals_generate_tss(engine):
    rng = random.Random(31)
    msg = b"new tss parity"
    for t, n in ((2, 3), (3, 4), (7, 10)):
        want, shares, secret = tbls.generate_tss(t, n, rng, engine=engine)
        tss = tbls.new_tss(want.commitments, n, engine=engine)
        assert tss.pubshares == want.pubshares and tss.public_key == want.public_key
        assert (tss.threshold, tss.num_shares, tss.commitments) == (t, n, want.commitments)
        assert tbls.pubshares_from_commitments_batch([want.commitments], n, engine=engine) == \
            [[want.pubshares[i].raw for i in range(1, n + 1)]]
        parts = [tbls.partial_sign(s, msg, engine=engine) for s in shares]
        sig, signers = tbls.verify_and_aggregate(tss, parts, msg, engine=engine)
        assert sig == tbls.sign(secret, msg, engine=engine) and signers == list(range(1, n + 1))


def test_new_tss_batch_errors(engine):
    c = ef.BY_NAME
    good = ef.commits(c["generic_t3"].coeffs)
    not_on_curve = next(e.data for e in ed.g1_entries() if ed.g1_class(e.data)[0] == ed.DEC_ERR_NOT_ON_CURVE)
    verifiers = [good, ef.commits(c["ident_c0"].coeffs), ef.commits(c["root_3"].coeffs), [good[0], not_on_curve],
                 ef.commits(c["ident_mid"].coeffs), [tbls.PublicKey(b) for b in good]]
    res = tbls.new_tss_batch(verifiers, 4, engine=engine)
    assert [str(r) if isinstance(r, Exception) else None for r in res] == [
        None, "unmarshal pubkey: public key is the identity", "unmarshal pubshare: public key is the identity",
        "unmarshal commitment: point is not on the curve", None, None]
    assert all(isinstance(r, tbls.TblsError) for r in res[1:4])
    assert res[0].pubshares == res[5].pubshares == {i: tbls.PublicKey(ef.expected(c["generic_t3"].coeffs, i)[1])
                                                    for i in range(1, 5)}
    assert res[4].threshold == 3 and res[4].commitments[1] == ef.IDENT48
    # two roots: fine below the first one, the first failing identifier decides
    assert len(tbls.new_tss(ef.commits(c["roots_2_5"].coeffs), 1, engine=engine).pubshares) == 1
    with pytest.raises(tbls.TblsError, match="unmarshal pubshare: public key is the identity"):
        tbls.new_tss(ef.commits(c["roots_2_5"].coeffs), 6, engine=engine)
    with pytest.raises(tbls.TblsError, match="unmarshal pubkey: public key is the identity"):
        tbls.new_tss(verifiers[1], 4, engine=engine)


def test_feldman_verify_batch(engine):
    rng = random.Random(32)
    shares, commits = tbls.split_secret(rng.randrange(1, R), 3, 5, rng, engine=engine)
    assert tbls.feldman_verify_batch([(commits, s) for s in shares], engine=engine) == [True] * 5
    S = tbls.SecretKeyShare
    not_in_field = next(e.data for e in ed.g1_entries() if ed.g1_class(e.data)[0] == ed.DEC_ERR_FIELD)
    items = [(commits, shares[0]),
             (commits, S(2, shares[0].value)),                 # another identifier
             (commits, S(1, (shares[0].value + 1) % R)),       # off by one
             (commits, S(3, 0)), (commits, S(3, R)),           # zero, out of range
             ([commits[0], not_in_field, commits[2]], shares[1]),
             (commits, shares[4]),
             (commits, S(3, 1 << 256))]
    res = tbls.feldman_verify_batch(items, engine=engine)
    assert res[:5] == [True, False, False, False, False] and res[6:] == [True, False]
    assert isinstance(res[5], tbls.TblsError) and str(res[5]) == "unmarshal commitment: invalid bytes - not in field"
    # a root of the polynomial: the public side is the identity, which no share value maps to
    root = ef.BY_NAME["root_3"].coeffs
    assert tbls.feldman_verify_batch([(ef.commits(root), S(3, 1)), (ef.commits(root), S(4, ef.f(root, 4)))],
                                     engine=engine) == [False, True]


@pytest.mark.parametrize("hardened", [False, True])
def test_create_cluster_tss_from_commitments(engine, hardened):
    seed = 33 + int(hardened)
    rng = random.Random(seed)
    secrets = [rng.randrange(1, R) for _ in range(5)]
    before = engine.pubkey_count
    dvs, splits = dkg.create_cluster_tss(secrets, 3, 4, random.Random(seed), engine=engine, hardened=hardened,
                                         from_commitments=True)
    after = engine.pubkey_count
    assert after == before + 5 * 4  # the pubshares are resident
    want_dvs, want_splits = dkg.create_cluster_tss(secrets, 3, 4, random.Random(seed), engine=engine, hardened=hardened)
    assert dvs == want_dvs and splits == want_splits
    assert engine.pubkey_count == after  # the default path found every one of its pubshares resident already


def test_argument_errors_and_empty_input(engine):
    cs = b"".join(ef.commits(ef.BY_NAME["generic_t3"].coeffs) + ef.commits(ef.BY_NAME["t1"].coeffs))
    ok = engine.eval_commitments(cs, [0, 3, 4], [0, 1], [1, 1])
    assert ok[1].tolist() == [0, 0]
    for first, poly in (([1, 3, 4], [0]),      # poly_first[0] != 0
                        ([0, 3, 2, 4], [0]),   # poly_first decreases
                        ([0, 3, 3, 4], [0]),   # an empty polynomial
                        ([0, 3, 4], [2]),      # eval_poly[e] >= n_polys
                        ([0, 3, 4], [0, 0xFFFFFFFF])):
        with pytest.raises(eng.EngineError, match=r"\(-1\)"):
            engine.eval_commitments(cs, first, poly, [1] * len(poly))
    # required pointers, through the C ABI
    lib, h = engine._lib, engine._h
    a = np.frombuffer(cs, dtype=np.uint8).copy()
    pf, ep, ei = np.array([0, 3, 4], np.uint32), np.array([0], np.uint32), np.array([1], np.uint32)
    out, st = np.zeros(48, np.uint8), np.zeros(1, np.int32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    args = [p(a), p(pf), 2, p(ep), p(ei), 1, p(out), p(st), None]
    assert lib.tbg_eval_commitments(h, *args) == 0 and st[0] == 0  # commit_status is optional
    for k in (0, 1, 3, 4, 6, 7):
        bad = list(args)
        bad[k] = None
        assert lib.tbg_eval_commitments(h, *bad) == eng.E_INVALID_ARG, k
    assert lib.tbg_eval_commitments(None, *args) == eng.E_INVALID_ARG
    # nothing to evaluate: OK, outputs untouched
    out[:] = 0xAA
    assert lib.tbg_eval_commitments(h, p(a), p(pf), 2, None, None, 0, None, None, None) == 0
    assert lib.tbg_eval_commitments(h, None, None, 0, None, None, 0, None, None, None) == 0
    assert (out == 0xAA).all()
    e_out, e_st, e_cst = engine.eval_commitments(cs, [0, 3, 4], [], [])
    assert e_out.shape == (0, 48) and e_st.shape == (0,)
