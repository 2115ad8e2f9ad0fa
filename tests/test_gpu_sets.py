"""GPU tests of the all-or-nothing set verification (tbg_submit_sets,
k_sets.hip): per set, whether every member verifies, with no narrowing of a
failed set.

Expected verdicts are f() over the per-partial statuses that TBG_OP_VERIFY
gives the same input (the existing suite pins that run to oracle/c; the small
batch is also compared with oracle/c directly here):
  SS_ERROR    some member has a negative TBG_PS_* code,
  SS_INVALID  none has, and some member's pairing check is false,
  SS_VALID    every member is PS_VALID (an empty set too).
partial_status: negative codes exact; a candidate is PS_VALID if its set is
VALID, else PS_NOT_VERIFIED."""
import dataclasses
import functools
import json
import os

import numpy as np
import pytest

from charon_amd import engine as eng
from charon_amd import parsig, signing, tbls
from charon_amd.parsig import Duty, ParSignedData

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SMALL_SETS = (1, 15, 16, 17, 0, 33, 1, 37)  # duties per set: 120 duties, 480 partials
N_SMALL = sum(SMALL_SETS)
SCHEDULES = {
    "l0_on": dict(rlc_batch=eng.RLC_L0_ON),
    "l0_off_g4": dict(rlc_batch=eng.RLC_L0_OFF, rlc_group=4),
    "l0_off_g16": dict(rlc_batch=eng.RLC_L0_OFF, rlc_group=16),
    "each": dict(verify_mode=eng.VERIFY_EACH),
}


_ENGINES = {}


def _engine(name):
    if name not in _ENGINES:
        _ENGINES[name] = eng.Engine(0, slots=2, **SCHEDULES[name])
    return _ENGINES[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    for cached in (_small, _large, _boundary_case, _cancelling):
        cached.cache_clear()


def _load_everywhere(b):
    """The batch's pubshares under the same ids in every schedule's engine."""
    for name in SCHEDULES:
        if name == "l0_on":
            continue  # (generated there)
        first, st = _engine(name).load_pubkeys(b.pubshares)
        assert first == b.pk_first and (st == 0).all()


def _wrong_sigs(e, b):
    """Every partial's signature over a wrong message (same share)."""
    sk32 = b"".join(s.to_bytes(32, "big") for s in b.shares)
    wrong = [m[:-1] + bytes([m[-1] ^ 0xFF]) for m in b.msgs]
    return e.sign(sk32, wrong, np.repeat(b.duty_msg, b.n).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def _small():
    """120 clean 3-of-4 duties (below 2,048 partials: every signature tested
    alone, level 0 by the bucket MSM) and their wrong-message signatures."""
    from tools.workload import make_batch
    e = _engine("l0_on")
    assert e.pubkey_count == 0
    b = make_batch(e, N_SMALL, 3, 4, seed=71)
    wrong = _wrong_sigs(e, b)
    _load_everywhere(b)
    return b, wrong


@functools.lru_cache(maxsize=None)
def _large():
    """700 clean duties (2,800 partials: batched subgroup test, fused level 0),
    loaded after the small batch's keys in the level-0 engine."""
    from tools.workload import make_batch
    _small()
    e = _engine("l0_on")
    b = make_batch(e, 700, 3, 4, seed=72)
    return b, _wrong_sigs(e, b)


def _set_first(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)


def _args(b, sigs=None, pubkey_ids=None):
    return dict(duty_first=b.duty_first, sigs=b.sigs if sigs is None else sigs, identifiers=b.identifiers,
                msgs=(b.msg_data, b.msg_off), duty_msg=b.duty_msg,
                pubkey_ids=b.pubkey_ids if pubkey_ids is None else pubkey_ids)


def f_sets(ps, duty_first, set_first):
    """f(set) of the module docstring over TBG_OP_VERIFY's per-partial statuses."""
    out = []
    for k in range(len(set_first) - 1):
        m = ps[int(duty_first[set_first[k]]):int(duty_first[set_first[k + 1]])]
        out.append(eng.SS_ERROR if (m < 0).any() else eng.SS_INVALID if (m != eng.PS_VALID).any() else eng.SS_VALID)
    return np.array(out, dtype=np.int32)


def expect_partials(ps, ss, duty_first, set_first):
    exp = ps.copy()
    for k in range(len(set_first) - 1):
        lo, hi = int(duty_first[set_first[k]]), int(duty_first[set_first[k + 1]])
        cand = exp[lo:hi] >= 0
        exp[lo:hi][cand] = eng.PS_VALID if ss[k] == eng.SS_VALID else eng.PS_NOT_VERIFIED
    return exp


def _reference(b, sigs, pubkey_ids=None):
    """TBG_OP_VERIFY's per-partial statuses of the same input (per-partial schedule)."""
    return _engine("each").run(eng.OP_VERIFY, **_args(b, sigs, pubkey_ids)).partial_status


def _check(name, b, sizes, sigs, ref_ps, pubkey_ids=None):
    e = _engine(name)
    sf = _set_first(sizes)
    t = e.submit_sets(sf, **_args(b, sigs, pubkey_ids))
    res = e.collect_sets(t)
    want = f_sets(ref_ps, b.duty_first, sf)
    print(name, "set_status", res.set_status.tolist(), "want", want.tolist(), "fallback", e.fallback(t))
    assert res.set_status.tolist() == want.tolist()
    assert np.array_equal(res.partial_status, expect_partials(ref_ps, want, b.duty_first, sf))
    return t, res, want


# ------------------------------------------------------------ 1. fixture parity
def test_fixture_parity_with_verify_sets():
    with open(os.path.join(HERE, "golden", "parsig_sets.json")) as fh:
        fx = json.load(fh)
    assert len(fx["sets"]) == 16
    e = eng.Engine(0)
    try:
        spec = signing.Spec(forks=[(ep, bytes.fromhex(v)) for ep, v in fx["forks"]],
                            genesis_validators_root=bytes.fromhex(fx["genesis_validators_root"]))
        pubshares = {d["pubkey"]: {int(k): tbls.PublicKey(bytes.fromhex(v)) for k, v in d["pubshares"].items()}
                     for d in fx["dvs"]}
        v = parsig.Eth2Verifier(spec, pubshares, e)
        sets = [(Duty(s["slot"], s["duty_type"]),
                 {it["pubkey"]: ParSignedData(it["domain"], it["epoch"], bytes.fromhex(it["message_root"]),
                                              bytes.fromhex(it["sig"]), it["share_idx"]) for it in s["items"]})
                for s in fx["sets"]]
        plain = v.verify_sets(sets)
        drop = v.verify_sets_drop(sets)
        assert any(r is None for r in plain) and any(r is not None for r in plain)
        for s, a, d in zip(fx["sets"], plain, drop):
            assert (d is None) == (a is None), (s["fault"], a, d)
            assert (d is None) == (s["expect_error"] is None)
            if s["fault"] in ("zero_signature", "bad_share_idx"):
                assert str(d) == str(a), s["fault"]  # host-detected: today's message
            elif d is not None and s["expect_error"] in ("invalid signature", "uncompress sig"):
                assert str(d) == f"invalid signature: set failed verification (duty={Duty(s['slot'], s['duty_type'])})"
        assert {"zero_signature", "bad_share_idx"} <= {s["fault"] for s in fx["sets"]}
        # the receive loop forwards the same sets either way
        got = {False: [], True: []}
        for mode in (False, True):
            ex = parsig.ParSigEx(v, drop_only=mode)
            ex.subscribe(lambda duty, pset, mode=mode: got[mode].append((duty, sorted(pset))))
            ex.handle_batch(sets)
        assert got[True] == got[False] and got[True]
    finally:
        e.close()


# ------------------------------------------------------------ 2. boundary shapes
_SF = _set_first(SMALL_SETS)
BAD_PARTIALS = {
    "first_of_set": 4 * int(_SF[3]),                 # first partial of the 17-duty set
    "last_of_set": 4 * int(_SF[2]) - 1,              # last partial of the 15-duty set
    "last_partial_group": 4 * (int(_SF[6]) - 1) + 1,  # the 33-duty set's last duty: a partly filled group at G = 4 and 16
    "one_duty_set": 4 * int(_SF[6]) + 2,             # the 1-duty set after it
}
BAD_SET = {"first_of_set": 3, "last_of_set": 1, "last_partial_group": 5, "one_duty_set": 6}


@functools.lru_cache(maxsize=None)
def _boundary_case(case):
    b, wrong = _small()
    sigs = b.sigs.copy()
    p = BAD_PARTIALS[case]
    sigs[p] = wrong[p]
    ref = _reference(b, sigs)
    assert np.flatnonzero(ref != eng.PS_VALID).tolist() == [p] and ref[p] == eng.PS_INVALID
    # the small batch directly against oracle/c
    from tests.test_gpu_fullsize import oracle_run
    ops, _, _ = oracle_run(dataclasses.replace(b, sigs=sigs))
    assert np.array_equal(ref, ops)
    return sigs, ref


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("case", list(BAD_PARTIALS))
def test_boundary_shapes_only_the_bad_set_fails(case, schedule):
    b, _ = _small()
    sigs, ref = _boundary_case(case)
    _, res, want = _check(schedule, b, SMALL_SETS, sigs, ref)
    expect = [eng.SS_VALID] * len(SMALL_SETS)
    expect[BAD_SET[case]] = eng.SS_INVALID
    assert res.set_status.tolist() == expect == want.tolist()  # clean neighbours VALID: no group straddles a set


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_clean_small_sets_all_valid(schedule):
    b, _ = _small()
    ref = np.full(4 * N_SMALL, eng.PS_VALID, dtype=np.int32)
    t, res, _ = _check(schedule, b, SMALL_SETS, b.sigs, ref)
    assert (res.set_status == eng.SS_VALID).all()
    if schedule == "l0_on":
        assert _engine(schedule).level0(t) == eng.L0_PASSED


# ------------------------------------------------------------ 3. larger batch
LARGE_SETS = (50,) * 14


def test_large_clean_batch_passes_level0():
    b, _ = _large()
    e = _engine("l0_on")
    ref = np.full(2800, eng.PS_VALID, dtype=np.int32)
    t, res, _ = _check("l0_on", b, LARGE_SETS, b.sigs, ref)
    assert (res.set_status == eng.SS_VALID).all()
    assert e.level0(t) == eng.L0_PASSED
    assert e.subgroup(t)["groups"] > 0  # the batched subgroup test ran (level 0 took S from its sums)


def test_large_batch_every_injection_kind_in_its_own_set():
    from tools.workload import INJECT_KINDS, NO_PUBKEY, invalid_pool
    b, wrong = _large()
    _load_large_everywhere(b)
    pool = invalid_pool()
    rng = np.random.default_rng(5)
    sigs, ids = b.sigs.copy(), b.pubkey_ids.copy()
    hit = {}
    for k, kind in enumerate(INJECT_KINDS):
        s = 1 + k  # sets 1..8
        p = 4 * (50 * s + 7 * k % 50) + k % 4
        hit[kind] = s
        if kind == "wrong_msg":
            sigs[p] = wrong[p]
        elif kind == "wrong_share":
            sigs[p] = b.sigs[p + 1 if p % 4 < 3 else p - 1]
        elif kind == "random_bytes":
            sigs[p] = np.frombuffer(rng.bytes(96), dtype=np.uint8)
        elif kind in ("non_subgroup", "off_curve"):
            sigs[p] = np.frombuffer(pool[kind][0], dtype=np.uint8)
        elif kind == "bad_flags":
            sigs[p, 0] &= 0x7F
        elif kind == "identity":
            sigs[p] = 0
            sigs[p, 0] = 0xC0
        elif kind == "missing_pubshare":
            ids[p] = NO_PUBKEY
        else:
            raise AssertionError(kind)
    ref = _reference(b, sigs, ids)
    sf = _set_first(LARGE_SETS)
    want = f_sets(ref, b.duty_first, sf)
    bad_sets = sorted(hit.values())
    assert np.flatnonzero(want != eng.SS_VALID).tolist() == bad_sets
    assert want[hit["wrong_msg"]] == eng.SS_INVALID and want[hit["wrong_share"]] == eng.SS_INVALID
    assert want[hit["non_subgroup"]] == eng.SS_ERROR and want[hit["missing_pubshare"]] == eng.SS_ERROR
    for name in ("l0_on", "l0_off_g16"):
        _check(name, b, LARGE_SETS, sigs, ref, ids)


def _load_large_everywhere(b):
    for name in SCHEDULES:
        e = _engine(name)
        if name != "l0_on" and e.pubkey_count == 4 * N_SMALL:
            first, st = e.load_pubkeys(b.pubshares)
            assert first == b.pk_first and (st == 0).all()


# ------------------------------------------------------------ 4. no narrowing
def test_bad_set_is_not_narrowed():
    b, _ = _small()
    sigs, ref = _boundary_case("first_of_set")
    e = _engine("l0_off_g16")
    t, res, _ = _check("l0_off_g16", b, SMALL_SETS, sigs, ref)
    fb = e.fallback(t)
    assert fb["groups"] > 0 and fb["group_size"] == 16 and fb["level0"] == eng.L0_NOT_RUN
    assert (fb["group_searches"], fb["chunks"], fb["chunk_searches"], fb["duty_searches"]) == (0, 0, 0, 0)
    assert fb["partial_checks"] == 0
    # the premise: the same input through TBG_OP_VERIFY narrows the failed group
    t2 = e.submit(eng.OP_VERIFY, **_args(b, sigs))
    assert np.array_equal(e.collect(t2).partial_status, ref)
    assert e.fallback(t2)["chunks"] > 0


def test_bad_set_feeds_the_adaptive_state():
    """Every candidate of a failed group counts as invalid: level-0 AUTO
    switches off after a bad set launch, as it does after bad partials."""
    b, _ = _small()
    sigs, ref = _boundary_case("one_duty_set")
    e = eng.Engine(0, slots=2)
    try:
        first, st = e.load_pubkeys(b.pubshares)
        assert first == b.pk_first
        sf = _set_first(SMALL_SETS)
        t = e.submit_sets(sf, **_args(b))
        assert (e.collect_sets(t).set_status == eng.SS_VALID).all()
        assert e.shape(t)["level0"] == 1
        t = e.submit_sets(sf, **_args(b, sigs))
        assert e.collect_sets(t).set_status.tolist() == f_sets(ref, b.duty_first, sf).tolist()
        t = e.submit_sets(sf, **_args(b))
        assert (e.collect_sets(t).set_status == eng.SS_VALID).all()
        assert e.shape(t)["level0"] == 0
    finally:
        e.close()


# ------------------------------------------------------------ 5. cancelling errors
@functools.lru_cache(maxsize=None)
def _cancelling(da, db):
    """s_a + D on the first partial of duty da, s_b - D on that of duty db."""
    from oracle import bls12_381 as bls
    b, _ = _small()
    delta = bls.g2_mul(bls.G2_GEN, 0x1234567)
    sigs = b.sigs.copy()
    for d, pt in ((da, delta), (db, bls.g2_neg(delta))):
        s = bls.g2_add(bls.g2_decompress(bytes(sigs[4 * d])), pt)
        sigs[4 * d] = np.frombuffer(bls.g2_compress(s), dtype=np.uint8)
    ref = _reference(b, sigs)
    assert np.flatnonzero(ref != eng.PS_VALID).tolist() == [4 * da, 4 * db]
    return sigs, ref


@pytest.mark.parametrize("schedule", ["l0_on", "l0_off_g16", "l0_off_g4"])
@pytest.mark.parametrize("pair", ["one_group", "across_sets"])
def test_cancelling_errors_fail_their_sets(pair, schedule):
    b, _ = _small()
    # one set and one group (duties 33, 34 of the 17-duty set: its first group
    # at G = 4 and 16), or the last duty of one set and the first of the next
    da, db = (int(_SF[3]) + 1, int(_SF[3]) + 2) if pair == "one_group" else (int(_SF[2]) - 1, int(_SF[2]))
    sigs, ref = _cancelling(da, db)
    _, res, _ = _check(schedule, b, SMALL_SETS, sigs, ref)
    bad = {3} if pair == "one_group" else {1, 2}
    assert set(np.flatnonzero(res.set_status == eng.SS_INVALID).tolist()) == bad
    assert set(np.flatnonzero(res.set_status == eng.SS_VALID).tolist()) == set(range(len(SMALL_SETS))) - bad


# ------------------------------------------------------------ 6. ABI errors
def test_abi_errors_and_replay():
    import ctypes
    b, _ = _small()
    sigs, ref = _boundary_case("last_of_set")
    e = _engine("l0_off_g16")
    n = N_SMALL
    for bad in ([1, n], [0, 50, 30, n], [0, 60, n - 1], [0, 60, n + 1]):
        with pytest.raises(eng.EngineError, match=r"\(-1\)"):
            e.submit_sets(bad, **_args(b))
    # any other op
    batch, keep, _, _ = e._batch(eng.OP_VERIFY_AGGREGATE, duty_threshold=b.threshold, **_args(b))
    sf = _set_first(SMALL_SETS)
    tk = ctypes.c_uint64()
    rc = e._lib.tbg_submit_sets(e._h, ctypes.byref(batch), sf.ctypes.data_as(ctypes.c_void_p), len(sf) - 1,
                                ctypes.byref(tk))
    assert rc == eng.E_INVALID_ARG
    # a plain ticket is no set ticket, and the other way round
    plain = e.submit(eng.OP_VERIFY, **_args(b, sigs))
    assert e._lib.tbg_collect_sets(e._h, plain, None, None, 1) == eng.E_TICKET
    assert np.array_equal(e.collect(plain).partial_status, ref)
    assert e._lib.tbg_fetch_sets(e._h, plain, None, None) == eng.E_TICKET
    t = e.submit_sets(sf, **_args(b, sigs))
    assert e.poll(t) in (True, False)
    assert e._lib.tbg_collect(e._h, t, None, None, None, 1) == eng.E_TICKET
    res = e.collect_sets(t)
    assert e._lib.tbg_fetch(e._h, t, None, None, None) == eng.E_TICKET
    want = f_sets(ref, b.duty_first, sf)
    assert res.set_status.tolist() == want.tolist()
    # replay, then fetch: the same statuses
    e.replay(t, 2)
    again = e.fetch_sets(t, len(SMALL_SETS), 4 * n)
    assert np.array_equal(again.set_status, res.set_status)
    assert np.array_equal(again.partial_status, res.partial_status)
    # the other per-ticket calls work on a set ticket
    names = [k for k, _ in e.replay_profile(t)]
    assert "k_set_resolve" in names and "k_set_status" in names and "k_rlc_resolve_groups" not in names
    assert not any(k.startswith(("k_rlc_gident", "k_rlc_check_chunks", "k_rlc_cident", "k_rlc_ident")) for k in names)
    assert np.array_equal(e.fetch_sets(t, len(SMALL_SETS), 4 * n).set_status, res.set_status)
    assert e.shape(t)["group"] == 16 and e.stats(t)["group_size"] == 16
    assert e.level0(t) == eng.L0_NOT_RUN and e.subgroup(t)["groups"] == 0
    dev, pin = e.slot_bytes(t)
    assert dev > 0 and pin > 0
    assert e.fallback(t)["chunks"] == 0
