"""GPU tests of TBG_OP_AGGREGATE_VERIFY (k_aggver.hip): per duty, the
recombination of TBG_OP_AGGREGATE, then CoreVerify of the aggregate under the
duty's group key, in one launch.

Expected values: oracle/c -- CombineSignatures (op 2) over the partials, then
CoreVerify (op 1) of every aggregate that combined, under the duty's key and
message; a duty whose check fails carries TBG_DS_AGG_INVALID / _AGG_PUBKEY and
an all-zero agg96, as a failed combination does.  The two-launch route on the
GPU (OP_AGGREGATE, then OP_VERIFY of the aggregates) is a second witness, run
once per case.  Every case runs under the four schedules of
tests/test_gpu_sets.py and must agree exactly."""
import ctypes
import functools

import numpy as np
import pytest

from charon_amd import engine as eng

pytestmark = pytest.mark.gpu

SCHEDULES = {
    "l0_on": dict(rlc_batch=eng.RLC_L0_ON),
    "l0_off_g4": dict(rlc_batch=eng.RLC_L0_OFF, rlc_group=4),
    "l0_off_g16": dict(rlc_batch=eng.RLC_L0_OFF, rlc_group=16),
    "each": dict(verify_mode=eng.VERIFY_EACH),
}
ALL = list(SCHEDULES)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
UNKNOWN_ID = 0xFFFFFF00  # past every table
BAD_KEY = bytes([0x9F]) + bytes([0xFF]) * 47  # compressed flag set, x >= p: fails to decode

_ENGINES = {}
_KEYS = {}  # resident id -> 48 bytes (the same ids in every schedule's engine)


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
    _KEYS.clear()
    for cached in (_small, _large, _forms, _failures, _cancelling, _shapes):
        cached.cache_clear()


def _load_all(pk48):
    """The keys under the same ids in every schedule's engine."""
    pk48 = np.ascontiguousarray(np.asarray(pk48, dtype=np.uint8).reshape(-1, 48))
    first, st = None, None
    for name in ALL:
        f, s = _engine(name).load_pubkeys(pk48)
        assert first is None or (f == first and np.array_equal(s, st))
        first, st = f, s
    for i in range(len(pk48)):
        _KEYS[first + i] = pk48[i].tobytes()
    return first, st


class Case:
    """One op-4 batch: inputs, per-duty key ids, and the expected outputs."""

    def __init__(self, duties, msgs, duty_msg, key_ids):
        # duties: per duty a list of (identifier, 96-byte signature)
        self.duty_first = np.concatenate([[0], np.cumsum([len(d) for d in duties])]).astype(np.uint32)
        flat = [p for d in duties for p in d]
        self.sigs = (np.frombuffer(b"".join(bytes(s) for _, s in flat), dtype=np.uint8).reshape(-1, 96).copy()
                     if flat else np.zeros((0, 96), np.uint8))
        self.ids = np.array([i for i, _ in flat], dtype=np.uint8)
        self.msgs = [bytes(m) for m in msgs]
        self.duty_msg = np.asarray(duty_msg, dtype=np.uint32)
        self.key_ids = np.asarray(key_ids, dtype=np.uint32)
        self.nd, self.np = len(duties), len(flat)
        self.ref = _reference(self)
        self.two = _two_launch(_engine("l0_on"), self)
        for a, b in zip(self.ref, self.two):
            assert np.array_equal(a, b), "oracle/c and the two-launch route on the GPU disagree"

    def args(self):
        return dict(duty_first=self.duty_first, sigs=self.sigs, identifiers=self.ids, msgs=self.msgs,
                    duty_msg=self.duty_msg, pubkey_ids=self.key_ids)


def _fold(ds, agg, ok, vps):
    """TBG_OP_AGGREGATE's outputs and the verdicts of the aggregates that combined -> op 4's."""
    ds, agg = ds.copy(), agg.copy()
    assert set(vps.tolist()) <= {eng.PS_VALID, eng.PS_INVALID, eng.PS_ERR_PUBKEY}
    ds[ok[vps == eng.PS_INVALID]] = eng.DS_AGG_INVALID
    ds[ok[vps == eng.PS_ERR_PUBKEY]] = eng.DS_AGG_PUBKEY
    agg[ds != eng.DS_OK] = 0
    return ds, agg


def _reference(c):
    from oracle import c as oc
    oc.build()
    used = sorted({int(k) for k in c.key_ids if int(k) in _KEYS})
    table = oc.PubkeyTable(np.frombuffer(b"".join(_KEYS[k] for k in used) or bytes(48), dtype=np.uint8))
    rel = np.array([used.index(int(k)) if int(k) in _KEYS else 0xFFFFFFFF for k in c.key_ids], dtype=np.uint32)
    ps, ds, agg = oc.run(2, c.duty_first, c.sigs, c.ids, table, threads=8)
    ok = np.flatnonzero(ds == eng.DS_OK)
    vps = np.zeros(0, np.int32)
    if len(ok):
        data, off = eng.pack_messages(c.msgs)
        vps, _, _ = oc.run(1, np.arange(len(ok) + 1), agg[ok], np.zeros(len(ok), np.uint8), table, msgs=data,
                           msg_off=off, duty_msg=c.duty_msg[ok], pubkey_ids=rel[ok], threads=8)
    ds, agg = _fold(ds, agg, ok, vps)
    return ps, ds, agg


def _two_launch(e, c):
    a = e.run(eng.OP_AGGREGATE, c.duty_first, c.sigs, c.ids)
    ok = np.flatnonzero(a.duty_status == eng.DS_OK)
    vps = np.zeros(0, np.int32)
    if len(ok):
        vps = e.run(eng.OP_VERIFY, np.arange(len(ok) + 1), a.agg[ok], np.zeros(len(ok), np.uint8), msgs=c.msgs,
                    duty_msg=c.duty_msg[ok], pubkey_ids=c.key_ids[ok]).partial_status
    ds, agg = _fold(a.duty_status, a.agg, ok, vps)
    return a.partial_status, ds, agg


def _run(name, c):
    e = _engine(name)
    t = e.submit(eng.OP_AGGREGATE_VERIFY, **c.args())
    res = e.collect(t)
    ps, ds, agg = c.ref
    print(name, "duty codes:", dict(zip(*np.unique(res.duty_status, return_counts=True))))
    assert np.array_equal(res.partial_status, ps)
    assert res.duty_status.tolist() == ds.tolist()
    assert np.array_equal(res.agg, agg)
    return e, t, res


def _duties_of(b, sigs=None):
    sigs = b.sigs if sigs is None else sigs
    return [[(int(b.identifiers[j]), sigs[j].tobytes()) for j in range(int(b.duty_first[d]), int(b.duty_first[d + 1]))]
            for d in range(b.n_dv)]


def _group_keys(e, secrets):
    pk = e.sk_to_pk(b"".join(s.to_bytes(32, "big") for s in secrets))
    first, st = _load_all(pk)
    assert (st == 0).all()
    return first + np.arange(len(secrets), dtype=np.uint32)


def _batch(n_dv, seed):
    """make_batch's clean 3-of-4 duties (all four partials), group keys loaded after the pubshares."""
    from tools.workload import make_batch
    e = _engine("l0_on")
    b = make_batch(e, n_dv, 3, 4, seed=seed, load=_load_all)
    return b, _group_keys(e, b.secrets)


# ------------------------------------------------------------ 1, 2. clean batches
@functools.lru_cache(maxsize=None)
def _small():
    """120 duties, 480 partials: every signature tested alone; the view's level 0 is the
    bucket MSM over 120 points."""
    b, gk = _batch(120, 91)
    return b, gk, Case(_duties_of(b), b.msgs, b.duty_msg, gk)


@functools.lru_cache(maxsize=None)
def _large():
    """700 duties, 2,800 partials: the partials take the batched subgroup test, the view none."""
    _small()
    b, gk = _batch(700, 92)
    return b, gk, Case(_duties_of(b), b.msgs, b.duty_msg, gk)


@pytest.mark.parametrize("schedule", ALL)
def test_clean_small(schedule):
    b, _, c = _small()
    e, t, res = _run(schedule, c)
    assert (res.duty_status == eng.DS_OK).all() and np.array_equal(res.agg, b.group_sig)
    assert (res.partial_status == eng.PS_NOT_VERIFIED).all()
    assert e.subgroup(t)["groups"] == 0
    fb = e.fallback(t)
    if schedule == "l0_on":
        assert e.level0(t) == eng.L0_PASSED and fb["level0"] == eng.L0_PASSED
        assert e.shape(t)["level0"] == 1 and e.level0_msgs(t)["merged"] is False
        assert fb["partial_checks"] == 0 and fb["duty_searches"] == 0
    elif schedule == "each":
        assert e.level0(t) == eng.L0_NOT_RUN and fb["partial_checks"] == 120 and fb["group_size"] == 0
    else:
        g = SCHEDULES[schedule]["rlc_group"]
        assert e.level0(t) == eng.L0_NOT_RUN and e.stats(t) == dict(groups=-(-120 // g), duty_checks=0,
                                                                      partial_checks=0, group_size=g)
    ms = e.timings()
    assert all(ms[k] >= 0 for k in eng.TIMING_KEYS) and ms["total"] >= ms["verify"] > 0 and ms["aggregate"] > 0


@pytest.mark.parametrize("schedule", ALL)
def test_clean_batched_decode(schedule):
    b, _, c = _large()
    e, t, res = _run(schedule, c)
    assert (res.duty_status == eng.DS_OK).all() and np.array_equal(res.agg, b.group_sig)
    sg = e.subgroup(t, schedule=True)
    assert sg["groups"] >= 2 and sg["failed"] == 0 and sg["schedule"] != "none"
    if schedule == "l0_on":
        assert e.level0(t) == eng.L0_PASSED


# ------------------------------------------------------------ 3. every way to finish a recombination
def _shares_at(secret, coeffs, xs):
    out = []
    for x in xs:
        acc = 0
        for cf in reversed([secret] + list(coeffs)):
            acc = (acc * x + cf) % R
        out.append(acc)
    return out


FORMS = [  # (threshold, identifiers of the partials submitted)
    (3, (1, 2, 3)), (3, (1, 2, 3, 4)),                  # denominator 1
    (2, (1, 3)), (3, (1, 2, 4)), (3, (1, 3, 4)),        # denominator > 1: k_aggregate_finish
    (7, tuple(range(1, 11))),                           # 7-of-10, all ten partials
    (7, (1, 2, 4, 5, 7, 9, 10)),                        # 7-of-10, exactly seven
    (9, tuple(range(247, 256))),                        # identifiers near 255: the integer form overflows,
    (3, (253, 254, 255)),                               #   agg_status sends the duty to the reference path
]


@functools.lru_cache(maxsize=None)
def _forms():
    _large()
    e = _engine("l0_on")
    rng = np.random.default_rng(93)
    from tools.workload import _scalars
    reps = 3  # (more than one lane pair per form; 27 duties)
    forms = FORMS * reps
    secrets = _scalars(rng, len(forms))
    msgs = [rng.bytes(32) for _ in forms]
    sks, item_msg = [], []
    for d, (t, xs) in enumerate(forms):
        sks += _shares_at(secrets[d], _scalars(rng, t - 1), xs)
        item_msg += [d] * len(xs)
    sig = e.sign(b"".join(s.to_bytes(32, "big") for s in sks), msgs, np.array(item_msg, dtype=np.uint32))
    group_sig = e.sign(b"".join(s.to_bytes(32, "big") for s in secrets), msgs, np.arange(len(forms)))
    duties, j = [], 0
    for _, xs in forms:
        duties.append([(x, sig[j + k].tobytes()) for k, x in enumerate(xs)])
        j += len(xs)
    gk = _group_keys(e, secrets)
    return group_sig, Case(duties, msgs, np.arange(len(forms)), gk)


@pytest.mark.parametrize("schedule", ALL)
def test_every_finish_of_a_recombination(schedule):
    group_sig, c = _forms()
    e, t, res = _run(schedule, c)
    assert (res.duty_status == eng.DS_OK).all() and np.array_equal(res.agg, group_sig)
    names = [k for k, _ in e.replay_profile(t)]
    for k in ("k_aggregate<false>", "k_aggregate_finish<false>", "k_aggregate_exc<false>", "k_aggver_candidates",
              "k_aggver_status"):
        assert k in names
    assert names.index("k_aggregate_exc<false>") < names.index("k_aggver_candidates") < names.index("k_aggver_status")
    assert not any(k.startswith(("k_sgb", "k_l0f", "k_l0m")) for k in names)
    again = e.fetch(t, c.nd, c.np)
    assert again.duty_status.tolist() == res.duty_status.tolist() and np.array_equal(again.agg, res.agg)


# ------------------------------------------------------------ 4. failures beside clean duties
# duties whose aggregate must fail its check: 6 of 120 = 5 %.  Level-1 groups of 16: group 0 holds
# one (3), group 1 two (20, 27), group 4 two (70, 71), group 6 one (100), the others none; of 4:
# 70 and 71 share group 17, the other four sit alone.
WRONG_MSG_PARTIAL, OTHER_DV_PARTIAL, WRONG_DUTY_MSG, OTHER_KEY = (3, 70), (20,), (27, 71), (100,)
NO_KEY, UNKNOWN_KEY, UNDECODED_KEY = 40, 41, 42
DUP_ID, LONE, IDENTITY, UNDECODABLE = 50, 51, 52, 53


@functools.lru_cache(maxsize=None)
def _failures():
    b, gk, _ = _small()
    e = _engine("l0_on")
    first, st = _load_all(np.frombuffer(BAD_KEY, dtype=np.uint8))
    assert st[0] != 0
    sk32 = b"".join(s.to_bytes(32, "big") for s in b.shares)
    wrong = [m[:-1] + bytes([m[-1] ^ 0xFF]) for m in b.msgs]
    wrong_sigs = e.sign(sk32, wrong, np.repeat(b.duty_msg, 4).astype(np.uint32))
    sigs = b.sigs.copy()
    for d in WRONG_MSG_PARTIAL:
        sigs[4 * d + 1] = wrong_sigs[4 * d + 1]       # the same share over a wrong message
    for d in OTHER_DV_PARTIAL:
        sigs[4 * d + 2] = b.sigs[4 * (d + 1) + 2]     # share 3 of the next DV (over its own message)
    duties = _duties_of(b, sigs)
    duty_msg, key_ids = b.duty_msg.copy(), gk.copy()
    for d in WRONG_DUTY_MSG:
        duty_msg[d] = duty_msg[d + 30]
    for d in OTHER_KEY:
        key_ids[d] = gk[d - 1]
    key_ids[NO_KEY], key_ids[UNKNOWN_KEY], key_ids[UNDECODED_KEY] = eng.NO_PUBKEY, UNKNOWN_ID, first
    duties[DUP_ID][3] = (duties[DUP_ID][0][0], duties[DUP_ID][3][1])
    duties[LONE] = duties[LONE][:1]
    duties[IDENTITY][2] = (3, bytes([0xC0]) + bytes(95))
    bad = bytearray(duties[UNDECODABLE][0][1])
    bad[0] &= 0x7F
    duties[UNDECODABLE][0] = (1, bytes(bad))
    return b, Case(duties, b.msgs, duty_msg, key_ids)


@pytest.mark.parametrize("schedule", ALL)
def test_failures_beside_clean_duties(schedule):
    b, c = _failures()
    want = np.full(120, eng.DS_OK, dtype=np.int32)
    for d in WRONG_MSG_PARTIAL + OTHER_DV_PARTIAL + WRONG_DUTY_MSG + OTHER_KEY:
        want[d] = eng.DS_AGG_INVALID
    want[[NO_KEY, UNKNOWN_KEY, UNDECODED_KEY]] = eng.DS_AGG_PUBKEY
    want[DUP_ID], want[LONE] = eng.DS_AGG_DUPLICATE_ID, eng.DS_AGG_TOO_FEW
    want[IDENTITY], want[UNDECODABLE] = eng.DS_AGG_IDENTITY, eng.DS_DECODE
    assert c.ref[1].tolist() == want.tolist()  # (the oracle's codes are the ones the issue names)
    e, t, res = _run(schedule, c)
    assert res.duty_status.tolist() == want.tolist()
    ok = want == eng.DS_OK
    assert np.array_equal(res.agg[ok], b.group_sig[ok]) and not res.agg[~ok].any()
    # the duties that never combined never reach a check, nor do the ones without a usable key
    fb = e.fallback(t)
    candidates = 120 - 4 - 3
    if schedule == "each":
        assert fb["partial_checks"] == candidates and fb["groups"] == 0
    else:
        g = fb["group_size"]
        bad_groups = {d // g for d in WRONG_MSG_PARTIAL + OTHER_DV_PARTIAL + WRONG_DUTY_MSG + OTHER_KEY}
        assert fb["groups"] == -(-120 // g)
        assert fb["group_searches"] + fb["chunks"] + fb["duty_searches"] + fb["partial_checks"] > 0
        assert fb["partial_checks"] <= min(candidates, g * len(bad_groups))
        assert fb["duty_searches"] <= g * len(bad_groups)
        if schedule == "l0_on":
            assert fb["level0"] == eng.L0_FAILED


# ------------------------------------------------------------ 5. cancelling errors
@functools.lru_cache(maxsize=None)
def _cancelling(da, db):
    """Partial 0 of duty da is s + D, that of duty db is s - D (D a point of G2; the same
    identifier set {1, 2, 3, 4}): the aggregates are off by +-lambda_1 D, which cancels in an
    unweighted sum of the two."""
    from oracle import bls12_381 as bls
    b, gk, _ = _small()
    delta = bls.g2_mul(bls.G2_GEN, 0x7654321)
    sigs = b.sigs.copy()
    for d, pt in ((da, delta), (db, bls.g2_neg(delta))):
        s = bls.g2_add(bls.g2_decompress(bytes(sigs[4 * d])), pt)
        sigs[4 * d] = np.frombuffer(bls.g2_compress(s), dtype=np.uint8)
    return Case(_duties_of(b, sigs), b.msgs, b.duty_msg, gk)


@pytest.mark.parametrize("schedule", ALL)
@pytest.mark.parametrize("pair", [(33, 34), (15, 16)], ids=["one_group", "two_groups"])
def test_cancelling_errors_both_fail(pair, schedule):
    c = _cancelling(*pair)
    _, _, res = _run(schedule, c)
    assert np.flatnonzero(res.duty_status != eng.DS_OK).tolist() == list(pair)
    assert (res.duty_status[list(pair)] == eng.DS_AGG_INVALID).all() and not res.agg[list(pair)].any()


# ------------------------------------------------------------ 6. shapes of the call
@functools.lru_cache(maxsize=None)
def _shapes():
    b, gk, _ = _small()
    duties = _duties_of(b)
    # six duties, five of them empty: n_duties > n_partials
    sparse = Case([[], duties[0], [], [], [], []], b.msgs[:6], [1, 0, 2, 3, 4, 5], [gk[1], gk[0]] + list(gk[2:6]))
    one = Case([duties[7]], [b.msgs[7]], [0], [gk[7]])
    parts = []
    for lo, hi, spoil in ((0, 30, 4), (30, 31, None), (31, 120, 77)):
        d = [list(x) for x in duties[lo:hi]]
        keys = gk[lo:hi].copy()
        if spoil is not None:
            keys[spoil - lo] = gk[spoil + 1]
        parts.append(Case(d, b.msgs[lo:hi], np.arange(hi - lo), keys))
    return sparse, one, parts


@pytest.mark.parametrize("schedule", ALL)
def test_sparse_and_single_duty(schedule):
    sparse, one, _ = _shapes()
    assert sparse.nd > sparse.np
    _, _, res = _run(schedule, sparse)
    assert res.duty_status.tolist() == [eng.DS_AGG_TOO_FEW, eng.DS_OK] + [eng.DS_AGG_TOO_FEW] * 4
    _, _, res = _run(schedule, one)  # (the express slot)
    assert res.duty_status.tolist() == [eng.DS_OK]


@pytest.mark.parametrize("schedule", ALL)
def test_group_replay_and_prefix(schedule):
    _, _, parts = _shapes()
    e = _engine(schedule)
    tickets = e.submit_group(eng.OP_AGGREGATE_VERIFY, [c.args() for c in parts])
    got = {}
    for k in (2, 0, 1):  # out of order
        assert e.poll(tickets[k]) in (True, False)
        got[k] = e.collect(tickets[k])
    for k, c in enumerate(parts):
        ps, ds, agg = c.ref
        assert np.array_equal(got[k].partial_status, ps) and got[k].duty_status.tolist() == ds.tolist()
        assert np.array_equal(got[k].agg, agg)
    assert [int((c.ref[1] == eng.DS_AGG_INVALID).sum()) for c in parts] == [1, 0, 1]
    dev, pin = e.slot_bytes(tickets[0])
    assert dev > 0 and pin > 0
    # the whole device batch again, then a one-batch prefix (a batch of its own): the same outputs
    for prefix, duties_run in ((False, 120), (True, 30)):
        if prefix:
            e.replay_plan([tickets[0]], [1])
        else:
            e.replay(tickets[1], 2)
        for k, c in enumerate(parts):
            f = e.fetch(tickets[k], c.nd, c.np)
            assert f.duty_status.tolist() == c.ref[1].tolist() and np.array_equal(f.agg, c.ref[2])
            assert np.array_equal(f.partial_status, c.ref[0])
        g = e.shape(tickets[0])["group"]
        assert e.stats(tickets[0])["groups"] == (-(-duties_run // g) if g else 0)


def test_abi_refusals():
    _, gk, c = _small()
    e = _engine("l0_off_g16")
    with pytest.raises(ValueError, match="one id per duty"):
        e.run(eng.OP_AGGREGATE_VERIFY, **dict(c.args(), pubkey_ids=np.repeat(gk, 4)))
    batch, keep, _, _ = e._batch(eng.OP_AGGREGATE_VERIFY, **c.args())
    sf = np.array([0, 60, 120], dtype=np.uint32)
    tk = ctypes.c_uint64()
    rc = e._lib.tbg_submit_sets(e._h, ctypes.byref(batch), sf.ctypes.data_as(ctypes.c_void_p), 2, ctypes.byref(tk))
    assert rc == eng.E_INVALID_ARG
    # the arrays the op requires
    for field in ("pubkey_ids", "duty_msg", "msg_off"):
        batch, keep, _, _ = e._batch(eng.OP_AGGREGATE_VERIFY, **c.args())
        setattr(batch, field, None)
        assert e._lib.tbg_submit(e._h, ctypes.byref(batch), ctypes.byref(tk)) == eng.E_INVALID_ARG
    assert e._lib.tbg_last_timings(e._h, None) == eng.E_INVALID_ARG
    # the adaptive state counts failed aggregates over checked duties: level 0 goes off after a bad batch
    a = eng.Engine(0, slots=1, express_partials=eng.EXPRESS_OFF)
    try:
        first, st = a.load_pubkeys(np.frombuffer(b"".join(_KEYS[int(k)] for k in gk), dtype=np.uint8))
        args = dict(c.args(), pubkey_ids=first + np.arange(120, dtype=np.uint32))
        t = a.submit(eng.OP_AGGREGATE_VERIFY, **args)
        assert (a.collect(t).duty_status == eng.DS_OK).all() and a.shape(t)["level0"] == 1
        spoiled = dict(args, pubkey_ids=np.roll(args["pubkey_ids"], 1))
        assert (a.run(eng.OP_AGGREGATE_VERIFY, **spoiled).duty_status == eng.DS_AGG_INVALID).all()
        t = a.submit(eng.OP_AGGREGATE_VERIFY, **args)
        assert (a.collect(t).duty_status == eng.DS_OK).all()
        assert a.shape(t)["level0"] == 0 and a.shape(t)["group"] == 4
    finally:
        a.close()


def test_multi_context_cut_inside_the_batch():
    """Two contexts on one GPU: pubkey_ids is cut at the duty offset."""
    _, c = _failures()
    ps, ds, agg = c.ref
    keys = {int(k): _KEYS[int(k)] for k in c.key_ids if int(k) in _KEYS}
    for e in _ENGINES.values():  # (their streams: TBG_MAX_SLOT_STREAMS is per process on one device)
        e.close()
    _ENGINES.clear()
    m = eng.MultiEngine([0, 0], slots=1, rlc_batch=eng.RLC_L0_OFF, rlc_group=16)
    try:
        order = sorted(keys)
        first, _ = m.load_pubkeys(np.frombuffer(b"".join(keys[k] for k in order), dtype=np.uint8))
        ids = np.array([first + order.index(int(k)) if int(k) in keys else int(k) for k in c.key_ids], dtype=np.uint32)
        t = m.submit(eng.OP_AGGREGATE_VERIFY, **dict(c.args(), pubkey_ids=ids))
        lay = m.layout(t)
        assert 0 < lay[1] < 120
        res = m.collect(t)
        assert np.array_equal(res.partial_status, ps) and res.duty_status.tolist() == ds.tolist()
        assert np.array_equal(res.agg, agg)
    finally:
        m.close()
