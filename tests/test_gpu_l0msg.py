"""Level 0 by message on the GPU (tbls_launch.h l0_by_msg, k_l0msg.hip).

In a fused launch whose duties share messages, level 0 sums the duties' key
sums P_d per distinct message and pairs one point Q_m with each H(m):
k_l0m_chunks / k_l0m_msgs / k_l0m_miller / k_l0m_fold in place of
k_miller_hex<MILLER_L0> / k_l0_fold.  Settings as test_gpu_l0_straus.py:
subgroup_batch = SGB_ON, level 0 forced on, slots = 1; contexts with
l0_msg_share ALWAYS, NEVER and the default (2), and one without level 0.  The
base shape is 512 DVs x 3-of-4 = 2,048 partials, the smallest fused launch.
Every result is compared with oracle/c (test_gpu_fullsize.oracle_run) and with
the NEVER context, byte for byte.
"""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_DV, T, N = 512, 3, 4
MILLER_DUTY, FOLD_DUTY = "k_miller_hex<MILLER_L0>", "k_l0_fold"
NEW = ("k_l0m_miller", "k_l0m_chunks", "k_l0m_msgs")


def _layouts():
    big = np.zeros(N_DV, dtype=np.uint32)  # 500 duties on message 0, 12 singletons spread through them
    big[np.arange(12) * 40 + 7] = np.arange(1, 13)
    sizes = [1 + (k * 7) % 27 for k in range(36)]  # 36 uneven messages, the 37th takes the rest
    sizes.append(N_DV - sum(sizes))
    assert sizes[-1] > 0
    many = np.repeat(np.arange(37), sizes).astype(np.uint32)
    many = many[np.random.default_rng(37).permutation(N_DV)]  # (interleaved)
    m257 = np.concatenate([np.repeat(np.arange(255), 2), [255, 256]]).astype(np.uint32)
    return dict(one=np.zeros(N_DV, dtype=np.uint32), two=(np.arange(N_DV) % 2).astype(np.uint32), big=big, many=many,
                pairs=np.repeat(np.arange(256), 2).astype(np.uint32), m257=m257)


@pytest.fixture(scope="module")
def ctx():
    """The contexts, one batch per message layout with its keys resident under
    the same ids in every context, and the oracle's results (computed once)."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import oracle_run
    from tools.workload import make_shared_batch
    kw = dict(slots=1, subgroup_batch=eng.SGB_ON)
    es = dict(always=eng.Engine(0, rlc_batch=eng.RLC_L0_ON, l0_msg_share=eng.L0_MSG_ALWAYS, **kw),
              never=eng.Engine(0, rlc_batch=eng.RLC_L0_ON, l0_msg_share=eng.L0_MSG_NEVER, **kw),
              default=eng.Engine(0, rlc_batch=eng.RLC_L0_ON, **kw),
              off=eng.Engine(0, rlc_batch=eng.RLC_L0_OFF, **kw))
    e = es["always"]
    batches = {name: make_shared_batch(e, N_DV, T, N, dm, seed=9000 + k)
               for k, (name, dm) in enumerate(_layouts().items())}
    # one message in use, a second index that no duty names
    batches["unused"] = make_shared_batch(e, N_DV, T, N, np.zeros(N_DV, dtype=np.uint32), seed=9090, n_msgs=2)
    # parsigex items: one partial per duty (1-of-1), 2,048 and 512 of them over 16 messages
    batches["items"] = make_shared_batch(e, 2048, 1, 1, np.repeat(np.arange(16), [130] * 15 + [98]), seed=9091)
    batches["items_small"] = make_shared_batch(e, 512, 1, 1, np.repeat(np.arange(16), 32), seed=9092)
    for b in batches.values():
        assert len(b.sigs) in (2048, 512)
    for other in es.values():
        if other is not e:
            for b in batches.values():
                first, st = other.load_pubkeys(b.pubshares)
                assert first == b.pk_first and (st == 0).all()
    ref = {}

    def oracle(name, b=None):
        if name not in ref:
            ref[name] = oracle_run(batches[name] if b is None else b)
        return ref[name]
    yield dict(es=es, b=batches, oracle=oracle)
    for x in es.values():
        x.close()


def run(e, b, sigs=None, pubkey_ids=None):
    from charon_amd import engine as eng
    t = e.submit(eng.OP_VERIFY_AGGREGATE, b.duty_first, b.sigs if sigs is None else sigs, b.identifiers,
                 msgs=(b.msg_data, b.msg_off), duty_msg=b.duty_msg,
                 pubkey_ids=b.pubkey_ids if pubkey_ids is None else pubkey_ids, duty_threshold=b.threshold)
    return e.collect(t), t


def variant(b, **kw):
    v = copy.copy(b)
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def kernels(e, t):
    return {name for name, _ in e.replay_profile(t)}


def same_bytes(a, b):
    return (np.array_equal(a.partial_status, b.partial_status) and np.array_equal(a.duty_status, b.duty_status) and
            np.array_equal(a.agg, b.agg))


def expected_hexads(e, t, n_slots):
    s = e.shape(t)
    G, C = s["group"], s["chunk"]
    return -(-n_slots // G) * -(-G // C)


def assert_merged(e, t, n_msgs):
    lm = e.level0_msgs(t)
    assert lm["merged"] is True and lm["hexads"] == expected_hexads(e, t, n_msgs), (lm, e.shape(t))
    ks = kernels(e, t)
    assert all(k in ks for k in NEW) and MILLER_DUTY not in ks and FOLD_DUTY not in ks, sorted(ks)


def both(ctx, b, sigs=None, pubkey_ids=None, ref=None):
    """The ALWAYS context's result and ticket, after checking it against the
    oracle and the NEVER context byte for byte."""
    from tests.test_gpu_fullsize import assert_same, oracle_run
    res, t = run(ctx["es"]["always"], b, sigs, pubkey_ids)
    res_never, t_never = run(ctx["es"]["never"], b, sigs, pubkey_ids)
    assert ctx["es"]["never"].level0_msgs(t_never)["merged"] is False
    if ref is None:
        kw = {k: v for k, v in dict(sigs=sigs, pubkey_ids=pubkey_ids).items() if v is not None}
        ref = oracle_run(variant(b, **kw))
    assert_same(res, ref)
    assert same_bytes(res, res_never)
    assert ctx["es"]["always"].level0(t) == ctx["es"]["never"].level0(t_never)
    return res, t


@pytest.mark.parametrize("layout,n_msgs", [("one", 1), ("two", 2), ("big", 13), ("many", 37)])
def test_clean_layouts_pair_per_message(ctx, layout, n_msgs):
    """One message for all 512 duties (32 chunks of 16 duties: a fold pass), odd /
    even duties, 500 duties plus 12 singletons (13 slots: no multiple of G or C),
    37 uneven interleaved messages."""
    from charon_amd import engine as eng
    e, b = ctx["es"]["always"], ctx["b"][layout]
    assert int(b.duty_msg.max()) + 1 == n_msgs
    res, t = both(ctx, b, ref=ctx["oracle"](layout))
    assert e.level0(t) == eng.L0_PASSED
    assert (res.partial_status == eng.PS_VALID).all() and (res.duty_status == 0).all()
    assert np.array_equal(res.agg, b.group_sig)
    assert_merged(e, t, n_msgs)
    assert e.level0(t) == eng.L0_PASSED
    # the per-duty form launches a hexad per chunk of duties
    tn = run(ctx["es"]["never"], b)[1]
    ks = kernels(ctx["es"]["never"], tn)
    assert MILLER_DUTY in ks and FOLD_DUTY in ks and not any(k in ks for k in NEW)
    assert ctx["es"]["never"].level0_msgs(tn) == {"merged": False,
                                                   "hexads": expected_hexads(ctx["es"]["never"], tn, N_DV)}
    # and a context without level 0 gives the same bytes
    res_off, t_off = run(ctx["es"]["off"], b)
    assert ctx["es"]["off"].level0(t_off) == eng.L0_NOT_RUN and same_bytes(res, res_off)
    assert ctx["es"]["off"].level0_msgs(t_off) == {"merged": False, "hexads": 0}


def test_default_share_merges_pairs_and_not_257_messages(ctx):
    """TBG_L0_MSG_SHARE = 2: 256 messages over 512 duties merge, 257 do not;
    both give the NEVER context's bytes."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    e = ctx["es"]["default"]
    for layout, n_msgs, merged in (("pairs", 256, True), ("m257", 257, False)):
        b = ctx["b"][layout]
        res, t = run(e, b)
        assert e.level0(t) == eng.L0_PASSED
        assert e.level0_msgs(t)["merged"] is merged
        assert e.level0_msgs(t)["hexads"] == expected_hexads(e, t, n_msgs if merged else N_DV)
        assert ("k_l0m_miller" in kernels(e, t)) is merged
        assert_same(res, ctx["oracle"](layout))
        assert same_bytes(res, run(ctx["es"]["never"], b)[0])
    # ALWAYS merges whenever n_msgs <= n_duties
    res, t = run(ctx["es"]["always"], ctx["b"]["m257"])
    assert ctx["es"]["always"].level0_msgs(t)["merged"] is True
    assert same_bytes(res, run(ctx["es"]["never"], ctx["b"]["m257"])[0])


@pytest.mark.parametrize("pos", [0, 2047], ids=["first", "last"])
def test_one_wrong_share_partial_inside_a_shared_message(ctx, pos):
    from charon_amd import engine as eng
    b = ctx["b"]["two"]
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = b.sigs[pos + 1 if pos % N == 0 else pos - 1]  # another share of its DV signed it
    res, t = both(ctx, b, sigs=sigs)
    assert ctx["es"]["always"].level0(t) == eng.L0_FAILED
    assert ctx["es"]["always"].level0_msgs(t)["merged"] is True
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]
    assert res.partial_status[pos] == eng.PS_INVALID


def test_cancelling_errors_across_two_duties_of_one_message(ctx):
    """s + D in one duty and s' - D in another duty of the same message (D as
    test_gpu_parity.py's cancelling test builds it): the errors cancel in an
    unweighted sum, not under the random scalars -- both are invalid."""
    from charon_amd import engine as eng
    from oracle import bls12_381 as bls
    b = ctx["b"]["one"]
    delta = bls.g2_mul(bls.G2_GEN, 0x1234567)
    sigs = np.array(b.sigs, copy=True)
    bad = [N * 3, N * 400 + 2]
    for p, d in zip(bad, (delta, bls.g2_neg(delta))):
        s = bls.g2_add(bls.g2_decompress(bytes(b.sigs[p])), d)
        sigs[p] = np.frombuffer(bls.g2_compress(s), dtype=np.uint8)
    res, t = both(ctx, b, sigs=sigs)
    assert ctx["es"]["always"].level0(t) == eng.L0_FAILED
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == bad
    assert (res.partial_status[bad] == eng.PS_INVALID).all()


def test_duty_without_candidates_inside_a_shared_message(ctx):
    from charon_amd import engine as eng
    b = ctx["b"]["two"]
    d = 301
    sigs = np.array(b.sigs, copy=True)
    sigs[N * d:N * d + N, 0] &= 0x7F  # no compression flag: a decode error, no candidate
    res, t = both(ctx, b, sigs=sigs)
    assert (res.partial_status[N * d:N * d + N] < 0).all()
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == list(range(N * d, N * d + N))
    assert ctx["es"]["always"].level0(t) == eng.L0_PASSED  # the duty is RLC_NONE: skipped by its message's sum
    assert ctx["es"]["always"].level0_msgs(t)["merged"] is True


def test_message_whose_duties_all_lack_candidates_is_an_empty_slot(ctx):
    from charon_amd import engine as eng
    b = ctx["b"]["many"]
    duties = np.flatnonzero(b.duty_msg == 5)
    assert 1 <= len(duties) < 40
    sigs = np.array(b.sigs, copy=True)
    parts = np.concatenate([np.arange(N * d, N * d + N) for d in duties])
    sigs[parts, 0] &= 0x7F
    res, t = both(ctx, b, sigs=sigs)
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == sorted(parts.tolist())
    assert ctx["es"]["always"].level0(t) == eng.L0_PASSED


def test_unused_message_index(ctx):
    from charon_amd import engine as eng
    e, b = ctx["es"]["always"], ctx["b"]["unused"]
    assert len(b.msg_off) == 3 and int(b.duty_msg.max()) == 0
    res, t = both(ctx, b, ref=ctx["oracle"]("unused"))
    assert e.level0(t) == eng.L0_PASSED and np.array_equal(res.agg, b.group_sig)
    assert_merged(e, t, 2)
    # the default context merges it too (2 x 2 <= 512)
    rd, td = run(ctx["es"]["default"], b)
    assert ctx["es"]["default"].level0_msgs(td)["merged"] is True and same_bytes(res, rd)


def test_one_missing_pubshare_voids_level0(ctx):
    from charon_amd import engine as eng
    from tools.workload import NO_PUBKEY
    b = ctx["b"]["big"]
    pos = 1024 + 6
    ids = np.array(b.pubkey_ids, copy=True)
    ids[pos] = NO_PUBKEY
    res, t = both(ctx, b, pubkey_ids=ids)
    assert res.partial_status[pos] == eng.PS_ERR_PUBKEY
    assert ctx["es"]["always"].level0(t) == eng.L0_FAILED
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]


@pytest.mark.parametrize("shape", ["items_small", "items"])
def test_set_launch(ctx, shape):
    """Sets of one-partial duties, one message per set (a peer's parsigex set is
    N items over one root): 16 x 32 items -- 512 partials, below the fused
    level 0's 2,048, so the launch cannot merge and must say so -- and 15 x 130 +
    98 = 2,048 items, whose sets are padded to the group size.  Verdicts equal
    the NEVER context's, clean and with one bad item."""
    from charon_amd import engine as eng
    b = ctx["b"][shape]
    sizes = [32] * 16 if shape == "items_small" else [130] * 15 + [98]
    set_first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    fused = shape == "items"
    bad = np.array(b.sigs, copy=True)
    pos = int(set_first[9]) + 5
    bad[pos] = b.sigs[pos + 1]  # another key's signature over the same root
    for sigs, want in ((b.sigs, [eng.SS_VALID] * 16), (bad, [eng.SS_VALID] * 9 + [eng.SS_INVALID] + [eng.SS_VALID] * 6)):
        out = {}
        for name in ("always", "never", "default"):
            e = ctx["es"][name]
            t = e.submit_sets(set_first, b.duty_first, sigs, b.identifiers, msgs=(b.msg_data, b.msg_off),
                              duty_msg=b.duty_msg, pubkey_ids=b.pubkey_ids)
            out[name] = e.collect_sets(t)
            assert e.level0_msgs(t)["merged"] is (fused and name != "never"), (name, shape)
            if fused and name == "always":
                padded = e.stats(t)["groups"] * e.shape(t)["group"]  # the launch decides from its padded duties
                assert padded >= 2048 and e.level0_msgs(t)["hexads"] == expected_hexads(e, t, 16)
                assert "k_l0m_miller" in kernels(e, t)
                assert e.level0(t) == (eng.L0_PASSED if sigs is b.sigs else eng.L0_FAILED)
        assert out["always"].set_status.tolist() == want
        for name in ("never", "default"):
            assert np.array_equal(out[name].set_status, out["always"].set_status)
            assert np.array_equal(out[name].partial_status, out["always"].partial_status)


def test_replayed_prefix_decides_from_its_own_messages(ctx):
    """Two caller batches in one grouped submit; replaying the first alone
    (n_parts = 1) runs the prefix's own plan and gives that batch's results."""
    from charon_amd import engine as eng
    e = ctx["es"]["always"]
    b0, b1 = ctx["b"]["big"], ctx["b"]["many"]
    args = [dict(duty_first=b.duty_first, sigs=b.sigs, identifiers=b.identifiers, msgs=(b.msg_data, b.msg_off),
                 duty_msg=b.duty_msg, pubkey_ids=b.pubkey_ids, duty_threshold=b.threshold) for b in (b0, b1)]
    alone, _ = run(e, b0)
    t0, t1 = e.submit_group(eng.OP_VERIFY_AGGREGATE, args)
    got0, got1 = e.collect(t0), e.collect(t1)
    assert same_bytes(got0, alone) and np.array_equal(got1.agg, b1.group_sig)
    assert e.level0_msgs(t0) == {"merged": True, "hexads": expected_hexads(e, t0, 13 + 37)}
    e.replay_plan([t0], n_parts=[1])
    assert e.level0(t0) == eng.L0_PASSED
    assert e.level0_msgs(t0) == {"merged": True, "hexads": expected_hexads(e, t0, 13)}
    again = e.fetch(t0, b0.n_dv, len(b0.sigs))
    assert same_bytes(again, alone)
    e.replay_plan([t0], n_parts=[0])  # the whole device batch again
    assert e.level0(t0) == eng.L0_PASSED and e.level0_msgs(t0)["hexads"] == expected_hexads(e, t0, 13 + 37)
    assert np.array_equal(e.fetch(t1, b1.n_dv, len(b1.sigs)).agg, b1.group_sig)


def test_multi_context_shards_decide_per_shard(ctx):
    """tbg_multi with two contexts on one device, 2 x 512 DVs, each shard over
    one message."""
    from charon_amd import engine as eng
    from tools.workload import make_shared_batch
    m = eng.MultiEngine([0, 0], slots=1, subgroup_batch=eng.SGB_ON, rlc_batch=eng.RLC_L0_ON)
    try:
        dm = np.repeat(np.arange(2), N_DV).astype(np.uint32)
        b = make_shared_batch(ctx["es"]["always"], 2 * N_DV, T, N, dm, seed=9100, load=m.load_pubkeys)
        t = m.submit(eng.OP_VERIFY_AGGREGATE, b.duty_first, b.sigs, b.identifiers, msgs=(b.msg_data, b.msg_off),
                     duty_msg=b.duty_msg, pubkey_ids=b.pubkey_ids, duty_threshold=b.threshold)
        assert m.layout(t) == [0, N_DV, 2 * N_DV]
        res = m.collect(t)
        assert (res.partial_status == eng.PS_VALID).all() and (res.duty_status == 0).all()
        assert np.array_equal(res.agg, b.group_sig)
        for i in range(2):
            c = m.context(i)
            # (a context numbers its tickets from 1: the shard's launch is its first)
            assert c.level0(1) == eng.L0_PASSED
            assert c.level0_msgs(1)["merged"] is True
            assert "k_l0m_miller" in kernels(c, 1)
        # the per-duty form on the same input, keys under the single context's ids
        never = ctx["es"]["never"]
        first, st = never.load_pubkeys(b.pubshares)
        for name, other in ctx["es"].items():  # (keep the contexts' key tables aligned)
            if other is not never:
                assert other.load_pubkeys(b.pubshares)[0] == first
        ids = (b.pubkey_ids.astype(np.int64) + first - b.pk_first).astype(np.uint32)
        assert same_bytes(res, run(never, b, pubkey_ids=ids)[0])
    finally:
        m.close()


def test_python_mirror_sends_each_distinct_message_once():
    """tbls.verify_sets_batch on one 2,048-item set over one root: [True], and
    the engine sees ONE message -- level 0 pairs per message with the hexads of
    a single group of message slots (2,048 messages would not merge)."""
    from charon_amd import engine as eng
    from charon_amd import tbls
    from tools.workload import make_shared_batch
    e = eng.Engine(0, slots=1, subgroup_batch=eng.SGB_ON, rlc_batch=eng.RLC_L0_ON)
    try:
        b = make_shared_batch(e, 2048, 1, 1, np.zeros(2048, dtype=np.uint32), seed=9200)
        items = [(bytes(b.pubshares[i]), b.msgs[0], bytes(b.sigs[i])) for i in range(2048)]
        seen = []
        submit_sets = e.submit_sets

        def recording(set_first, duty_first, sigs, identifiers, **kw):
            t = submit_sets(set_first, duty_first, sigs, identifiers, **kw)
            seen.append((t, len(kw["msgs"]), np.asarray(kw["duty_msg"])))
            return t
        e.submit_sets = recording
        assert tbls.verify_sets_batch([items], e) == [True]
        (t, n_msgs, duty_msg), = seen
        assert n_msgs == 1 and not duty_msg.any() and len(duty_msg) == 2048
        assert e.level0(t) == eng.L0_PASSED
        assert e.level0_msgs(t) == {"merged": True, "hexads": expected_hexads(e, t, 1)}
        # one bad item fails the set, two roots are two messages
        items[77] = (items[77][0], items[77][1], items[78][2])
        assert tbls.verify_sets_batch([items], e) == [False]
        out = tbls.verify_batch([(items[0][0], b"\x01" * 32, items[0][2]), items[1], items[2]], e)
        assert out == [False, True, True]
    finally:
        e.close()
