"""The batched subgroup test's triple schedule on the GPU (k_sgb.hip: buckets
over three combinations' digits at once, groups larger than 1,024 partials,
the sort in global memory) against oracle/c, against a context that tests
every signature alone, and against the paired schedule's context.

The threshold and the group size are brought down to 2,048 partials
(tbg_config.sgb_tri_partials, sgb_tri_m), so 2,048 partials are one full
group and 2,052 a full group and a last group of four; one batch runs at the
compiled default group size.  Every run states which schedule its kernels took
(Engine.subgroup(..., schedule=True)), so a pass here is a pass of the triple
kernels; the last test checks that a context with the default configuration
keeps the paired schedule at this size.
"""
import dataclasses
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
M, TRI_M, DEFAULT_TRI_M = 1024, 2048, 16384  # SGB_M; the tests' sgb_tri_m; SGB_TRI_M
T, N = 3, 4


def run(e, b, sigs=None):
    from charon_amd import engine as eng
    t = e.submit(eng.OP_VERIFY_AGGREGATE, b.duty_first, b.sigs if sigs is None else sigs, b.identifiers,
                 msgs=(b.msg_data, b.msg_off), duty_msg=b.duty_msg, pubkey_ids=b.pubkey_ids,
                 duty_threshold=b.threshold)
    return e.collect(t), t


def new_engine(mode, **kw):
    from charon_amd import engine as eng
    return eng.Engine(0, slots=1, subgroup_batch=mode, rlc_batch=eng.RLC_L0_ON, **kw)


@pytest.fixture(scope="module")
def ctx():
    """Two batches, their oracle results, a context that tests every signature
    alone and one on the paired schedule.  Contexts on the triple schedule are
    made per test: the schedule follows the non-subgroup share of what a
    context has collected."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import oracle_run
    from tools.workload import make_batch
    off = new_engine(eng.SGB_OFF)
    b = make_batch(off, 512, T, N, seed=9300)
    tail = make_batch(off, 513, T, N, seed=9301)
    assert len(b.sigs) == TRI_M and len(tail.sigs) == TRI_M + 4
    paired = new_engine(eng.SGB_ON, sgb_tri_partials=eng.SGB_TRI_NEVER)
    load_keys(paired, dict(b=b, tail=tail))
    yield dict(off=off, paired=paired, b=b, tail=tail, ref=oracle_run(b), ref_tail=oracle_run(tail))
    paired.close()
    off.close()


def load_keys(e, ctx):
    """Both batches' keys in the order the `off` context loaded them."""
    for b in (ctx["b"], ctx["tail"]):
        first, st = e.load_pubkeys(b.pubshares)
        assert first == b.pk_first and (st == 0).all()


def tri_engine(ctx, partials=TRI_M, m=TRI_M):
    """A fresh context with the batched test forced on and the triple schedule
    from `partials` partials in groups of m, holding the keys."""
    from charon_amd import engine as eng
    e = new_engine(eng.SGB_ON, sgb_tri_partials=partials, sgb_tri_m=m)
    load_keys(e, ctx)
    return e


def crafted_points():
    with open(os.path.join(HERE, "golden", "sgb_points.json")) as f:
        return {k: [bytes.fromhex(h) for h in v] for k, v in json.load(f)["points"].items()}


@pytest.mark.parametrize("which", ["b", "tail"], ids=["2048", "2052_short_last_group"])
def test_clean_batch_passes_on_the_triple_schedule(ctx, which):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    b, ref = ctx[which], ctx["ref" if which == "b" else "ref_tail"]
    res_off, _ = run(ctx["off"], b)
    res_p, t_p = run(ctx["paired"], b)
    assert ctx["paired"].subgroup(t_p, schedule=True)["schedule"] == "paired"
    e = tri_engine(ctx)
    try:
        res, t = run(e, b)
        sg = e.subgroup(t, schedule=True)
        print("subgroup", sg, "level0", e.level0(t))
        assert sg == {"groups": -(-len(b.sigs) // TRI_M), "failed": 0, "group_size": TRI_M, "schedule": "triple"}, sg
        assert e.level0(t) == eng.L0_PASSED
        assert_same(res, ref)
        assert_same(res_off, ref)
        assert (res.partial_status == eng.PS_VALID).all() and np.array_equal(res.agg, b.group_sig)
        assert np.array_equal(res.agg, res_p.agg) and np.array_equal(res.partial_status, res_p.partial_status)
        assert np.array_equal(res.duty_status, res_p.duty_status)
    finally:
        e.close()


@pytest.mark.parametrize("pos,kind", [(TRI_M, "t13"), (TRI_M + 2, "t23"), (TRI_M + 3, "torsion13")],
                         ids=["first", "middle", "last"])
def test_one_crafted_point_in_group_1(ctx, pos, kind):
    """One non-subgroup signature in the short group 1 of the 2,052-partial
    batch: only group 1 fails, level 0 is voided, every verdict is exact."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    b = ctx["tail"]
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = np.frombuffer(crafted_points()[kind][0], dtype=np.uint8)
    ref = oracle_run(dataclasses.replace(b, sigs=sigs))
    res_off, t_off = run(ctx["off"], b, sigs=sigs)
    assert ctx["off"].subgroup(t_off, schedule=True)["schedule"] == "none"
    e = tri_engine(ctx)
    try:
        res, t = run(e, b, sigs=sigs)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 2, "failed": 1, "group_size": TRI_M, "schedule": "triple"}, sg  # group 1 alone failed
        assert e.level0(t) == eng.L0_FAILED
        assert_same(res, ref)
        assert_same(res_off, ref)
        assert np.flatnonzero(res.partial_status == eng.PS_ERR_SUBGROUP).tolist() == [pos]
        assert np.array_equal(res.partial_status, res_off.partial_status)
        assert np.array_equal(res.duty_status, res_off.duty_status) and np.array_equal(res.agg, res_off.agg)
    finally:
        e.close()


def test_one_crafted_point_in_the_full_group(ctx):
    """The same in the full group 0 of the 2,048-partial batch (its only group)."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    b = ctx["b"]
    pos = 1301
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = np.frombuffer(crafted_points()["t13"][1], dtype=np.uint8)
    ref = oracle_run(dataclasses.replace(b, sigs=sigs))
    e = tri_engine(ctx)
    try:
        res, t = run(e, b, sigs=sigs)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 1, "failed": 1, "group_size": TRI_M, "schedule": "triple"}, sg
        assert e.level0(t) == eng.L0_FAILED
        assert_same(res, ref)
        assert np.flatnonzero(res.partial_status == eng.PS_ERR_SUBGROUP).tolist() == [pos]
    finally:
        e.close()


def test_a_duty_replayed_48_times_and_a_decode_failure(ctx):
    """Duties 0..47 are one duty 48 times (three signatures 48 times each):
    equal bucket sums, redone with the complete formulas, fail nothing.  Then
    the same batch with one undecodable signature: left out of every sum, no
    group fails."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    b = ctx["b"]
    reps = 48
    sigs, ids, pk = np.array(b.sigs, copy=True), np.array(b.identifiers, copy=True), np.array(b.pubkey_ids, copy=True)
    duty_msg, group_sig = np.array(b.duty_msg, copy=True), np.array(b.group_sig, copy=True)
    thr = np.array(b.threshold, copy=True)
    for d in range(1, reps):
        sigs[N * d:N * d + N], ids[N * d:N * d + N], pk[N * d:N * d + N] = sigs[:N], ids[:N], pk[:N]
        duty_msg[d], group_sig[d], thr[d] = duty_msg[0], group_sig[0], thr[0]
    rb = dataclasses.replace(b, sigs=sigs, identifiers=ids, pubkey_ids=pk, duty_msg=duty_msg, group_sig=group_sig,
                             threshold=thr)
    e = tri_engine(ctx)
    try:
        res, t = run(e, rb)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 1, "failed": 0, "group_size": TRI_M, "schedule": "triple"}, sg
        assert e.level0(t) == eng.L0_PASSED
        assert_same(res, oracle_run(rb))
        assert (res.partial_status == eng.PS_VALID).all() and np.array_equal(res.agg, rb.group_sig)
        pos = 1500
        bad = np.array(sigs, copy=True)
        bad[pos, 0] &= 0x7F  # no compression flag: a decode error
        res, t = run(e, rb, sigs=bad)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 1, "failed": 0, "group_size": TRI_M, "schedule": "triple"}, sg
        assert_same(res, oracle_run(dataclasses.replace(rb, sigs=bad)))
        assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]
    finally:
        e.close()


def test_group_of_two_batches_and_prefix_replay(ctx):
    """Both batches as one device batch (4,100 partials: three groups, the
    callers straddle them), then the first replayed as a prefix: 2,048
    partials, still one triple group."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    parts, refs = [ctx["b"], ctx["tail"]], [ctx["ref"], ctx["ref_tail"]]
    args = [dict(duty_first=p.duty_first, sigs=p.sigs, identifiers=p.identifiers, msgs=(p.msg_data, p.msg_off),
                 duty_msg=p.duty_msg, pubkey_ids=p.pubkey_ids, duty_threshold=p.threshold) for p in parts]
    e = tri_engine(ctx)
    try:
        tickets = e.submit_group(eng.OP_VERIFY_AGGREGATE, args)
        for p, ref, t in zip(parts, refs, tickets):
            res = e.collect(t)
            assert_same(res, ref)
            assert np.array_equal(res.agg, p.group_sig)
        assert e.level0(tickets[0]) == eng.L0_PASSED
        sg = e.subgroup(tickets[0], schedule=True)
        assert sg == {"groups": 3, "failed": 0, "group_size": TRI_M, "schedule": "triple"}, sg
        e.replay_plan([tickets[0]], [1])
        e.synchronize()
        assert e.level0(tickets[0]) == eng.L0_PASSED
        sg = e.subgroup(tickets[0], schedule=True)
        assert sg == {"groups": 1, "failed": 0, "group_size": TRI_M, "schedule": "triple"}, sg
        assert_same(e.fetch(tickets[0], parts[0].n_dv, len(parts[0].sigs)), refs[0])
    finally:
        e.close()


def test_prefix_below_the_threshold_goes_back_to_the_paired_schedule(ctx):
    """With the threshold at 4,100 partials the group of two takes the triple
    schedule and its 2,048-partial prefix the paired one, in the same arena."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    parts, refs = [ctx["b"], ctx["tail"]], [ctx["ref"], ctx["ref_tail"]]
    args = [dict(duty_first=p.duty_first, sigs=p.sigs, identifiers=p.identifiers, msgs=(p.msg_data, p.msg_off),
                 duty_msg=p.duty_msg, pubkey_ids=p.pubkey_ids, duty_threshold=p.threshold) for p in parts]
    e = tri_engine(ctx, partials=2 * TRI_M + 4)
    try:
        tickets = e.submit_group(eng.OP_VERIFY_AGGREGATE, args)
        for p, ref, t in zip(parts, refs, tickets):
            assert_same(e.collect(t), ref)
        assert e.subgroup(tickets[0], schedule=True)["schedule"] == "triple"
        e.replay_plan([tickets[0]], [1])
        e.synchronize()
        sg = e.subgroup(tickets[0], schedule=True)
        assert sg == {"groups": 2, "failed": 0, "group_size": M, "schedule": "paired"}, sg
        assert e.level0(tickets[0]) == eng.L0_PASSED
        assert_same(e.fetch(tickets[0], parts[0].n_dv, len(parts[0].sigs)), refs[0])
        e.replay_plan([tickets[0]], [0])  # the whole device batch again: triple
        e.synchronize()
        assert e.subgroup(tickets[0], schedule=True)["schedule"] == "triple"
        assert_same(e.fetch(tickets[1], parts[1].n_dv, len(parts[1].sigs)), refs[1])
    finally:
        e.close()


@pytest.fixture(scope="module")
def big(ctx):
    """SGB_TRI_M + 4 partials: one group of the compiled default size and a
    last group of four.  Valid by construction (make_batch's aggregates are
    the known answers); the oracle runs on the crafted variant's duty only."""
    from tools.workload import make_batch
    b = make_batch(ctx["off"], DEFAULT_TRI_M // N + 1, T, N, seed=9302)
    assert len(b.sigs) == DEFAULT_TRI_M + 4
    return b


def test_default_group_size_clean_and_crafted_in_the_short_last_group(ctx, big):
    from charon_amd import engine as eng
    b = big
    e = new_engine(eng.SGB_ON, sgb_tri_partials=len(b.sigs))
    try:
        load_keys(e, ctx)
        first, st = e.load_pubkeys(b.pubshares)
        assert first == b.pk_first and (st == 0).all()
        res, t = run(e, b)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 2, "failed": 0, "group_size": DEFAULT_TRI_M, "schedule": "triple"}, sg
        assert e.level0(t) == eng.L0_PASSED
        assert (res.partial_status == eng.PS_VALID).all() and (res.duty_status == eng.DS_OK).all()
        assert np.array_equal(res.agg, b.group_sig)
        pos = DEFAULT_TRI_M + 1
        sigs = np.array(b.sigs, copy=True)
        sigs[pos] = np.frombuffer(crafted_points()["t23"][0], dtype=np.uint8)
        res_off, _ = run(ctx["off"], b, sigs=sigs)
        res, t = run(e, b, sigs=sigs)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 2, "failed": 1, "group_size": DEFAULT_TRI_M, "schedule": "triple"}, sg
        assert e.level0(t) == eng.L0_FAILED
        assert np.flatnonzero(res.partial_status == eng.PS_ERR_SUBGROUP).tolist() == [pos]
        assert np.array_equal(res.partial_status, res_off.partial_status)
        assert np.array_equal(res.duty_status, res_off.duty_status) and np.array_equal(res.agg, res_off.agg)
        assert np.array_equal(res.agg[:DEFAULT_TRI_M // N], b.group_sig[:DEFAULT_TRI_M // N])
    finally:
        e.close()


def test_default_configuration_keeps_the_paired_schedule(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    b = ctx["tail"]
    e = new_engine(eng.SGB_ON)
    try:
        load_keys(e, ctx)
        res, t = run(e, b)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 3, "failed": 0, "group_size": M, "schedule": "paired"}, sg
        assert e.level0(t) == eng.L0_PASSED
        assert_same(res, ctx["ref_tail"])
    finally:
        e.close()
