"""The batched subgroup test's paired schedule on the GPU (k_sgb.hip: buckets
over two combinations' digits at once, groups of 256 partials and more)
against oracle/c and against a context that tests every signature alone.

The smallest batch that takes the batched test: 2 x 1,024 partials (512
3-of-4 duties), and 2,052 (a short last group of four).  Every run states
which schedule its kernels took (Engine.subgroup(..., schedule=True)), so a
pass here is a pass of the paired kernels; the last test drives a context's
group size below the threshold and checks that the classic schedule still
runs there, exact.
"""
import dataclasses
import json
import os

import numpy as np
import pytest

from tests.plan_mirror import sgb_plan

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
M, PAIR_M = 1024, 256  # SGB_M, SGB_PAIR_M
T, N = 3, 4


def run(e, b, sigs=None):
    from charon_amd import engine as eng
    t = e.submit(eng.OP_VERIFY_AGGREGATE, b.duty_first, b.sigs if sigs is None else sigs, b.identifiers,
                 msgs=(b.msg_data, b.msg_off), duty_msg=b.duty_msg, pubkey_ids=b.pubkey_ids,
                 duty_threshold=b.threshold)
    return e.collect(t), t


def new_engine(mode):
    from charon_amd import engine as eng
    return eng.Engine(0, slots=1, subgroup_batch=mode, rlc_batch=eng.RLC_L0_ON)


@pytest.fixture(scope="module")
def ctx():
    """Two batches, their oracle results, and a context that tests every
    signature alone.  Contexts with the batched test are made per test: their
    group size follows the non-subgroup share of what they have collected."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import oracle_run
    from tools.workload import make_batch
    off = new_engine(eng.SGB_OFF)
    b = make_batch(off, 512, T, N, seed=9100)
    tail = make_batch(off, 513, T, N, seed=9101)
    assert len(b.sigs) == 2 * M and len(tail.sigs) == 2 * M + 4
    yield dict(off=off, b=b, tail=tail, ref=oracle_run(b), ref_tail=oracle_run(tail))
    off.close()


def load_keys(e, ctx):
    """Both batches' keys in the order the `off` context loaded them."""
    for b in (ctx["b"], ctx["tail"]):
        first, st = e.load_pubkeys(b.pubshares)
        assert first == b.pk_first and (st == 0).all()


def on_engine(ctx):
    """A fresh context with the batched test forced on, holding the keys."""
    from charon_amd import engine as eng
    e = new_engine(eng.SGB_ON)
    load_keys(e, ctx)
    return e


def crafted_points():
    with open(os.path.join(HERE, "golden", "sgb_points.json")) as f:
        return {k: [bytes.fromhex(h) for h in v] for k, v in json.load(f)["points"].items()}


@pytest.mark.parametrize("which", ["b", "tail"], ids=["2048", "2052_short_last_group"])
def test_clean_batch_passes_on_the_paired_schedule(ctx, which):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    b, ref = ctx[which], ctx["ref" if which == "b" else "ref_tail"]
    e = on_engine(ctx)
    try:
        res, t = run(e, b)
        sg = e.subgroup(t, schedule=True)
        print("subgroup", sg, "level0", e.level0(t))
        assert sg == {"groups": -(-len(b.sigs) // M), "failed": 0, "group_size": M, "schedule": "paired"}, sg
        assert e.level0(t) == eng.L0_PASSED
        assert_same(res, ref)
        assert (res.partial_status == eng.PS_VALID).all() and np.array_equal(res.agg, b.group_sig)
        assert e.subgroup(t) == {"groups": -(-len(b.sigs) // M), "failed": 0, "group_size": M}
    finally:
        e.close()


@pytest.mark.parametrize("pos,kind", [(M, "t13"), (M + 517, "t23"), (2 * M - 1, "torsion13")],
                         ids=["first", "middle", "last"])
def test_one_crafted_point_in_a_group(ctx, pos, kind):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    b = ctx["b"]
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = np.frombuffer(crafted_points()[kind][0], dtype=np.uint8)
    ref = oracle_run(dataclasses.replace(b, sigs=sigs))
    res_off, t_off = run(ctx["off"], b, sigs=sigs)
    assert ctx["off"].subgroup(t_off, schedule=True)["schedule"] == "none"
    e = on_engine(ctx)
    try:
        res, t = run(e, b, sigs=sigs)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 2, "failed": 1, "group_size": M, "schedule": "paired"}, sg  # group 1 alone failed
        assert e.level0(t) == eng.L0_FAILED
        assert_same(res, ref)
        assert_same(res_off, ref)
        assert np.flatnonzero(res.partial_status == eng.PS_ERR_SUBGROUP).tolist() == [pos]
        assert np.array_equal(res.partial_status, res_off.partial_status)
        assert np.array_equal(res.duty_status, res_off.duty_status) and np.array_equal(res.agg, res_off.agg)
    finally:
        e.close()


def test_a_duty_replayed_48_times_passes(ctx):
    """Duties 0..47 of group 0 are one duty 48 times (144 partials, three
    signatures 48 times each): equal bucket sums, redone with the complete
    formulas, fail nothing."""
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
    e = on_engine(ctx)
    try:
        res, t = run(e, rb)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 2, "failed": 0, "group_size": M, "schedule": "paired"}, sg
        assert e.level0(t) == eng.L0_PASSED
        assert_same(res, oracle_run(rb))
        assert (res.partial_status == eng.PS_VALID).all() and np.array_equal(res.agg, rb.group_sig)
    finally:
        e.close()


def test_a_negated_signature_gives_the_same_verdicts_as_alone(ctx):
    """s replaced by -s (the compressed form's sign bit) in one partial: a
    point of G2, so no group fails; the partial is invalid either way."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    b = ctx["b"]
    pos = M + 300
    sigs = np.array(b.sigs, copy=True)
    sigs[pos, 0] ^= 0x20
    ref = oracle_run(dataclasses.replace(b, sigs=sigs))
    res_off, _ = run(ctx["off"], b, sigs=sigs)
    e = on_engine(ctx)
    try:
        res, t = run(e, b, sigs=sigs)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 2, "failed": 0, "group_size": M, "schedule": "paired"}, sg
        assert_same(res, ref)
        assert_same(res_off, ref)
        assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]
        assert res.partial_status[pos] == eng.PS_INVALID
        assert np.array_equal(res.partial_status, res_off.partial_status)
        assert np.array_equal(res.duty_status, res_off.duty_status) and np.array_equal(res.agg, res_off.agg)
    finally:
        e.close()


def test_groups_below_the_threshold_keep_the_classic_schedule(ctx):
    """Five non-subgroup signatures in 2,048 partials bring an adaptive
    context's group size to 128: below SGB_PAIR_M, so its next batch runs the
    classic schedule -- and stays exact."""
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same
    b = ctx["b"]
    pts = crafted_points()
    bad = [3, 700, 1024, 1500, 2047]
    sigs = np.array(b.sigs, copy=True)
    for k, i in enumerate(bad):
        sigs[i] = np.frombuffer(pts["t13"][k % len(pts["t13"])], dtype=np.uint8)
    e = new_engine(eng.SGB_AUTO)
    try:
        load_keys(e, ctx)
        res, t = run(e, b, sigs=sigs)  # clean history: groups of 1,024, paired
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": 2, "failed": 2, "group_size": M, "schedule": "paired"}, sg
        assert np.flatnonzero(res.partial_status == eng.PS_ERR_SUBGROUP).tolist() == bad
        on, m = sgb_plan(0.5 * len(bad) / len(sigs))
        assert on and m < PAIR_M, m
        res, t = run(e, b)
        sg = e.subgroup(t, schedule=True)
        assert sg == {"groups": len(b.sigs) // m, "failed": 0, "group_size": m, "schedule": "classic"}, sg
        assert e.level0(t) == eng.L0_PASSED
        assert_same(res, ctx["ref"])
        assert (res.partial_status == eng.PS_VALID).all() and np.array_equal(res.agg, b.group_sig)
    finally:
        e.close()
