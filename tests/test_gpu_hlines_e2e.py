"""The H(m) lines from the projective steps (k_lines_h through px_h_lines)
under each of their readers, end to end against oracle/c
(test_gpu_fullsize.oracle_run), as test_gpu_sgb_pair.py runs its batches:
subgroup_batch = SGB_ON, level 0 forced on, slots = 1.

513 3-of-4 duties are 2,052 partials, the smallest fused launch
(k_miller_hex<MILLER_L0> reads the lines, one message per duty); the same
batch with one wrong-share partial sends the launch down the fallback levels
(chunk_f, the duty and partial levels, k_verify_list); 513 duties over 40
messages pair one key sum per message (k_l0m_miller reads the lines); 5 duties
run unfused.  A stored line differs from the pinned Jacobian form's by an Fp2
factor that every final exponentiation removes: statuses and aggregates are
exact in every case.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, N = 3, 4
N_DV = 513


def run(e, b, sigs=None):
    from charon_amd import engine as eng
    t = e.submit(eng.OP_VERIFY_AGGREGATE, b.duty_first, b.sigs if sigs is None else sigs, b.identifiers,
                 msgs=(b.msg_data, b.msg_off), duty_msg=b.duty_msg, pubkey_ids=b.pubkey_ids,
                 duty_threshold=b.threshold)
    return e.collect(t), t


def kernels(e, t):
    return {name for name, _ in e.replay_profile(t)}


@pytest.fixture(scope="module")
def ctx():
    from charon_amd import engine as eng
    from tools.workload import make_batch, make_shared_batch
    e = eng.Engine(0, slots=1, subgroup_batch=eng.SGB_ON, rlc_batch=eng.RLC_L0_ON)
    per_duty = make_batch(e, N_DV, T, N, seed=9300)
    sizes = [1 + (k * 5) % 23 for k in range(39)]  # 39 uneven messages, the 40th takes the rest
    sizes.append(N_DV - sum(sizes))
    assert sizes[-1] > 0
    dm = np.repeat(np.arange(40), sizes).astype(np.uint32)
    dm = dm[np.random.default_rng(40).permutation(N_DV)]
    shared = make_shared_batch(e, N_DV, T, N, dm, seed=9301)
    small = make_batch(e, 5, T, N, seed=9302)
    assert len(per_duty.sigs) == len(shared.sigs) == 2052 and len(small.sigs) == 20
    yield dict(e=e, per_duty=per_duty, shared=shared, small=small)
    e.close()


def assert_clean(e, b, res, t):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    assert_same(res, oracle_run(b))
    assert (res.partial_status == eng.PS_VALID).all() and (res.duty_status == 0).all()
    assert np.array_equal(res.agg, b.group_sig)


def test_fused_launch_one_message_per_duty(ctx):
    from charon_amd import engine as eng
    e, b = ctx["e"], ctx["per_duty"]
    assert len(set(b.duty_msg.tolist())) == N_DV
    res, t = run(e, b)
    assert e.level0(t) == eng.L0_PASSED
    fb = e.fallback(t)
    print("fallback", fb, "level0_msgs", e.level0_msgs(t))
    assert (fb["group_searches"], fb["chunks"], fb["chunk_searches"], fb["duty_searches"], fb["partial_checks"]) == \
        (0, 0, 0, 0, 0), fb
    assert e.level0_msgs(t)["merged"] is False
    ks = kernels(e, t)
    assert "k_lines_h" in ks and "k_miller_hex<MILLER_L0>" in ks, sorted(ks)
    assert_clean(e, b, res, t)


def test_one_wrong_share_partial_fails_level0_and_is_found(ctx):
    from charon_amd import engine as eng
    from tests.test_gpu_fullsize import assert_same, oracle_run
    import dataclasses
    e, b = ctx["e"], ctx["per_duty"]
    pos = N * 301 + 2
    sigs = np.array(b.sigs, copy=True)
    sigs[pos] = b.sigs[pos + 1]  # another share of its DV signed it
    res, t = run(e, b, sigs=sigs)
    assert e.level0(t) == eng.L0_FAILED
    fb = e.fallback(t)
    print("fallback", fb)
    assert fb["groups"] > 0 and fb["chunks"] > 0, fb  # the group levels ran and narrowed the failed group
    assert_same(res, oracle_run(dataclasses.replace(b, sigs=sigs)))
    assert np.flatnonzero(res.partial_status != eng.PS_VALID).tolist() == [pos]
    assert res.partial_status[pos] == eng.PS_INVALID
    keep = np.arange(N_DV) != 301
    assert np.array_equal(res.agg[keep], b.group_sig[keep])


def test_fused_launch_over_40_messages_pairs_per_message(ctx):
    from charon_amd import engine as eng
    e, b = ctx["e"], ctx["shared"]
    assert int(b.duty_msg.max()) + 1 == 40
    res, t = run(e, b)
    assert e.level0(t) == eng.L0_PASSED
    assert e.level0_msgs(t)["merged"] is True
    ks = kernels(e, t)
    assert "k_lines_h" in ks and "k_l0m_miller" in ks, sorted(ks)
    assert_clean(e, b, res, t)


def test_five_duties_unfused(ctx):
    e, b = ctx["e"], ctx["small"]
    res, t = run(e, b)
    print("level0", e.level0(t), "fallback", e.fallback(t))
    assert "k_lines_h" in kernels(e, t)
    assert_clean(e, b, res, t)
