"""The shrunk fallback passes on the GPU: passes of the level-2b and level-3
lists at or past DevBatch::fb_full run on grids of FB_SMALL = 640 list
positions whose hexads (k_rlc_ident_check, k_verify_list) and lane pairs
(k_lines_fold<FOLD_IDENT>, k_lines_sig_list) loop over the pass
(tbls_launch.h fb_passes / fb_pass_loop).  tests/test_fb_passes_host.py
proves the index arithmetic on the CPU; here the loops run on real lanes,
where the hexads of one wave make different numbers of trips and each trip
ends in lead-lane-only work before the next one's cross-lane products.

Windows: 1003 = 640 + 363 (in the last looping wave 3 hexads make two trips
and 7 make one) and 1507 = 2 * 640 + 227 (three trips, ragged in the same
way) -- the smallest windows with these shapes.  Level 0 is off, groups of 8
duties in chunks of one: a failed duty is alone in its chunk and goes to
level 2b, and with 30 % of the partials invalid a third of the duties carry
two or more and go on to level 3.

Each case mirrors the pass schedule (expected_passes of the host test, from
the plan twin's fb_w / fb_full and the list lengths the engine reports) and
asserts that the passes it is about did run, then compares every verdict
and aggregate with oracle/c and with the same batch on a context with the
default window, where every list is one full pass.
"""
import numpy as np
import pytest

from tests.test_fb_passes_host import FB_SMALL, expected_passes
from tests.test_gpu_fullsize import assert_same, engine_run, oracle_run
from tests.test_plan_host import DEFAULT_CFG, OP_VERIFY_AGGREGATE, layout

pytestmark = pytest.mark.gpu

CFG = dict(verify_mode=0, rlc_group=8, rlc_chunk=1, rlc_batch=2, rlc_seed=0x6b)


class Work:
    """The module's batches, made once on the default-window context `wide`
    (key ids in the order heavy, tail, light), with what every case compares
    against: oracle/c and wide's own results."""

    def __init__(self):
        from charon_amd import engine as eng
        from tools.workload import make_batch
        self.wide = eng.Engine(0, slots=1, **CFG)
        self.heavy = make_batch(self.wide, 3000, 3, 4, seed=1003, inject=0.3)
        self.tail = make_batch(self.wide, 2080, 3, 4, seed=1508, inject=0.3)
        self.light = make_batch(self.wide, 500, 3, 4, seed=21, inject=0.02)
        self._ref = {}

    def fresh(self, window):
        """A context with no history (invalid_ema = 0) and the same key ids."""
        from charon_amd import engine as eng
        e = eng.Engine(0, slots=1, fb_window=window, **CFG)
        for b in (self.heavy, self.tail, self.light):
            first, _ = e.load_pubkeys(b.pubshares)
            assert first == b.pk_first
        return e

    def ref(self, name):
        if name not in self._ref:
            b = getattr(self, name)
            self._ref[name] = (oracle_run(b), engine_run(self.wide, b))
        return self._ref[name]


@pytest.fixture(scope="module")
def work():
    w = Work()
    yield w
    w.wide.close()


def planned(window, invalid_ema, b):
    """(fb_w, fb_full) of a launch of batch b on a context of CFG with this window and history."""
    cfg = list(DEFAULT_CFG)
    cfg[0], cfg[1], cfg[2], cfg[3], cfg[4] = CFG["rlc_group"], CFG["rlc_chunk"], 0, 0, CFG["rlc_batch"]
    cfg[5], cfg[8] = invalid_ema, window
    plan, _, _ = layout(dict(cfg=cfg, op=OP_VERIFY_AGGREGATE, msg_bytes=32 * b.n_dv,
                             batches=[[b.n_dv, len(b.identifiers), b.n_dv]], set_first=None))
    return plan["fb_w"], plan["fb_full"]


def passes_of(fb_w, fb_full, max_entries, count):
    """The passes of a list of `count` entries that hold any: (base, held, shrunk)."""
    return [(base, min(count - base, fb_w), shrunk)
            for base, _, shrunk in expected_passes(fb_w, fb_full, max_entries, True) if base < count]


def run_and_compare(work, e, name):
    """Batch `name` on e: (the schedule's inputs, the result), after every parity assertion."""
    from charon_amd import engine as eng
    b = getattr(work, name)
    t = e.submit(eng.OP_VERIFY_AGGREGATE, b.duty_first, b.sigs, b.identifiers, msgs=(b.msg_data, b.msg_off),
                 duty_msg=b.duty_msg, pubkey_ids=b.pubkey_ids, duty_threshold=b.threshold)
    res = e.collect(t)
    fb = e.fallback(t)
    print(name, fb)
    ref, wide = work.ref(name)
    assert_same(res, ref)
    assert np.array_equal(res.partial_status == eng.PS_VALID, ~b.injected)
    assert np.array_equal(res.partial_status, wide.partial_status)
    assert np.array_equal(res.duty_status, wide.duty_status) and np.array_equal(res.agg, wide.agg)
    ok = res.duty_status == 0
    assert np.array_equal(ok, b.expect_ok) and np.array_equal(res.agg[ok], b.group_sig[ok])
    return fb, res


def test_level_2b_and_level_3_loop_twice(work):
    """W = 1003, fresh context: both lists have a shrunk pass filled to the
    window, whose hexads and pairs make two trips (ragged in the last wave)."""
    W = 1003
    b = work.heavy
    assert planned(W, 0.0, b) == (W, W)
    e = work.fresh(W)
    try:
        fb, _ = run_and_compare(work, e, "heavy")
    finally:
        e.close()
    for max_entries, count in ((b.n_dv, fb["duty_searches"]), (len(b.identifiers), fb["partial_checks"])):
        sched = passes_of(W, W, max_entries, count)
        assert any(shrunk and held == W for _, held, shrunk in sched), (count, sched)


def test_three_trips_and_the_list_ends_inside_a_shrunk_pass(work):
    """W = 1507: level 3's last pass is shrunk and holds more than 2 * 640
    entries but not the window -- three trips, and the list's end (k >= count),
    not the window's, stops the loops."""
    W = 1507
    b = work.tail
    assert planned(W, 0.0, b) == (W, W)
    e = work.fresh(W)
    try:
        fb, _ = run_and_compare(work, e, "tail")
    finally:
        e.close()
    sched = passes_of(W, W, len(b.identifiers), fb["partial_checks"])
    base, held, shrunk = sched[-1]
    assert shrunk and base > 0 and 2 * FB_SMALL < held < W, sched


def test_full_passes_up_to_a_measured_fb_full(work):
    """fb_full from a measured history: after a batch with 2 % invalid
    partials the context expects the heavy batch's lists to reach into their
    second window, so level 3's second pass is full and the later ones are
    shrunk."""
    from charon_amd import engine as eng
    W = 1003
    b, light = work.heavy, work.light
    e = work.fresh(W)
    try:
        r = engine_run(e, light)
        assert np.array_equal(r.partial_status == eng.PS_INVALID, light.injected)
        # the context's average after its first collected batch (tbg_collect: half the batch's invalid share)
        ema = 0.5 * int((r.partial_status == eng.PS_INVALID).sum()) / len(r.partial_status)
        # the planner's expected list length, well inside a window: no rounding decides fb_full
        windows = len(b.identifiers) * min(1.0, 10.0 * ema) / W
        assert abs(windows - round(windows)) > 0.1, windows
        fb_w, fb_full = planned(W, ema, b)
        assert fb_w == W and fb_full == 2 * W, (ema, fb_w, fb_full)
        fb, _ = run_and_compare(work, e, "heavy")
    finally:
        e.close()
    sched = passes_of(fb_w, fb_full, len(b.identifiers), fb["partial_checks"])
    full = [k for k, (base, held, shrunk) in enumerate(sched) if base > 0 and not shrunk and held == W]
    assert full and any(shrunk and held > FB_SMALL for _, held, shrunk in sched[full[-1] + 1:]), sched
