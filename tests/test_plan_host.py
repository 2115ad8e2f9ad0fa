"""The launch plan and the arena section table (charon_amd/csrc/tbls_plan.h)
on the CPU, through the host twin tests/plan.

1. Layout unchanged: tests/golden/launch_layout.json holds, for a fixed list
   of launches, every number the hand-written sizing block of submit produced
   before it became the table (recorded from the parent commit by a host
   program that ran that block as it stood); the table reproduces each one.
2. Table invariants on those launches and a seeded random sweep.
3. bind over fake arena bases.
4. The replay fit rule derived from the table against its closed form
   (tests/plan_mirror.py shape_fits) and the cases the GPU tests pin.
5. l0_shape and sgb_plan against their Python mirrors.
6. The workspaces of the one-shot calls (tbls_work.h): tests/golden/
   oneshot_workspaces.json holds, for the smallest shapes that reach every
   section rule, the bytes each call allocated and the bytes each of its
   sections received while both were written by hand (recorded from the parent
   commit by a host program that ran those lines as they stood); the
   descriptions reproduce every section and never allocate more.
"""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from tests import plan_mirror
from tests.plan import lib

HERE = os.path.dirname(os.path.abspath(__file__))
ARENAS = {"in": 0, "work": 1, "out": 2}
OP_VERIFY, OP_AGGREGATE, OP_VERIFY_AGGREGATE, OP_AGGREGATE_VERIFY = 1, 2, 3, 4
# tbg_config's defaults, PlanConfig's order (group size and chunk not configured)
DEFAULT_CFG = [16, 4, 1, 1, 0, 0.0, 0.0, 0, 32768, 0, 600000, 131072, 2, 262144, 16384, 1024]
PLAN_FIELDS = ["n_duties", "rlc_group_cfg", "G", "C", "l0", "vp", "fb_w", "fb_full", "sgb", "sgb_m", "sgb_m_small",
               "sgb_split", "fused", "msm", "l0m_in", "l0m", "l0m_chunks", "gident", "aggver", "l0_msg_share"]
CANDIDATES = [(16, 4), (16, 8), (14, 7)] + [(c, c) for c in range(5, 11)]  # l0_shape's


def _args(row):
    cfg = np.array(row["cfg"], dtype=np.float64)
    b = np.array(row["batches"], dtype=np.uint32).reshape(-1, 3)
    sf = None if row["set_first"] is None else np.array(row["set_first"], dtype=np.uint32)
    return cfg, b, sf, [cfg.ctypes.data, row["op"], row["msg_bytes"], b.ctypes.data, len(b),
                        None if sf is None else sf.ctypes.data, 0 if sf is None else len(sf) - 1]


def layout(row):
    """The C++ plan and layout of a launch: (plan dict, totals dict, [(name, arena, offset, bytes)])."""
    keep = _args(row)
    n_max = lib().pl_max_sections()
    plan = np.zeros(20, dtype=np.uint64)
    tot = np.zeros(4, dtype=np.uint64)
    secs = np.zeros((n_max, 3), dtype=np.uint64)
    names = (ctypes.c_char_p * n_max)()
    n = lib().pl_layout(*keep[3], plan.ctypes.data, tot.ctypes.data, secs.ctypes.data, ctypes.addressof(names))
    assert 0 < n <= n_max
    sections = [(names[i].decode(), int(secs[i, 0]), int(secs[i, 1]), int(secs[i, 2])) for i in range(n)]
    return (dict(zip(PLAN_FIELDS, map(int, plan))),
            dict(zip(("in_bytes", "work_bytes", "w_out", "out_bytes"), map(int, tot))), sections)


def bind(row, in_base, work_base, out_base=0):
    keep = _args(row)
    n_max = lib().pl_max_sections()
    ptrs = np.zeros(n_max, dtype=np.uint64)
    alias = np.zeros(5, dtype=np.uint64)
    scalars = np.zeros(12, dtype=np.uint32)
    n = lib().pl_bind(*keep[3], in_base, work_base, out_base, ptrs.ctypes.data, alias.ctypes.data, scalars.ctypes.data)
    assert n > 0
    return [int(x) for x in ptrs[:n]], [int(x) for x in alias], [int(x) for x in scalars]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "launch_layout.json")) as f:
        return json.load(f)["rows"]


def random_rows(count, seed):
    """Launches over every op and knob, small counts with the occasional batch past SGB_MIN_PARTIALS."""
    rng = random.Random(seed)
    rows = []
    for _ in range(count):
        cfg = list(DEFAULT_CFG)
        if rng.random() < 0.5:  # a configured group size (and maybe chunk)
            cfg[0], cfg[3] = rng.choice([0, 1, 2, 4, 5, 8, 14, 16, 33, 100]), 0
            if rng.random() < 0.5:
                cfg[1], cfg[2] = rng.choice([1, 2, 4, 7, 8, 16, 50]), 0
        cfg[4] = rng.choice([0, 0, 1, 2])
        cfg[5] = rng.choice([0.0, 0.0, 1e-6, 1e-5, 0.004, 0.05, 0.5])
        cfg[6] = rng.choice([0.0, 0.0, 1e-5, 6.7e-4, 1.25e-3, 4e-3, 2e-2])
        cfg[7] = rng.choice([0, 1, 2])
        cfg[8] = rng.choice([1, 16, 100, 5000, 32768])
        cfg[9] = rng.choice([0, 0, 1, 2])
        cfg[12] = rng.choice([1, 2, 2, 3, 0xFFFFFFFF])
        cfg[13] = rng.choice([2048, 4096, 262144, 0xFFFFFFFF])
        cfg[14] = rng.choice([2048, 4096, 16384, 32768])
        cfg[15] = rng.choice([4, 8, 64, 1024, 1216])
        op = rng.choice([OP_VERIFY, OP_AGGREGATE, OP_VERIFY_AGGREGATE, OP_VERIFY_AGGREGATE, OP_AGGREGATE_VERIFY])
        sets = op == OP_VERIFY and rng.random() < 0.4
        batches = []
        for _ in range(1 if sets else rng.choice([1, 1, 2, 5])):
            nd = rng.choice([1, 2, 7, 16, 17, 100, 683, 1000, 3001])
            per = rng.choice([0, 1, 3, 4, 10])
            nm = 0 if op == OP_AGGREGATE else rng.choice([1, 2, nd // 2 + 1, nd])
            batches.append([nd, nd * per, nm])
        set_first = None
        if sets:
            nd, cuts = batches[0][0], [0]
            while cuts[-1] < nd:
                cuts.append(min(nd, cuts[-1] + rng.choice([0, 1, 2, 5, 23, 200])))
            set_first = cuts
        msg_bytes = 0 if op == OP_AGGREGATE else rng.choice([0, 1, 31, 32]) * sum(b[2] for b in batches)
        rows.append({"label": "random", "cfg": cfg, "op": op, "msg_bytes": msg_bytes, "batches": batches,
                     "set_first": set_first})
    return rows


def test_layout_equals_the_recorded_one(golden):
    assert 40 <= len(golden)
    for row in golden:
        plan, tot, secs = layout(row)
        for k, v in row["plan"].items():
            assert plan[k] == v, (row["label"], k, plan[k], v)
        for k in ("in_bytes", "work_bytes", "w_out", "out_bytes"):
            assert tot[k] == row[k], (row["label"], k, tot[k], row[k])
        want = [(name, ARENAS[arena], off) for name, arena, off in row["sections"]]
        assert [(name, arena, off) for name, arena, off, _ in secs] == want, row["label"]


def check_invariants(row):
    plan, tot, secs = layout(row)
    label = (row["label"], row["cfg"], row["op"], row["batches"], row["set_first"])
    assert len({name for name, *_ in secs}) == len(secs), label  # each section named once
    end = {0: 0, 1: 0}
    seen_out = False
    for name, arena, off, nbytes in secs:
        assert off % 16 == 0, (label, name)
        if arena == ARENAS["out"]:
            if not seen_out:  # the outputs begin at w_out, where the work sections end
                assert off == tot["w_out"] == end[1], (label, name)
            seen_out = True
        else:
            assert not (arena == ARENAS["work"] and seen_out), (label, name)  # the outputs are the tail
        a = 0 if arena == ARENAS["in"] else 1
        # ascending and disjoint: a section starts where the one before it ended, rounded up to 16 --
        # so an empty section holds no byte, and no byte of it is another section's
        assert off == end[a], (label, name)
        end[a] = (off + nbytes + 15) // 16 * 16
    assert seen_out
    assert end[0] == tot["in_bytes"] and end[1] == tot["work_bytes"], label
    assert tot["out_bytes"] == tot["work_bytes"] - tot["w_out"], label
    return plan, tot, secs


def check_bind(row):
    plan, tot, secs = layout(row)
    in_base, work_base = 0x100000000000, 0x200000000000
    ptrs, alias, scalars = bind(row, in_base, work_base)
    label = (row["label"], row["cfg"], row["op"], row["batches"], row["set_first"])
    ranges = []
    for (name, arena, off, nbytes), ptr in zip(secs, ptrs):
        base, size = (in_base, tot["in_bytes"]) if arena == ARENAS["in"] else (work_base, tot["work_bytes"])
        if ptr == 0:  # only the members of set / aggver launches, in other launches
            assert nbytes == 0 and name in ("duty_set", "av_iota", "agg_aff", "av_status", "av_counters", "set_status"), (label, name)
            continue
        assert ptr == base + off and base <= ptr and ptr + nbytes <= base + size, (label, name)
        if arena == ARENAS["out"]:
            assert ptr >= work_base + tot["w_out"], (label, name)
        if nbytes:
            ranges.append((ptr, ptr + nbytes, name))
    ranges.sort()
    for (a0, a1, an), (b0, b1, bn) in zip(ranges, ranges[1:]):
        assert a1 <= b0, (label, an, bn)
    by_name = {name: (arena, ptr) for (name, arena, _, _), ptr in zip(secs, ptrs)}
    for name in ("msgs", "msg_off", "duty_msg", "duty_first", "duty_threshold", "partial_duty", "sigs", "identifiers",
                 "pubkey_ids"):
        assert by_name[name][0] == ARENAS["in"] and in_base <= by_name[name][1] <= in_base + tot["in_bytes"], (label, name)
    for name in ("partial_status", "duty_status", "agg"):
        assert by_name[name][0] == ARENAS["out"] and by_name[name][1] >= work_base + tot["w_out"], (label, name)
    sets = row["set_first"] is not None
    assert (by_name["set_status"][1] != 0) == sets and (by_name["duty_set"][1] != 0) == sets, label
    for name in ("av_iota", "agg_aff", "av_status", "av_counters"):
        assert (by_name[name][1] != 0) == (row["op"] == OP_AGGREGATE_VERIFY), (label, name)
    # the host views: the input image alone (what the packers write), and the pinned output image apart
    # from any work arena (what collect reads) -- the other arenas' members stay null
    out_base = 0x300000000000
    for bases in ((in_base, 0, 0), (0, 0, out_base), (in_base, 0, out_base)):
        view, _, _ = bind(row, *bases)
        for (name, arena, off, nbytes), ptr, dev in zip(secs, view, ptrs):
            if arena == ARENAS["in"]:
                want = dev if bases[0] else 0
            elif arena == ARENAS["out"]:
                want = out_base + off - tot["w_out"] if bases[2] and dev else 0
                assert want == 0 or out_base <= want and want + nbytes <= out_base + tot["out_bytes"], (label, name)
            else:
                want = 0
            assert ptr == want, (label, name, bases)
    # the documented aliases: one fallback line buffer
    assert alias == [by_name["sig_lines"][1]] * 5, label
    aggver = row["op"] == OP_AGGREGATE_VERIFY
    assert scalars == [row["op"], plan["n_duties"], sum(b[1] for b in row["batches"]), sum(b[2] for b in row["batches"]),
                       0 if aggver else plan["G"], plan["C"], 0 if aggver else plan["l0"], plan["fb_w"], plan["sgb"],
                       plan["sgb_m"], int(sets), len(row["set_first"]) - 1 if sets else 0], label


def test_table_invariants_and_bind(golden):
    for row in golden + random_rows(400, seed=20):
        check_invariants(row)
        check_bind(row)


def test_fit_rule_equals_its_closed_form():
    fits = lambda *a: bool(lib().pl_shape_fits(*a))  # noqa: E731
    # the cases the GPU tests pin (test_gpu_replay_shape.py)
    assert not fits(160000, 16, 8, 90000, 16, 4)
    assert fits(40000, 16, 4, 17500, 14, 7) and not fits(40000, 16, 4, 17500, 5, 5)
    rng = random.Random(4)
    n_fit = 0
    for k in range(3000):
        nd0 = rng.choice([rng.randint(1, 200), rng.randint(1, 200000)])
        G0, C0 = rng.choice(CANDIDATES)
        G, C = rng.choice(CANDIDATES)
        # most draws near the boundary, where the seven inequalities disagree with one another
        nd = rng.choice([nd0, rng.randint(1, nd0), max(1, min(nd0, nd0 * G * C0 // (G0 * C) + rng.randint(-40, 40)))])
        want = plan_mirror.shape_fits(nd0, G0, C0, nd, G, C)
        assert fits(nd0, G0, C0, nd, G, C) == want, (nd0, G0, C0, nd, G, C)
        n_fit += want
    assert 300 < n_fit < 2700  # the sweep sees both answers


def _l0_shape(nd, n_simd, g_free=True, G=16, slot=None, prefixes=()):
    out = np.zeros(2, dtype=np.uint32)
    pre = np.array(prefixes, dtype=np.uint32)
    nd0, G0, C0 = slot or (0, 0, 0)
    lib().pl_l0_shape(nd, n_simd, int(g_free), G, nd0, G0, C0, pre.ctypes.data if len(pre) else None, len(pre),
                      out.ctypes.data)
    return int(out[0]), int(out[1])


def test_shape_rule_equals_its_mirror():
    # the literal cases of test_gpu_shape.py test_shape_mirror, on the C++
    assert _l0_shape(160000, 1024) == (16, 8)
    assert _l0_shape(125000, 1024) == (14, 7)
    assert _l0_shape(10000, 1024) == (16, 4)
    assert _l0_shape(100000, 1024) == (10, 10)
    assert _l0_shape(125000, 1024, g_free=False, G=16) == (16, 8)
    assert _l0_shape(200000, 1024, slot=(160000, 16, 8), prefixes=(70000, 70000, 60000)) == (10, 10)
    assert _l0_shape(480000, 1024) == (16, 8)
    rng = random.Random(5)
    duties = [1, 7, 100, 9999, 10000, 100000, 125000, 160000, 200000, 480000] + [rng.randint(1, 600000) for _ in range(150)]
    for n_cu in (304, 256):
        for nd in duties:
            assert _l0_shape(nd, n_cu * 4) == plan_mirror.expected_shape(nd, n_cu), (nd, n_cu)
            for G in (4, 8, 16, 100):
                assert _l0_shape(nd, n_cu * 4, g_free=False, G=G) == plan_mirror.expected_shape(nd, n_cu, g_free=False, G=G)
        # under a fits filter: prefixes of a slot sized at another shape
        for _ in range(150):
            nd0 = rng.randint(1000, 200000)
            G0, C0 = rng.choice(CANDIDATES)
            pre = [rng.randint(1, nd0) for _ in range(rng.randint(1, 3))]
            keep = lambda g, c: all(plan_mirror.shape_fits(nd0, G0, C0, n, g, c) for n in pre)  # noqa: E731
            want = plan_mirror.expected_shape(sum(pre), n_cu, fits=keep)
            # (nothing fits: the C++ leaves the caller's G, the mirror answers None)
            assert _l0_shape(sum(pre), n_cu * 4, slot=(nd0, G0, C0), prefixes=pre) == (want or (16, 4)), (nd0, G0, C0, pre)


def test_sgb_plan_equals_its_mirror():
    m = ctypes.c_uint32(0)
    for rho in (0, 1e-5, 6.7e-4, 1.25e-3, 2.5e-3, 2e-2, 4e-3, 1.0, 3.0):
        on = bool(lib().pl_sgb_plan(rho, ctypes.addressof(m)))
        assert (on, m.value) == plan_mirror.sgb_plan(rho), rho
    assert plan_mirror.sgb_plan(0) == (True, 1024) and plan_mirror.sgb_plan(1.25e-3) == (True, 128)
    assert not plan_mirror.sgb_plan(2e-2)[0]


WORK_CALLS = ["tbg_sk_to_pk", "tbg_sk_to_pk_ct", "tbg_sign", "tbg_sign_ct", "tbg_sum_pubkeys", "tbg_sum_sigs",
              "tbg_fast_aggregate_verify"]


def work(call, dims, base=0):
    """The C++ workspace of a one-shot call: (total bytes, [(name, offset, bytes, pointer)])."""
    signer = call in WORK_CALLS[:4]
    items = "n_keys" if call == "tbg_fast_aggregate_verify" else "n_items"
    keys = ("n", "n_msgs", "msg_bytes", "tab_words") if signer else ("n_sets", "n_chunks", items, "msg_bytes")
    d = np.array([dims.get(k, 0) for k in keys], dtype=np.uint64)
    n_max = lib().pl_max_work_sections()
    total = ctypes.c_uint64(0)
    secs = np.zeros((n_max, 2), dtype=np.uint64)
    ptrs = np.zeros(n_max, dtype=np.uint64)
    names = (ctypes.c_char_p * n_max)()
    n = lib().pl_work(WORK_CALLS.index(call), d.ctypes.data, base, ctypes.addressof(total), secs.ctypes.data,
                      ptrs.ctypes.data, ctypes.addressof(names))
    assert 0 < n <= n_max
    return total.value, [(names[i].decode(), int(secs[i, 0]), int(secs[i, 1]), int(ptrs[i])) for i in range(n)]


def test_oneshot_workspaces_equal_the_recorded_ones():
    with open(os.path.join(HERE, "golden", "oneshot_workspaces.json")) as f:
        rows = json.load(f)["rows"]
    assert {r["call"] for r in rows} == set(WORK_CALLS)
    # the shapes: signers n {1, 3} x messages {1, 2} x message bytes {0, 1, 33}; sums of 1 and 3 sets with an
    # empty set, no item at all and a set of two chunks
    for call in ("tbg_sign", "tbg_sign_ct"):
        got = {(r["dims"]["n"], r["dims"]["n_msgs"], r["dims"]["msg_bytes"]) for r in rows if r["call"] == call}
        assert got == {(n, m, b) for n in (1, 3) for m in (1, 2) for b in (0, 1, 33)}, call
    for call in ("tbg_sk_to_pk", "tbg_sk_to_pk_ct"):
        assert {r["dims"]["n"] for r in rows if r["call"] == call} == {1, 3}, call
    for call in WORK_CALLS[4:]:
        mine = [r["dims"] for r in rows if r["call"] == call]
        items = "n_keys" if call == "tbg_fast_aggregate_verify" else "n_items"
        assert {d["n_sets"] for d in mine} == {1, 3}, call
        assert any(d[items] == 0 for d in mine) and any(d["n_chunks"] > d["n_sets"] for d in mine), call
        assert any(0 < d["n_chunks"] < d["n_sets"] for d in mine), call  # an empty set among others
    base = 0x7F0000001000
    for r in rows:
        label = (r["call"], r["dims"])
        total, secs = work(r["call"], r["dims"])
        assert len({name for name, *_ in secs}) == len(secs), label  # each section named once
        end = 0
        for name, off, nbytes, ptr in secs:
            assert off % 16 == 0 and ptr == 0, (label, name)  # (the sizing walk hands out nothing)
            assert off >= end, (label, name)                  # disjoint, in walk order
            end = off + nbytes
        assert end <= total, label
        # the binding walk: the same sections at the same offsets, each pointer its section's address
        total_b, bound = work(r["call"], r["dims"], base)
        assert total_b == total and len(bound) == len(secs), label
        for (name, off, nbytes, _), (name_b, off_b, nbytes_b, ptr) in zip(secs, bound):
            assert (name_b, off_b, nbytes_b) == (name, off, nbytes) and ptr == base + off, (label, name)
        # against the parent: every section what its sec() call received, the allocation never larger
        assert [nbytes for _, _, nbytes, _ in secs] == r["sections"], label
        assert total <= r["need"], label
        if r["call"] != "tbg_fast_aggregate_verify":  # (whose sum reserved one 48-byte-per-set block it never carved)
            assert total == r["need"], label
