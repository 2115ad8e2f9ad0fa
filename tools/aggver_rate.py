"""Aggregate-and-verify in one launch against the two launches it replaces.

  python tools/aggver_rate.py [--out profiles/aggver/rate.json]

Clean 3-of-4 duties (all four partials, one message and one group key per
duty) at 10k, 40k and 160k duties, through submit / collect with the host
packing included:

  (a) TBG_OP_AGGREGATE_VERIFY;
  (b) the route it replaces: TBG_OP_AGGREGATE, collect, TBG_OP_VERIFY of the
      aggregates under the group keys, collect;
  (c) TBG_OP_AGGREGATE alone.

One context; per size each route is warmed once, then the three are timed
alternately, `reps` rounds, each timing repeated until it passes `seconds`.
The repeats of (c) give the run-to-run spread.  Every timed call's outputs are
checked after the clock stops (duty codes, aggregates against engine.sign's
group signatures).  One profiled replay of (a) per size gives the per-kernel
split (tbg_replay_profile)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (10000, 40000, 160000)


def main():
    from charon_amd import engine as eng
    from tools.workload import make_batch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=lambda v: tuple(int(x) for x in v.split(",")), default=SIZES)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    e = eng.Engine(0, slots=2)
    rows, profiles = [], {}
    for n in args.sizes:
        b = make_batch(e, n, 3, 4, seed=88000 + n)
        gk_first, st = e.load_pubkeys(e.sk_to_pk(b"".join(s.to_bytes(32, "big") for s in b.secrets)))
        assert (st == 0).all()
        gk = gk_first + np.arange(n, dtype=np.uint32)
        msgs = (b.msg_data, b.msg_off)
        iota = np.arange(n + 1, dtype=np.uint32)
        zeros = np.zeros(n, dtype=np.uint8)

        def route_a():
            t = e.submit(eng.OP_AGGREGATE_VERIFY, b.duty_first, b.sigs, b.identifiers, msgs=msgs, duty_msg=b.duty_msg,
                         pubkey_ids=gk)
            return t, e.collect(t)

        def route_c():
            return e.run(eng.OP_AGGREGATE, b.duty_first, b.sigs, b.identifiers)

        def route_b():
            a = route_c()
            v = e.run(eng.OP_VERIFY, iota, a.agg, zeros, msgs=msgs, duty_msg=b.duty_msg, pubkey_ids=gk)
            return a, v

        def check_a(r):
            assert (r[1].duty_status == eng.DS_OK).all() and np.array_equal(r[1].agg, b.group_sig), n

        def check_b(r):
            assert (r[0].duty_status == eng.DS_OK).all() and np.array_equal(r[0].agg, b.group_sig), n
            assert (r[1].partial_status == eng.PS_VALID).all(), n

        def check_c(r):
            assert (r.duty_status == eng.DS_OK).all() and np.array_equal(r.agg, b.group_sig), n

        routes = {"a": (route_a, check_a), "b": (route_b, check_b), "c": (route_c, check_c)}
        once = {}
        for name, (fn, chk) in routes.items():  # warm every shape, and size the timed windows
            chk(fn())
            t0 = time.perf_counter()
            chk(fn())
            once[name] = time.perf_counter() - t0
        rates = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, (fn, chk) in routes.items():  # alternated
                k = max(1, int(np.ceil(args.seconds / once[name])))
                t0 = time.perf_counter()
                outs = [fn() for _ in range(k)]
                dt = time.perf_counter() - t0
                for r in outs:
                    chk(r)
                rates[name].append(k * n / dt)
        t, _ = route_a()
        shape, l0, sg = e.shape(t), e.level0(t), e.subgroup(t, schedule=True)
        acc = {}
        for kname, ms in e.replay_profile(t):
            acc[kname] = acc.get(kname, 0.0) + ms
        profiles[str(n)] = {kn: round(ms, 4) for kn, ms in sorted(acc.items(), key=lambda x: -x[1])[:16]}
        profiles[str(n)]["(all kernels)"] = round(sum(acc.values()), 4)
        f = e.fetch(t, n, 4 * n)
        assert (f.duty_status == eng.DS_OK).all() and np.array_equal(f.agg, b.group_sig)
        med = {name: float(np.median(r)) for name, r in rates.items()}
        row = {"duties": n, "shape": shape, "level0": l0, "subgroup": sg,
               **{f"{name}_duties_per_s": [round(x) for x in rates[name]] for name in routes},
               **{f"{name}_median": round(med[name]) for name in routes},
               "c_spread": round((max(rates["c"]) - min(rates["c"])) / med["c"], 4),
               "a_over_b": round(med["a"] / med["b"], 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"shape": "clean 3-of-4 duties, four partials each, one message and one group key per duty; "
                    "submit / collect, host packing included; duties per second",
           "rows": rows, "profiles_ms": profiles, "a_faster_than_b": {str(r["duties"]): r["a_over_b"] > 1 for r in rows}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps({"profiles_ms": profiles, "a_faster_than_b": out["a_faster_than_b"]}), flush=True)
    e.close()


if __name__ == "__main__":
    main()
