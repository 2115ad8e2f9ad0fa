"""A/B of the all-or-nothing set verification (tbg_submit_sets) against the
per-partial TBG_OP_VERIFY launch that parsig.Eth2Verifier.verify_sets makes.

Workload: `--sets` peer sets of `--dvs` 3-of-4 duties each (tools.workload.
make_batch), as ONE launch; run clean, then with one set carrying `--inject`
wrong-message partials.  Contexts are fresh and configured explicitly and
identically for the two arms: rlc_group = 16, level 0 ON for the clean input
and OFF for the bad one (what the adaptive policy settles on for each).
  arm A  TBG_OP_VERIFY over every partial (narrows a failed group to its bad partial)
  arm B  tbg_submit_sets (a failed group fails its set; no narrowing)
Per arm: the median and the max - min spread of `--iters` device-resident
replays (tbg_replay, HIP-event time of the kernel chain) after `--warmup`,
the arms' replays alternating.  Prints one JSON line (and writes --out).

Acceptance: on the bad input B's median is below A's by more
than A's spread; on the clean input B's median is within A's spread of A's."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def concat(batches):
    """Several make_batch batches back to back as one batch's arrays."""
    d0 = p0 = m0 = 0
    duty_first, duty_msg, msg_off = [np.zeros(1, np.uint32)], [], [np.zeros(1, np.uint32)]
    for b in batches:
        duty_first.append(b.duty_first[1:].astype(np.uint32) + p0)
        duty_msg.append(b.duty_msg.astype(np.uint32) + d0)
        msg_off.append(b.msg_off[1:].astype(np.uint32) + m0)
        d0 += b.n_dv
        p0 += len(b.identifiers)
        m0 += int(b.msg_off[-1])
    return dict(duty_first=np.concatenate(duty_first), sigs=np.concatenate([b.sigs for b in batches]),
                identifiers=np.concatenate([b.identifiers for b in batches]),
                msgs=(np.concatenate([b.msg_data for b in batches] + [np.zeros(1, np.uint8)]), np.concatenate(msg_off)),
                duty_msg=np.concatenate(duty_msg), pubkey_ids=np.concatenate([b.pubkey_ids for b in batches]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=16)
    ap.add_argument("--dvs", type=int, default=10000, help="duties per set")
    ap.add_argument("--inject", type=float, default=0.01, help="wrong-message share of the one bad set's partials")
    ap.add_argument("--bad-set", type=int, default=5)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=4242)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.iters < 7:
        sys.exit("bench_sets.py: at least 7 timed replays per arm")

    from charon_amd import engine as eng
    from tools.workload import make_batch

    gen = eng.Engine(0, slots=1)
    clean = [make_batch(gen, args.dvs, 3, 4, seed=args.seed + k) for k in range(args.sets)]
    bad_k = args.bad_set % args.sets
    assert clean[0].pk_first == 0
    # the bad set: the clean set's keys (same seed -> same shares) with injected wrong-message partials
    n_keys = gen.pubkey_count
    bad_b = make_batch(gen, args.dvs, 3, 4, seed=args.seed + bad_k, inject=args.inject)
    assert np.array_equal(bad_b.pubshares, clean[bad_k].pubshares)
    bad_b.pubkey_ids = clean[bad_k].pubkey_ids
    bad = list(clean)
    bad[bad_k] = bad_b
    pubshares = np.concatenate([b.pubshares for b in clean])
    assert len(pubshares) == n_keys
    gen.close()
    set_first = (np.arange(args.sets + 1) * args.dvs).astype(np.uint32)
    n_p = sum(len(b.identifiers) for b in clean)

    def measure(batches, rlc_batch):
        call = concat(batches)
        injected = np.concatenate([b.injected for b in batches])
        want_sets = [eng.SS_INVALID if b.injected.any() else eng.SS_VALID for b in batches]
        arms = {}
        for arm in ("A", "B"):
            e = eng.Engine(0, slots=1, rlc_group=16, rlc_batch=rlc_batch, express_partials=eng.EXPRESS_OFF)
            first, st = e.load_pubkeys(pubshares)
            assert first == 0 and (st == 0).all()
            if arm == "A":
                t = e.submit(eng.OP_VERIFY, **call)
                res = e.collect(t)
                assert np.array_equal(res.partial_status == eng.PS_VALID, ~injected), "arm A verdicts"
            else:
                t = e.submit_sets(set_first, **call)
                res = e.collect_sets(t)
                assert res.set_status.tolist() == want_sets, "arm B verdicts"
            arms[arm] = (e, t)
        ms = {"A": [], "B": []}
        for k in range(args.warmup + args.iters):
            for arm in ("A", "B"):
                e, t = arms[arm]
                total = e.replay(t, 1)["total"]
                if k >= args.warmup:
                    ms[arm].append(total)
        out = {}
        for arm in ("A", "B"):
            e, t = arms[arm]
            v = ms[arm]
            out[arm] = dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                            spread_ms=round(max(v) - min(v), 4), runs_ms=[round(x, 4) for x in v],
                            fallback=e.fallback(t))
            if arm == "B":  # the replays' outputs are still the collected ones
                assert e.fetch_sets(t, args.sets, n_p).set_status.tolist() == want_sets
            e.close()
        out["B_over_A"] = round(out["B"]["median_ms"] / out["A"]["median_ms"], 4)
        return out

    clean_r = measure(clean, eng.RLC_L0_ON)
    bad_r = measure(bad, eng.RLC_L0_OFF)
    a, b = bad_r["A"], bad_r["B"]
    ca, cb = clean_r["A"], clean_r["B"]
    result = {
        "bench": "sets", "sets": args.sets, "duties_per_set": args.dvs, "partials": n_p,
        "bad_set_inject": args.inject, "bad_partials": int(bad_b.injected.sum()), "iters": args.iters,
        "warmup": args.warmup, "config": {"rlc_group": 16, "rlc_batch": {"clean": "ON", "bad": "OFF"}},
        "clean": clean_r, "bad": bad_r,
        "B_bad_over_B_clean": round(b["median_ms"] / cb["median_ms"], 4),
        "accept_bad": bool(a["median_ms"] - b["median_ms"] > a["spread_ms"]),
        "accept_clean": bool(abs(cb["median_ms"] - ca["median_ms"]) <= ca["spread_ms"]),
    }
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
