"""create_cluster_tss with the split on the device against the hardened path.

  python tools/split_rate.py [--validators 1000] [--t 3] [--n 4] [--out FILE.json]

Wall time of dkg.create_cluster_tss for `validators` seeded secrets, host work
and copies included, in two arms with the same rng seed:

  hardened      hardened=True: the split on host integers, ONE tbg_sk_to_pk_ct
                launch for every commitment and pubshare
  device_split  device_split=True: ONE tbg_split_secret_ct call (Horner on the
                device, then the same ladder over the device copies)

One context; each arm is warmed once, then the arms are timed alternately,
`reps` rounds.  After the clock stops the two arms' return values must be
equal.  Also timed: the engine calls alone (Engine.split_secret_ct over the
same polynomials, Engine.combine_shares_ct over one t-subset per validator).
There is no pass mark: the ladders dominate and are the same code in both."""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from charon_amd import dkg, tbls
    from charon_amd import engine as eng
    ap = argparse.ArgumentParser()
    ap.add_argument("--validators", type=int, default=1000)
    ap.add_argument("--t", type=int, default=3)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    v, t, n = args.validators, args.t, args.n
    rng = random.Random(0x5917)
    secrets = [rng.randrange(1, tbls.R) for _ in range(v)]
    e = eng.Engine(0, slots=2)

    def arm(**kw):
        t0 = time.perf_counter()
        out = dkg.create_cluster_tss(secrets, t, n, random.Random(0xD5), engine=e, **kw)
        return time.perf_counter() - t0, out

    arms = {"hardened": dict(hardened=True), "device_split": dict(device_split=True)}
    results = {k: arm(**kw)[1] for k, kw in arms.items()}  # warm-up
    a, b = results["hardened"], results["device_split"]
    assert a[1] == b[1] and all(x.pubshares == y.pubshares and x.commitments == y.commitments for x, y in zip(a[0], b[0]))
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, kw in arms.items():
            times[k].append(arm(**kw)[0])

    polys = [[s] + [rng.randrange(1, tbls.R) for _ in range(t - 1)] for s in secrets]
    coef = b"".join(c.to_bytes(32, "big") for p in polys for c in p)
    first = np.arange(0, t * v + 1, t, dtype=np.uint32)
    calls = {"split_secret_ct": [], "combine_shares_ct": []}
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        sh, cm, pub, st = e.split_secret_ct(coef, first, n)
        calls["split_secret_ct"].append(time.perf_counter() - t0)
        assert (st == eng.SH_OK).all()
        val = sh.reshape(v, n, 32)[:, :t].tobytes()
        t0 = time.perf_counter()
        sec, cst = e.combine_shares_ct(val, list(range(1, t + 1)) * v, first)
        calls["combine_shares_ct"].append(time.perf_counter() - t0)
        assert (cst == eng.SH_OK).all() and sec.tobytes() == b"".join(p[0].to_bytes(32, "big") for p in polys)
    e.close()

    med = lambda xs: float(np.median(xs))  # noqa: E731
    res = {"validators": v, "t": t, "n": n, "reps": args.reps,
           "create_cluster_tss_s": {k: {"median": med(x), "min": min(x), "max": max(x)} for k, x in times.items()},
           "engine_call_s": {k: {"median": med(x[1:]), "min": min(x[1:]), "max": max(x[1:])} for k, x in calls.items()}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
