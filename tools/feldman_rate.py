"""Pubshares from the Feldman commitments against pubshares from the shares.

  python tools/feldman_rate.py [--evals 100000] [--out profiles/feldman/feldman_rate.json]

For (t, n) = (3, 4), (7, 10) and (170, 255), about `evals` pubshares per shape
(V = evals // n seeded verifiers at identifiers 1..n), through the C ABI with
host work and copies included:

  eval      Engine.eval_commitments: the V*t commitments decoded, V*n Horner
            evaluations (tbg_eval_commitments)
  ladder    the parent's way to the same bytes: Engine.sk_to_pk of the
            host-computed shares f(i) (tbg_sk_to_pk, plain double-and-add)
  ladder_ct the same through the hardened signer (tbg_sk_to_pk_ct)

and dkg.create_cluster_tss end to end (host split included), with and without
from_commitments, plain and hardened, at `cluster_evals` pubshares per shape
(every call splits the same seeded secrets, so the pubshares are resident
after the warm-up call and key_from_bytes_batch is a cache hit in both arms).

One context; every arm is warmed once, then the arms are timed alternately,
`reps` rounds, each timing repeated until it passes `seconds`.  Every timed
call's outputs are checked after the clock stops: the arms must agree byte for
byte.  The model column is the group-operation count per pubshare of each arm
(bls_feldman.h: (t - 1) (bits(i) + weight(i) - 1) averaged over i = 1..n,
against 256 doublings + 64 additions).  There is no pass mark."""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SHAPES = [(3, 4), (7, 10), (170, 255)]


def horner_ops(t, n):
    """Mean group operations of one evaluation over identifiers 1..n."""
    return (t - 1) * sum(i.bit_length() + bin(i).count("1") - 1 for i in range(1, n + 1)) / n


def timed(arms, want, reps, seconds, items):
    """arms: {name: fn}.  Warm and check each, then alternate.  -> {name: [items per second]}"""
    once = {}
    for name, fn in arms.items():
        assert np.array_equal(fn(), want), name
        t0 = time.perf_counter()
        fn()
        once[name] = time.perf_counter() - t0
    rates = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            k = max(1, int(np.ceil(seconds / once[name])))
            t0 = time.perf_counter()
            outs = [fn() for _ in range(k)]
            dt = time.perf_counter() - t0
            for o in outs:
                assert np.array_equal(o, want), name
            rates[name].append(k * items / dt)
    return rates


def main():
    from charon_amd import dkg
    from charon_amd import engine as eng
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=100000)
    ap.add_argument("--cluster-evals", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    e = eng.Engine(0, slots=2)
    rows = []
    for t, n in SHAPES:
        V = max(1, args.evals // n)
        rng = random.Random(0xFE1D + t)
        polys = [[rng.randrange(1, R) for _ in range(t)] for _ in range(V)]
        commits = e.sk_to_pk(b"".join(a.to_bytes(32, "big") for p in polys for a in p))
        first = np.arange(V + 1, dtype=np.uint32) * t
        eval_poly = np.repeat(np.arange(V, dtype=np.uint32), n)
        eval_id = np.tile(np.arange(1, n + 1, dtype=np.uint32), V)
        shares = []
        for p in polys:
            for i in range(1, n + 1):
                acc = 0
                for a in reversed(p):
                    acc = (acc * i + a) % R
                shares.append(acc)
        sk = b"".join(v.to_bytes(32, "big") for v in shares)

        def ev():
            out, st, cst = e.eval_commitments(commits, first, eval_poly, eval_id)
            assert not st.any() and not cst.any()
            return out

        def ct():
            out, st = e.sk_to_pk_ct(sk)
            assert not st.any()
            return out

        want = e.sk_to_pk(sk)
        rates = timed({"ladder": lambda: e.sk_to_pk(sk), "eval": ev, "ladder_ct": ct}, want, args.reps, args.seconds, V * n)
        med = {k: float(np.median(v)) for k, v in rates.items()}
        row = {"shape": f"{t}-of-{n}", "verifiers": V, "pubshares": V * n,
               "model_ops": {"eval": round(horner_ops(t, n), 1), "ladder": 320},
               "per_s": {k: [round(x) for x in v] for k, v in rates.items()},
               "median_per_s": {k: round(v) for k, v in med.items()},
               "ladder_spread": round((max(rates["ladder"]) - min(rates["ladder"])) / med["ladder"], 4),
               "eval_over_ladder": round(med["eval"] / med["ladder"], 3),
               "eval_over_ladder_ct": round(med["eval"] / med["ladder_ct"], 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)

        Vc = max(1, args.cluster_evals // n)
        secrets = [rng.randrange(1, R) for _ in range(Vc)]

        def cluster(hardened, fc):
            dvs, _ = dkg.create_cluster_tss(secrets, t, n, random.Random(7), engine=e, hardened=hardened, from_commitments=fc)
            return np.frombuffer(b"".join(d.pubshares[i].raw for d in dvs for i in range(1, n + 1)), dtype=np.uint8)

        want_c = cluster(False, False)
        arms = {"shares": lambda: cluster(False, False), "commitments": lambda: cluster(False, True),
                "shares_ct": lambda: cluster(True, False), "commitments_ct": lambda: cluster(True, True)}
        rates = timed(arms, want_c, args.reps, 0.0, Vc * n)
        med = {k: float(np.median(v)) for k, v in rates.items()}
        row = {"shape": f"{t}-of-{n}", "create_cluster_tss": True, "validators": Vc, "pubshares": Vc * n,
               "per_s": {k: [round(x) for x in v] for k, v in rates.items()},
               "median_per_s": {k: round(v) for k, v in med.items()},
               "commitments_over_shares": round(med["commitments"] / med["shares"], 3),
               "commitments_ct_over_shares_ct": round(med["commitments_ct"] / med["shares_ct"], 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "pubshares per second through the C ABI (decode of the commitments, copies and host work included); "
                   "eval: tbg_eval_commitments, ladder: tbg_sk_to_pk, ladder_ct: tbg_sk_to_pk_ct of the host-computed "
                   "shares; create_cluster_tss rows: the whole call, host split included", "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    e.close()


if __name__ == "__main__":
    main()
