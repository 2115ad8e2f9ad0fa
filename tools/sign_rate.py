"""The hardened signer against the test-only one it stands beside.

  python tools/sign_rate.py [--n 16384] [--out profiles/keyed/sign_rate.json]

16,384 seeded keys through the C ABI, host work and copies included:

  sign_1     every key signs ONE message (a lock hash: one H(m), one table)
  sign_each  every key signs its own message (deposit data: a table per key)
  sk_to_pk   every key's public key

each by the old entry point (tbg_sign / tbg_sk_to_pk: plain double-and-add)
and by the new one (tbg_sign_ct / tbg_sk_to_pk_ct: 256 doublings, 64 complete
additions and 64 scans of a nine-entry table whatever the key is).  One
context; every shape is warmed once, then the two arms are timed alternately,
`reps` rounds, each timing repeated until it passes `seconds`.  The repeats of
the old arm give the run-to-run spread.  Every timed call's outputs are
checked after the clock stops: the two arms must agree byte for byte.  There is
no pass mark: the old path is the yardstick, the feature is safety."""
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


def main():
    from charon_amd import engine as eng
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.n
    rng = random.Random(0x516E)
    sk = b"".join(rng.randrange(1, R).to_bytes(32, "big") for _ in range(n))
    one = eng.pack_messages([b"\x5a" * 32])
    each = eng.pack_messages([rng.randbytes(32) for _ in range(n)])
    zeros, iota = np.zeros(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)
    e = eng.Engine(0, slots=2)

    def new_sign(msgs, im):
        out, st = e.sign_ct(sk, msgs, im)
        assert not st.any()
        return out

    def new_pk():
        out, st = e.sk_to_pk_ct(sk)
        assert not st.any()
        return out

    shapes = {
        "sign_1": (lambda: e.sign(sk, one, zeros), lambda: new_sign(one, zeros)),
        "sign_each": (lambda: e.sign(sk, each, iota), lambda: new_sign(each, iota)),
        "sk_to_pk": (lambda: e.sk_to_pk(sk), new_pk),
    }
    rows = []
    for name, arms in shapes.items():
        want = arms[0]()
        once = []
        for fn in arms:  # warm, check, and size the timed windows
            assert np.array_equal(fn(), want), name
            t0 = time.perf_counter()
            fn()
            once.append(time.perf_counter() - t0)
        rates = ([], [])
        for _ in range(args.reps):
            for a, fn in enumerate(arms):  # alternated
                k = max(1, int(np.ceil(args.seconds / once[a])))
                t0 = time.perf_counter()
                outs = [fn() for _ in range(k)]
                dt = time.perf_counter() - t0
                for o in outs:
                    assert np.array_equal(o, want), name
                rates[a].append(k * n / dt)
        med = [float(np.median(r)) for r in rates]
        row = {"shape": name, "items": n,
               "old_per_s": [round(x) for x in rates[0]], "new_per_s": [round(x) for x in rates[1]],
               "old_median": round(med[0]), "new_median": round(med[1]),
               "old_ms": round(1e3 * n / med[0], 3), "new_ms": round(1e3 * n / med[1], 3),
               "old_spread": round((max(rates[0]) - min(rates[0])) / med[0], 4),
               "new_over_old_time": round(med[0] / med[1], 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"what": "items per second through the C ABI (host range check, staging, copies and wiping included); "
                   "old: tbg_sign / tbg_sk_to_pk, new: tbg_sign_ct / tbg_sk_to_pk_ct", "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    e.close()


if __name__ == "__main__":
    main()
