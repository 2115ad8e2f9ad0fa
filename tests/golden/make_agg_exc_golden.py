#!/usr/bin/env python3
"""Writes tests/golden/agg_exceptional.json: tbls.Aggregate duties whose
integer-form combination (k_aggregate.hip combine_int_pair: double-and-add
over the bits of |N_j|, additions without a doubling branch) meets the group
law's exceptional cases -- an addition of two equal points (the duty then
goes to the reference path), a cancellation that returns the accumulator to
infinity mid-loop, and a sum that is the identity -- with D = 1 and D > 1.

The partial signatures are small multiples [c] S of one honest signature S
(TBG_OP_AGGREGATE verifies nothing), so every intermediate value of the loop
is a known multiple of S.  Each row's event is re-derived here by a
restatement of that loop on integers and asserted; the expected status and
aggregate come from oracle.tbls_oracle.combine_signatures.  Deterministic; it
draws no random numbers (tests/golden/make_golden.py's stream is untouched).

Run from the repository root: python tests/golden/make_agg_exc_golden.py
"""
import json
import os
import sys
from fractions import Fraction
from math import lcm

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import bls12_381 as bls  # noqa: E402
from oracle import tbls_oracle as tb  # noqa: E402

SK = 0x2A5F1C0DE5EED0FA66C0FFEE1234567890ABCDEF0FEDCBA9876543210F00D
MSG = b"aggregation: exceptional cases"

# identifiers, multipliers c, the event the row was chosen for, expected status
ROWS = [
    ((1, 2, 3), (1, -1, 1), "doubling_first_additions", "ok"),
    ((1, 2, 3), (1, 1, 1), "two_cancellations", "ok"),
    ((1, 2, 3), (1, 2, 3), "identity_sum", "identity"),
    ((1, 2, 3), (2, 1, -3), "doubling_then_identity", "identity"),
    ((1, 2, 3, 4), (1, -1, 2, 1), "two_doublings", "ok"),
    ((1, 2, 3, 4), (1, 1, 1, 2), "cancellations_to_identity", "identity"),
    ((1, 2, 4), (1, 1, 2), "doubling_den", "ok"),
    ((1, 2, 4), (1, 1, -2), "identity_den", "identity"),
    ((1, 2, 4), (1, 2, 1), "cancellation_den", "ok"),
    ((2, 3, 4), (2, 1, 2), "cancellation_then_doubling", "ok"),
]


def integer_form(ids):
    """(N, D): lambda_i(0) = N_i / D over the integers, D the common denominator."""
    lam = []
    for i, xi in enumerate(ids):
        v = Fraction(1)
        for j, xj in enumerate(ids):
            if i != j:
                v *= Fraction(xj, xj - xi)
        lam.append(v)
    D = lcm(*[v.denominator for v in lam])
    return [int(v * D) for v in lam], D


def schedule(N, c):
    """combine_int_pair's loop on multiples of S: the accumulator is [a] S.
    Returns the events in order -- ("double", bit, j) where an addition met
    acc == +-N_j's point (the kernel sets exc; here the exact law goes on, so
    later events are still seen), ("cancel", bit, j) where it returned to
    infinity -- and the final multiple."""
    nbits = max(abs(n).bit_length() for n in N)
    a, events = 0, []
    for bit in range(nbits - 1, -1, -1):
        a *= 2
        for j, (n, cj) in enumerate(zip(N, c)):
            if not (abs(n) >> bit) & 1:
                continue
            term = cj if n > 0 else -cj
            if a != 0 and a == term:
                events.append(("double", bit, j))
            elif a != 0 and a == -term:
                events.append(("cancel", bit, j))
            a += term
    return events, a


def check_event(name, N, D, c):
    ev, a = schedule(N, c)
    assert a == sum(n * cj for n, cj in zip(N, c))
    kinds = [e[0] for e in ev]
    nbits = max(abs(n).bit_length() for n in N)
    if name == "doubling_first_additions":
        assert ev[0] == ("double", nbits - 1, 1) and D == 1
    elif name == "two_cancellations":
        assert kinds == ["cancel", "cancel"] and a != 0 and D == 1
    elif name == "identity_sum":
        assert kinds == ["cancel"] and a == 0 and D == 1
    elif name == "doubling_then_identity":
        assert kinds[0] == "double" and a == 0 and D == 1
    elif name == "two_doublings":
        assert kinds == ["double", "double"] and a != 0 and D == 1
    elif name == "cancellations_to_identity":
        assert "double" not in kinds and kinds.count("cancel") >= 2 and a == 0 and D == 1
    elif name == "doubling_den":
        assert kinds == ["double"] and a != 0 and D > 1
    elif name == "identity_den":
        assert kinds == ["cancel"] and a == 0 and D > 1
    elif name == "cancellation_den":
        assert kinds == ["cancel"] and a != 0 and D > 1
    elif name == "cancellation_then_doubling":
        assert kinds == ["cancel", "double"] and a != 0 and D == 1
    else:
        raise AssertionError(name)
    return ev, a


def main():
    S = tb.sign(SK, MSG)
    out = []
    for ids, c, event, status in ROWS:
        N, D = integer_form(ids)
        ev, a = check_event(event, N, D, c)
        pts = [bls.g2_mul(S, cj % bls.R) for cj in c]
        try:
            agg = bls.g2_compress(tb.combine_signatures(list(zip(ids, pts)))).hex()
            got = "ok"
            # the aggregate is [a / D] S
            assert agg == bls.g2_compress(bls.g2_mul(S, a * pow(D, -1, bls.R) % bls.R)).hex()
        except tb.TblsError as e:
            assert "identity aggregate" in str(e) and a == 0
            agg, got = None, "identity"
        assert got == status, (ids, c, got)
        out.append({"label": f"{event}_ids{''.join(map(str, ids))}", "event": event,
                    "integer_form": {"N": N, "D": D}, "multipliers": list(c),
                    "schedule_events": [list(e) for e in ev], "sum_multiple": a,
                    "partials": [{"identifier": i, "sig": bls.g2_compress(p).hex()} for i, p in zip(ids, pts)],
                    "expect": {"status": status, "agg": agg}})
    with open(os.path.join(HERE, "agg_exceptional.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_agg_exc_golden.py", "base_signature": bls.g2_compress(S).hex(),
                   "vectors": out}, f, indent=1)
    print("agg_exceptional.json", len(out))


if __name__ == "__main__":
    main()
