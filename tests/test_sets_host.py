"""CPU tests of the all-or-nothing set verification's host layers
(Eth2Verifier.verify_sets_drop, ParSigEx(drop_only=True), the C header): sets
with a host-detected fault never reach the engine and keep verify_sets'
messages, only clean sets are forwarded, and tbls_gpu.h stays plain C."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from charon_amd import engine as eng
from charon_amd import parsig, signing
from charon_amd.parsig import Duty, ParSignedData

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class NoEngine:
    """Stands in for the GPU engine where the host must decide alone."""
    uid = -1

    def __getattr__(self, name):
        raise AssertionError(f"GPU engine used ({name}) on a host-only path")


def _pd(root=b"\x01" * 32, sig=b"\x02" * 96, idx=1, domain=signing.DOMAIN_BEACON_ATTESTER):
    return ParSignedData(domain, 3, root, sig, idx)


def test_verify_sets_drop_host_faults_never_touch_the_engine():
    pubshares = {"dv1": {1: bytes(48), 2: bytes(48)}}
    v = parsig.Eth2Verifier(signing.Spec(), pubshares, engine=NoEngine())
    duty = Duty(10, parsig.DUTY_ATTESTER)
    sets = [(duty, {"dvX": _pd()}),
            (duty, {"dv1": _pd(idx=7)}),
            (duty, {"dv1": _pd(sig=bytes(96))}),
            (duty, {"dv1": _pd(sig=b"\x02" * 95)}),
            (duty, {"dv1": _pd(domain="NO_SUCH_DOMAIN")}),
            (duty, {})]
    got = v.verify_sets_drop(sets)
    want = v.verify_sets(sets)  # (host-only too: every item is rejected before the GPU)
    assert [str(g) for g in got[:5]] == [str(w) for w in want[:5]]
    assert "unknown pubkey" in str(got[0])
    assert "invalid shareIdx" in str(got[1])
    assert "invalid signature" in str(got[2]) and "no signature found" in str(got[2]) and "duty=" in str(got[2])
    assert "invalid length" in str(got[3])
    assert "domain type not found" in str(got[4])
    assert got[5] is None and want[5] is None  # an empty set verifies
    assert all(isinstance(g, parsig.ParSigError) for g in got[:5])


class StubEngine:
    """An engine whose set launches return canned statuses."""
    uid = -2

    def __init__(self, statuses):
        self.statuses = list(statuses)
        self.calls = []

    def load_pubkeys(self, pk48):
        n = len(bytes(pk48)) // 48
        return 0, np.zeros(n, dtype=np.int32)

    def run_sets(self, set_first, duty_first, sigs, identifiers, **kw):
        set_first = [int(x) for x in set_first]
        self.calls.append(set_first)
        assert len(set_first) - 1 == len(self.statuses)
        assert set_first[-1] == len(duty_first) - 1 == len(bytes(sigs)) // 96
        return eng.SetsResult(np.array(self.statuses, dtype=np.int32), np.zeros(set_first[-1], dtype=np.int32))


def test_parsigex_drop_only_forwards_only_clean_sets():
    pubshares = {"dv1": {1: bytes([1]) * 48, 2: bytes([2]) * 48}, "dv2": {1: bytes([3]) * 48}}
    stub = StubEngine([eng.SS_VALID, eng.SS_INVALID, eng.SS_ERROR, eng.SS_VALID])
    v = parsig.Eth2Verifier(signing.Spec(), pubshares, engine=stub)
    ex = parsig.ParSigEx(v, drop_only=True)
    got = []
    ex.subscribe(lambda d, s: got.append((d.slot, sorted(s))))
    sets = [(Duty(1, parsig.DUTY_ATTESTER), {"dv1": _pd(idx=1), "dv2": _pd(idx=1)}),
            (Duty(2, parsig.DUTY_ATTESTER), {"dv1": _pd(idx=2)}),
            (Duty(3, parsig.DUTY_ATTESTER), {"dv1": _pd(idx=9)}),           # host fault: off the GPU
            (Duty(4, parsig.DUTY_ATTESTER), {"dv2": _pd(idx=1)}),
            (Duty(5, parsig.DUTY_ATTESTER), {"dv1": _pd(idx=1), "dv2": _pd(idx=1)})]
    verdicts = ex.handle_batch(sets)
    assert stub.calls == [[0, 2, 3, 4, 6]]  # one set launch, the host-rejected set left out
    assert verdicts[0] is None and verdicts[4] is None
    assert str(verdicts[1]) == f"invalid signature: set failed verification (duty={sets[1][0]})"
    assert "invalid shareIdx" in str(verdicts[2])
    assert str(verdicts[3]) == f"invalid signature: set failed verification (duty={sets[3][0]})"
    assert got == [(1, ["dv1", "dv2"]), (5, ["dv1", "dv2"])]
    # the default stays the per-partial path
    assert parsig.ParSigEx(v).drop_only is False


def test_header_with_set_entry_points_is_plain_c(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None and os.path.exists("/opt/rocm/llvm/bin/clang"):
        cc = "/opt/rocm/llvm/bin/clang"
    assert cc, "no C compiler"
    src = tmp_path / "sets_abi.c"
    src.write_text('#include "tbls_gpu.h"\n'
                   "void* const set_entry_points[3] = {(void*)tbg_submit_sets, (void*)tbg_collect_sets, "
                   "(void*)tbg_fetch_sets};\n"
                   "int set_codes_ordered[(TBG_SS_ERROR < TBG_SS_INVALID && TBG_SS_INVALID < TBG_SS_VALID) ? 1 : -1];\n")
    r = subprocess.run([cc, "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_constants_match_the_header():
    import re
    text = open(os.path.join(ROOT, "include", "tbls_gpu.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define (TBG_SS_\w+) (\d+)", text)}
    assert (vals["TBG_SS_ERROR"], vals["TBG_SS_INVALID"], vals["TBG_SS_VALID"]) == \
        (eng.SS_ERROR, eng.SS_INVALID, eng.SS_VALID)
    ds = {int(v) for v in re.findall(r"#define TBG_DS_\w+ \(?(-?\d+)\)?", text)}
    assert not ds & set(vals.values())
