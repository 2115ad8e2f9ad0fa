#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, object by object and function
by function: the check that a refactor left the kernels as they were.

  python tools/device_code_diff.py charon_amd/build_obj/A charon_amd/build_obj/B

A and B are object directories of charon_amd._native.build (one per output
library).  Per object the gfx950 code object is disassembled
(_native.device_functions: llvm-objdump -d --no-show-raw-insn
--no-leading-addr; the "// address: encoding" comment that this disassembler
still appends to every instruction is dropped, as those flags ask) and every
function's instructions compared.  Two things are normalised, both layout and
not code:
  - the 32-bit literal of the s_add_u32 / s_addc_u32 pair that follows an
    s_getpc_b64 (a PC-relative call or data address: it moves when anything
    before it in the code object grows or shrinks);
  - the run of `s_nop 0` at a function's end (alignment padding).
Prints the functions only in A, only in B and those that differ; exit status 1
if any list is non-empty (--diff also prints each differing function's
unified diff).
"""
import argparse
import difflib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from charon_amd import _native  # noqa: E402

FLAGS = ("--no-show-raw-insn", "--no-leading-addr")
_LIT = re.compile(r",\s*(0x[0-9a-fA-F]+|-?\d+)\s*$")


def normalise(body: str):
    lines = [ln.split("//")[0].strip() for ln in body.splitlines()]
    lines = [ln for ln in lines if ln]
    # the literals of the s_add_u32 / s_addc_u32 pair after an s_getpc_b64
    pending = []
    for i, ln in enumerate(lines):
        op = ln.split()[0]
        if op == "s_getpc_b64":
            pending = ["s_add_u32", "s_addc_u32"]
        elif pending and op == pending[0]:
            lines[i] = _LIT.sub(", <pcrel>", ln)
            pending.pop(0)
    while lines and re.fullmatch(r"s_nop\s+0", lines[-1]):
        lines.pop()
    return lines


def functions_of(objdir: str):
    """{(object, function): normalised lines} over the device objects of objdir"""
    out = {}
    for f in sorted(os.listdir(objdir)):
        if not f.endswith(".o"):
            continue
        code = _native.device_functions(os.path.join(objdir, f), FLAGS)
        if code is None:
            continue  # host-only unit
        for name, body in code[0]:
            out[(f, name)] = normalise(body)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--diff", action="store_true", help="print the unified diff of every differing function")
    args = ap.parse_args()
    fa, fb = functions_of(args.a), functions_of(args.b)
    only_a = sorted(set(fa) - set(fb))
    only_b = sorted(set(fb) - set(fa))
    differ = sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
    print(f"{len(set(fa) & set(fb))} functions in both, {len(set(fa) & set(fb)) - len(differ)} identical")
    for title, keys in ((f"only in {args.a}", only_a), (f"only in {args.b}", only_b), ("differ", differ)):
        print(f"{title}: {len(keys)}")
        for obj, name in keys:
            print(f"  {obj}: {name}")
    if args.diff:
        for k in differ:
            print("\n".join(difflib.unified_diff(fa[k], fb[k], f"{args.a}/{k[0]}:{k[1]}", f"{args.b}/{k[0]}:{k[1]}",
                                                 lineterm="", n=2)))
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
