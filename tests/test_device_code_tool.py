"""The device-code helpers on disassembly text (no GPU, no compiler): the
listing split and return-address test that _native.check_return_address is
made of, and what tools/device_code_diff.py normalises before it compares."""
from charon_amd import _native
from tools import device_code_diff as dcd

# llvm-objdump -d, default flags: leading addresses, "// address: encoding" comments
LISTING = """
co:\tfile format elf64-amdgpu

Disassembly of section .text:

0000000000001000 <_ZN3tbg6kernelENS_8DevBatchE>:
\ts_getpc_b64 s[30:31]                                       // 000000001000: BE9E1C00
\ts_add_u32 s30, s30, 0x7c5d0                                // 000000001004: 801EFF1E 0007C5D0
\ts_cbranch_scc0 6                                           // 00000000100C: BF840006 <_ZN3tbg6kernelENS_8DevBatchE+0x40>
\ts_endpgm                                                   // 000000001010: BF810000

0000000000002000 <_ZN3tbg7jac_addINS_3Fp2EEENS_3JacIT_EERKS4_S6_>:
\ts_getpc_b64 s[30:31]                                       // 000000002000: BE9E1C00
\ts_setpc_b64 s[30:31]                                       // 000000002004: BE801D1E

0000000000003000 <_ZN3tbg7jac_dblINS_3Fp2EEENS_3JacIT_EERKS4_>:
\ts_getpc_b64 s[16:17]                                       // 000000003000: BE901C00
\ts_setpc_b64 s[30:31]                                       // 000000003004: BE801D1E
"""
KERNEL = "_ZN3tbg6kernelENS_8DevBatchE"
JAC_ADD = "_ZN3tbg7jac_addINS_3Fp2EEENS_3JacIT_EERKS4_S6_"
JAC_DBL = "_ZN3tbg7jac_dblINS_3Fp2EEENS_3JacIT_EERKS4_"


def test_split_functions_with_and_without_leading_addresses():
    fs = _native.split_functions(LISTING)
    assert [n for n, _ in fs] == [KERNEL, JAC_ADD, JAC_DBL]
    assert "s_endpgm" in fs[0][1] and "s_endpgm" not in fs[1][1]
    # a branch target's "<name+0x40>" in a comment does not start a function
    assert "s_cbranch_scc0" in fs[0][1]
    import re
    bare = re.sub(r"^[0-9a-f]{16} <", "<", LISTING, flags=re.M)  # --no-leading-addr
    assert [n for n, _ in _native.split_functions(bare)] == [KERNEL, JAC_ADD, JAC_DBL]


def test_return_address_clobber_is_refused_in_callable_functions_only():
    fs = _native.split_functions(LISTING)
    # the kernel may use s[30:31]; jac_dbl's long branch goes through another pair
    assert _native.return_address_clobbers(fs, {KERNEL}) == [JAC_ADD]
    assert _native.return_address_clobbers(fs, set()) == [KERNEL, JAC_ADD]


def test_normalise_masks_pc_relative_literals_and_end_padding_only():
    body = """
\ts_add_u32 s12, s0, 0x348
\ts_getpc_b64 s[98:99]                                       // 0000000C7B28: BEE21C00
\ts_add_u32 s98, s98, 0x7c5d0                                // 0000000C7B2C: 8062FF62 0007C5D0
\ts_addc_u32 s99, s99, 0                                     // 0000000C7B34: 8263FF63 00000000
\ts_setpc_b64 s[98:99]
\ts_add_u32 s12, s0, 0x348
\ts_nop 0
\tv_mov_b32_e32 v0, 0x577a
\ts_endpgm
\ts_nop 0
\ts_nop 0
"""
    assert dcd.normalise(body) == [
        "s_add_u32 s12, s0, 0x348",  # not after an s_getpc_b64: a real operand
        "s_getpc_b64 s[98:99]",
        "s_add_u32 s98, s98, <pcrel>",
        "s_addc_u32 s99, s99, <pcrel>",
        "s_setpc_b64 s[98:99]",
        "s_add_u32 s12, s0, 0x348",  # the pair is masked once per s_getpc_b64
        "s_nop 0",  # inside the function: kept
        "v_mov_b32_e32 v0, 0x577a",
        "s_endpgm",
    ]
    moved = body.replace("0x7c5d0", "0x7c584")
    assert dcd.normalise(moved) == dcd.normalise(body)
    assert dcd.normalise(body.replace("0x577a", "0x577b")) != dcd.normalise(body)
