"""The scalars every test of the hardened signer runs (shared data, no tests).

VALID: small values around a window's digit range, powers of two and their
predecessors at nibble, word and top-of-scalar positions, the neighbourhood of
r (a regular recoding can meet a doubling in its last addition there), the two
halves of r, a full carry chain of the signed recoding (every nibble 8), a top
nibble of 6 over all ones, and 32 seeded random scalars.
INVALID: what the range check must refuse, with the TBG_KS_* code of each.
"""
import random

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

KS_OK, KS_ZERO, KS_RANGE, KS_MSG = 0, -40, -41, -42

SMALL = [1, 2, 7, 8, 9, 15, 16, 17]
POWERS = [v for k in (4, 8, 128, 252, 254) for v in (1 << k, (1 << k) - 1)]
NEAR_R = [R - 1, R - 2, R - 8, R - 9, R - 16, R - 30]
HALVES = [(R - 1) // 2, (R + 1) // 2]
CARRY_CHAIN = int("8" * 63, 16)
SIX_F = int("6" + "f" * 63, 16)
_rng = random.Random(0xC7A11)
RANDOM = [_rng.randrange(1, R) for _ in range(32)]

VALID = SMALL + POWERS + NEAR_R + HALVES + [CARRY_CHAIN, SIX_F] + RANDOM
assert all(0 < k < R for k in VALID) and len(RANDOM) == 32

INVALID = [(0, KS_ZERO), (R, KS_RANGE), (R + 1, KS_RANGE), ((1 << 256) - 1, KS_RANGE)]


def be32(k: int) -> bytes:
    return int(k).to_bytes(32, "big")
