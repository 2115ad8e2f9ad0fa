"""The fallback lists' pass schedule and the grid-stride loops of the shrunk
passes (charon_amd/csrc/tbls_launch.h fb_passes, fb_pass_loop; the slot
geometry hex_slot / hex_threads / hex_slots_of of bls_hex.h and
pair_slots_of) on the CPU, through the host twin tests/plan.

A pass of the level-2b or level-3 list past DevBatch::fb_full starts grids of
FB_SMALL = 640 list positions, and each hexad (k_verify_list,
k_rlc_ident_check) or lane pair (k_lines_sig_list, k_lines_fold) walks
first, first + stride, ... through the pass.  pl_fb_cover runs the real
fb_passes, builds for every pass the grid its launcher starts, finds each
thread's slot as the kernels do and runs the real fb_pass_loop once per slot.
What is asserted per pass:

  * the schedule is the one stated here independently (expected_passes): a
    pass is shrunk exactly when may_shrink, base > 0, base >= fb_full and
    n > 640 all hold;
  * every list position of [base, min(base + fb_w, count)) is visited once,
    in that pass, and nothing else is (a stride too large skips entries, one
    too small checks an entry twice against another entry's lines);
  * every line-buffer slot formed is inside the buffer of fb_w entries;
  * the stride equals the slots of the grid, and a shrunk pass holding more
    than 640 entries makes some walker run its body twice or more.
"""
import numpy as np
import pytest

from tests.plan import lib

U32_MAX = 0xFFFFFFFF
FB_SMALL = 640
HEX, PAIR = 0, 1
KINDS = {"hexad": HEX, "pair": PAIR}
WINDOWS = [1, 64, 640, 641, 1003, 1507, 32768]


def expected_passes(fb_w, fb_full, max_entries, may_shrink):
    """[(base, n, shrunk)]: the passes over [0, max_entries) in windows of fb_w."""
    out = []
    for base in range(0, max_entries, fb_w):
        n = min(fb_w, max_entries - base)
        out.append((base, n, bool(may_shrink and base > 0 and base >= fb_full and n > FB_SMALL)))
    return out


def grid_slots(n, kind):
    """List positions the launcher's grid for n positions holds (blocks of 64 threads)."""
    if kind == HEX:
        return -(-n // 10) * 10  # grid_for(hex_threads(n)): whole waves of 10 hexads
    return -(-2 * n // 64) * 32  # grid_for(2 n): whole waves of 32 pairs


class Cover:
    """pl_fb_cover with buffers sized once for a (fb_w, max_entries)."""

    def __init__(self, fb_w, max_entries):
        self.fb_w, self.max_entries = fb_w, max_entries
        self.max_passes = max_entries // fb_w + 2
        self.passes = np.zeros((self.max_passes, 6), dtype=np.uint64)
        self.trips = np.zeros(7 * max_entries + 128 * self.max_passes, dtype=np.uint32)
        self.hits = np.zeros(max(1, max_entries), dtype=np.uint32)
        self.hit_pass = np.zeros(max(1, max_entries), dtype=np.uint32)

    def run(self, fb_full, count, may_shrink, kind):
        self.hits[:] = 0
        self.hit_pass[:] = U32_MAX
        n = lib().pl_fb_cover(self.fb_w, fb_full, count, self.max_entries, int(may_shrink), kind,
                              self.passes.ctypes.data, self.max_passes, self.trips.ctypes.data, len(self.trips),
                              self.hits.ctypes.data, self.hit_pass.ctypes.data)
        assert n >= 0, ("pl_fb_cover", n)
        return [dict(base=int(r[0]), n=int(r[1]), stride=int(r[2]), walkers=int(r[3]),
                     trips=self.trips[int(r[4]):int(r[4]) + int(r[3])], max_slot=int(r[5])) for r in self.passes[:n]]


def check(cov, fb_full, count, may_shrink, kind):
    """Every assertion of this module on one list; the number of shrunk passes that looped."""
    fb_w, max_entries = cov.fb_w, cov.max_entries
    what = dict(fb_w=fb_w, fb_full=fb_full, count=count, max_entries=max_entries, may_shrink=may_shrink, kind=kind)
    got = cov.run(fb_full, count, may_shrink, kind)
    want = expected_passes(fb_w, fb_full, max_entries, may_shrink)
    assert [(g["base"], g["n"]) for g in got] == [(b, FB_SMALL if s else n) for b, n, s in want], what
    # coverage: each listed position once, in its own pass; nothing past the list
    miss = np.flatnonzero(cov.hits[:count] != 1)
    assert miss.size == 0, (what, "positions not visited exactly once", miss[:8], cov.hits[miss[:8]])
    assert not cov.hits[count:].any(), what
    assert np.array_equal(cov.hit_pass[:count], np.arange(count, dtype=np.uint32) // fb_w), what
    looped = 0
    words = lib().pl_lines_words()
    for g, (base, n, shrunk) in zip(got, want):
        held = min(max(count - base, 0), fb_w)  # list entries in this pass
        assert g["walkers"] == grid_slots(g["n"], kind), (what, g)
        assert g["stride"] == g["walkers"], (what, g)
        assert int(g["trips"].sum()) == held, (what, g)
        assert g["max_slot"] < fb_w * words and g["max_slot"] == words * max(held - 1, 0), (what, g)
        top = int(g["trips"].max())
        assert top == -(-held // g["walkers"]), (what, g)
        if not shrunk:
            assert top <= 1, (what, g)
        elif held > FB_SMALL:
            assert g["n"] == FB_SMALL and top >= 2, (what, g)
            looped += 1
    return looped


def counts_for(fb_w, max_entries, step):
    """List lengths 0..max_entries: every value within 1 of a multiple of the window, of the small grid and of
    their sum, and every step-th one between."""
    c = {0, max_entries}
    for m in (fb_w, FB_SMALL, fb_w + FB_SMALL):
        for q in range(max_entries // m + 2):
            c.update((q * m - 1, q * m, q * m + 1))
    c.update(range(0, max_entries + 1, step))
    return sorted(x for x in c if 0 <= x <= max_entries)


def test_constants():
    assert lib().pl_fb_small() == FB_SMALL


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("fb_w", WINDOWS)
def test_every_pass_covers_its_window_once(fb_w, kind):
    # lists up to five windows (the default window: two and the start of a third, which is shrunk past 2 fb_w)
    max_entries = 5 * fb_w + 7 if fb_w < 32768 else 2 * fb_w + 2 * FB_SMALL + 20
    step = 1 if max_entries <= 400 else 29 if fb_w < 32768 else 9973
    cov = Cover(fb_w, max_entries)
    looped = 0
    for may_shrink in (False, True):
        # (fb_full is read only when a pass may shrink)
        for fb_full in ((fb_w, 2 * fb_w, 3 * fb_w, U32_MAX) if may_shrink else (fb_w,)):
            for count in counts_for(fb_w, max_entries, step):
                looped += check(cov, fb_full, count, may_shrink, KINDS[kind])
    # the windows above the small grid did reach passes whose walkers loop
    assert (looped > 0) == (fb_w > FB_SMALL)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("max_entries,count,loops", [
    (33408, 33408, 0),   # the second pass holds 640 positions: a full grid
    (40000, 33408, 0),   # shrunk, and every walker runs at most once
    (40000, 33409, 1),   # the first list length at which a walker runs twice
    (40000, 40000, 1),
])
def test_default_window_in_a_fresh_context(max_entries, count, loops, kind):
    """The default shape: fb_window = 32,768 and, with no invalid partial
    collected yet, fb_full = fb_window -- the second pass of a list past
    33,408 positions runs on the small grid."""
    fb_w = 32768
    want = expected_passes(fb_w, fb_w, max_entries, True)
    assert [s for _, _, s in want] == [False, max_entries > fb_w + FB_SMALL]
    assert check(Cover(fb_w, max_entries), fb_w, count, True, KINDS[kind]) == loops
