"""Python statements of the engine's planning rules (charon_amd/csrc/tbls_plan.h),
written independently of the C++: the GPU tests predict a launch's shape and
subgroup-test group size from them, and tests/test_plan_host.py compares them
with the C++ on the CPU."""

SGB_M = 1024


def shape_fits(nd0, G0, C0, nd, G, C):
    """Closed form of the replay fit rule (tbls_plan.h shape_fits, there derived
    from the section table): a launch of nd duties at (G, C) in an arena
    sized for nd0 duties at (G0, C0)."""
    ng0, nch0 = -(-nd0 // G0), -(-G0 // C0)
    ng, nch = -(-nd // G), -(-G // C)
    return (ng <= ng0 and ng * (nch + 1) <= ng0 * (nch0 + 1) and ng * nch <= ng0 * nch0
            and ng * nch * C <= ng0 * nch0 * C0 and ng * G <= ng0 * G0
            and max(ng * nch, nd) <= max(ng0 * nch0, nd0) and (G <= 64) == (G0 <= 64))


def expected_shape(nd, n_cu, g_free=True, G=16, fits=lambda g, c: True):
    """Mirror of l0_shape: the hexad cost 0.948 + 1.395 C (M u32 mul-adds,
    profiles/work_model.json) x ceil(waves / SIMDs), SIMDs = CUs x 4, over the
    candidates `fits` keeps (a replay's arenas)."""
    n_simd = n_cu * 4

    def cost(g, c):
        waves = -(-(-(-nd // g) * -(-g // c)) // 10)
        return (0.948 + 1.395 * c) * -(-waves // n_simd)

    if G < 8:
        return G, 4
    cand = [(16 if g_free else G, 4), (16 if g_free else G, 8)] + ([(14, 7)] if g_free else [])
    if g_free:
        cand += [(c, c) for c in range(5, 11)]  # round 6: one chunk per group, 5 .. 10 duties
    best = None
    for gc in cand:
        if fits(*gc) and (best is None or cost(*gc) < cost(*best) - 1e-9):
            best = gc
    return best


def sgb_plan(rho):
    """Mirror of sgb_plan: (on, partials per group)."""
    best, m = None, None
    k = SGB_M
    while k >= 64:
        cost = 0.55 + 1.1 * 18 / k + 1 - (1 - min(rho, 1.0)) ** k
        if best is None or cost < best - 1e-12:
            best, m = cost, k
        k //= 2
    return best < 0.95, m
