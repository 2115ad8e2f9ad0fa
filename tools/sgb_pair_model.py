"""Count model of the batched subgroup test's three schedules (k_sgb.hip):
where SGB_PAIR_M, the smallest group on the paired schedule, and SGB_TRI_M,
the triple schedule's group size, come from.

Unit: one lane-pair slot = one lane pair busy for one mixed G2 addition.  A
wave is 32 lane pairs and runs as long as its longest lane, so it is charged
32 x its longest chain.  A Jacobian + Jacobian addition (fold, running sums)
is 16 Fp2 products against the mixed addition's 11: weight 16/11.  The 18
tests per group (63 doublings + 5 additions each) and the unweighted sum T
(one slot per member) are the same in both schedules and left out.

  classic   6 buckets per combination x `split` slices, lane pairs in
            (bucket, slice) order; fold (split - 1 additions on 108 pairs);
            running sums (12 additions on 18 pairs)
  paired    84 buckets per pair of combinations, 768 lane pairs per group in
            index order or ranked by entry count; fold (13 terms on 108
            pairs); running sums as above
  triple    1,098 buckets per triple of combinations, 6,592 lane pairs per
            group ranked by entry count; fold in two passes (per triple 84
            sums P and 72 sums E of 13 terms, 12 sums E of 7 or 6; then 12
            sums of 13 and 6 of 14); running sums as above

Digits are uniform in {-6..6} (sgb_digits is SHA-256 output reduced mod 13;
numpy's generator stands in for it).  Usage: python tools/sgb_pair_model.py
"""
import numpy as np

K, V, PAIRS, PB, TB, WAVE = 18, 6, 9, 84, 1098, 32
JJ = 16.0 / 11.0  # Jacobian + Jacobian addition in mixed additions


def wave_slots(chains):
    """Lane-pair slots of consecutive lane pairs with these chain lengths."""
    n = -(-len(chains) // WAVE) * WAVE
    c = np.zeros(n, dtype=np.int64)
    c[:len(chains)] = chains
    return int(c.reshape(-1, WAVE).max(axis=1).sum()) * WAVE


def classic(d, m):
    split = max(1, 4 * m // 1024)
    chains, adds = [], 0
    for k in range(K):
        for v in range(1, V + 1):
            n = int((np.abs(d[:, k]) == v).sum())
            adds += n
            chains += [n * (s + 1) // split - n * s // split for s in range(split)]
    red = 0.0
    if split > 1:
        red += K * V * (split - 1) * JJ  # fold: every lane the same chain
    red += K * 2 * V * JJ                # running sums
    return adds, wave_slots(chains), red


def paired(d, m, ranked):
    adds, counts = 0, []
    for p in range(PAIRS):
        a, b = d[:, 2 * p].copy(), d[:, 2 * p + 1].copy()
        neg = (a < 0) | ((a == 0) & (b < 0))
        a[neg], b[neg] = -a[neg], -b[neg]
        live = (a != 0) | (b != 0)
        idx = np.where(a == 0, b - 1, V + (a - 1) * (2 * V + 1) + b + V)[live]
        adds += int(live.sum())
        counts += np.bincount(idx, minlength=PB).tolist()
    counts = np.array(counts)
    if ranked:
        counts = np.sort(counts)[::-1]
    red = K * V * (2 * V + 1) * JJ + K * 2 * V * JJ  # fold (13 terms, charged in full), running sums
    return adds, wave_slots(counts), red


def triple(d, m):
    adds, counts = 0, []
    for t in range(K // 3):
        a, b, c = d[:, 3 * t].copy(), d[:, 3 * t + 1].copy(), d[:, 3 * t + 2].copy()
        neg = (a < 0) | ((a == 0) & ((b < 0) | ((b == 0) & (c < 0))))
        a[neg], b[neg], c[neg] = -a[neg], -b[neg], -c[neg]
        live = (a != 0) | (b != 0) | (c != 0)
        idx = ((a * (2 * V + 1) + b + V) * (2 * V + 1) + c + V)[live]  # (any injective index: only the counts matter)
        adds += int(live.sum())
        cnt = np.bincount(idx, minlength=(V + 1) * (2 * V + 1) ** 2)
        counts += np.sort(cnt)[::-1][:TB].tolist()  # the 1,098 buckets that exist (the others are never hit)
    counts = np.sort(np.array(counts))[::-1]
    row = 2 * V + 1
    fold1 = PB * row + V * (2 * V * row + (V + 1) + V)  # P; E(v, a >= 1, +-), E(v, 0, +), E(v, 0, -)
    fold2 = 2 * V * row + V * 2 * (V + 1)
    red = (K // 3) * (fold1 + fold2) * JJ + K * 2 * V * JJ
    return adds, wave_slots(counts), red


def large_groups(rng):
    """Paired (stretched past SGB_M, as a yardstick) against triple."""
    print()
    print("     m | paired adds ranked +red  total | triple adds ranked  +red  total")
    for m in (1024, 4096, 8192, 16384, 32768):
        groups = max(2, 32768 // m)
        acc = np.zeros(6)
        for _ in range(groups):
            d = rng.integers(-6, 7, size=(m, K))
            pa, pk, pr = paired(d, m, True)
            ta, tk, tr = triple(d, m)
            acc += [pa, pk, pr, ta, tk, tr]
        pa, pk, pr, ta, tk, tr = acc / (groups * m)
        print(f"{m:6d} | {pa:10.2f} {pk:6.2f} {pr:5.2f} {pk + pr:6.2f} | {ta:10.2f} {tk:6.2f} {tr:5.2f} {tk + tr:6.2f}")


def main():
    rng = np.random.default_rng(0x5B)
    print("  m | classic adds slots +red | paired adds  index ranked +red | classic total  paired total")
    for m in (64, 128, 256, 512, 1024):
        groups = max(8, 8192 // m)
        acc = np.zeros(7)
        for _ in range(groups):
            d = rng.integers(-6, 7, size=(m, K))
            ca, cs, cr = classic(d, m)
            pa, pi, pr = paired(d, m, False)
            _, pk, _ = paired(d, m, True)
            acc += [ca, cs, cr, pa, pi, pk, pr]
        ca, cs, cr, pa, pi, pk, pr = acc / (groups * m)
        print(f"{m:5d} | {ca:7.2f} {cs:6.2f} {cr:6.2f} | {pa:7.2f} {pi:6.2f} {pk:6.2f} {pr:6.2f} |"
              f" {cs + cr:8.2f} {pk + pr:12.2f}")
    large_groups(rng)


if __name__ == "__main__":
    main()
