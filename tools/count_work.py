#!/usr/bin/env python3
"""Freeze the algorithmic work model of the engine's per-item schedule.

Builds the host copy of the device math with TBG_COUNT_OPS (every Montgomery
product / square / reduction adds its u32 multiply-add count) and measures
one item of each pipeline stage on real inputs from the golden fixtures.
Writes profiles/work_model.json, which bench.py uses for roofline.achieved.
One Fp multiplication = 392 u32 mul-adds in this radix-2^28 schedule
(196 a*b + 196 m*p); the survey's 12x32-bit CIOS figure is 300.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import twin_build  # noqa: E402  (the TBG_COUNT_OPS builds are entries of its table)
L0_DUTY_PARTIALS = 600000  # include/tbls_gpu.h TBG_L0_DUTY_PARTIALS


def main():
    lib = twin_build.lib("hostcheck_count")
    lib.hc_count_get.restype = ctypes.c_ulonglong
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "cfg1_3of4_single.json")))["vectors"][0]
    msg = bytes.fromhex(gold["msg"])
    sigs = [bytes.fromhex(p["sig"]) for p in gold["partials"]]
    pks = [bytes.fromhex(gold["tss"]["pubshares"][str(p["identifier"])]) for p in gold["partials"]]

    def measure(fn, *a):
        lib.hc_count_reset()
        r = fn(*a)
        return lib.hc_count_get(), r

    decode, st = measure(lib.hc_stage_decode_sig, sigs[0])
    assert st == 0
    hash_, _ = measure(lib.hc_stage_hash, msg, len(msg))
    lib.hc_count_reset()
    assert lib.hc_stage_verify(pks[0], sigs[0], msg, len(msg)) == 1
    verify = lib.hc_count_get()
    lib.hc_count_reset()
    assert lib.hc_stage_lines(sigs[0], msg, len(msg)) == 0
    lines_sig = lib.hc_count_get()
    # H lines (per message, k_lines_h): the projective steps of bls_pair.h
    # (hline_dbl_s / hline_add_s, 2 products + 7 squarings per tangent step),
    # l1 and l4 stored unevaluated.  Probe: tests/hlines/hlines_host.cpp built
    # with TBG_COUNT_OPS, both lanes of the pair counted.  (The signature side
    # keeps the Jacobian steps: lines_sig above.)
    hlib = twin_build.lib("hlines_count")
    hlib.hl_count_get.restype = ctypes.c_ulonglong
    h_aff = ctypes.create_string_buffer(192)
    assert hlib.hl_hash(msg, len(msg), h_aff) == 0
    hlib.hl_count_reset()
    hlib.hl_probe_lines(h_aff)
    lines_h = hlib.hl_count_get()
    lines_h_jacobian = lines_sig - 68 * 4 * 392  # the same 68 steps in Jacobian form with P left out (before)
    lib.hc_count_reset()
    assert lib.hc_stage_verify_quad(pks[0]) == 1
    verify_quad = lib.hc_count_get()
    out = ctypes.create_string_buffer(96)
    ids = bytes([p["identifier"] for p in gold["partials"]])
    lib.hc_count_reset()
    assert lib.hc_stage_aggregate(ids, b"".join(sigs), len(sigs), out) == 0
    agg_with_decode = lib.hc_count_get()
    assert out.raw.hex() == gold["expect"]["agg"]
    agg = agg_with_decode - len(sigs) * decode
    # RLC schedule (k_rlc.hip), default group G = 16 duties, chunk C = 4 duties
    G, C = 16, 4
    for fn in ("hc_stage_setup", "hc_stage_rlc_partial", "hc_stage_duty_sum", "hc_stage_group_lines",
               "hc_stage_miller_chunk", "hc_stage_group_final"):
        getattr(lib, fn).restype = ctypes.c_int
    lib.hc_stage_rlc_partial.argtypes = [ctypes.c_uint64]
    assert lib.hc_stage_setup(sigs[0], pks[0], msg, len(msg)) == 0
    rlc_partial, _ = measure(lib.hc_stage_rlc_partial, 0x9E3779B97F4A7C15)
    duty_sum4, _ = measure(lib.hc_stage_duty_sum, 4)
    group_lines8, _ = measure(lib.hc_stage_group_lines, G)
    # hc_stage_miller_chunk forms its line products as the trio does (quad_line_lane, the Karatsuba
    # form: five REDC(ab + cd) per hexad lane); the kernels run the hexad's direct form (bls_hex.h
    # hex_line_mul: two fp_mul_sum<6> per lane).  Probe: tests/hexline/hexline_host.cpp built with
    # TBG_COUNT_OPS counts one line product over the six lanes in either form; every line product of a
    # measured chunk is corrected by the difference (miller_chunk below: 68 lines per duty pair and for
    # the folded S).
    xlib = twin_build.lib("hexline_count")
    xlib.hxl_hc_count.restype = ctypes.c_ulonglong
    line_direct, line_kara = xlib.hxl_hc_count(0), xlib.hxl_hc_count(1)
    assert line_direct == 6 * 2 * 7 * 196 and line_kara - line_direct == 6 * (196 + 2 * 14), (line_direct, line_kara)
    line_delta = line_kara - line_direct  # 224 per lane and line: one product's 196, two fp_reduce at 14

    def miller_chunk(pairs, folded):
        """hc_stage_miller_chunk with its 68 * (pairs + folded) line products in the direct form."""
        n, _ = measure(lib.hc_stage_miller_chunk, pairs, folded)
        return n - 68 * (pairs + folded) * line_delta
    chunk2 = miller_chunk(C, 0)
    chunk2f = miller_chunk(C, 1)
    final4, _ = measure(lib.hc_stage_group_final, G // C)
    rlc_check_per_group = chunk2f + (G // C - 1) * chunk2 + final4
    # Level 0 (k_msm.hip): per partial the G1 table product and 4 bucket
    # additions; per duty the G1-only sum; per group its P chunks and the
    # products folding them (nch quad products, tree included); per launch
    # the bucket scalings (sampled over j), the tree sums, S's lines, S's
    # Miller quad and ONE final exponentiation.
    for fn in ("hc_stage_l0_partial", "hc_stage_duty_sum_p", "hc_stage_l0_bucket_scale", "hc_stage_g2_add"):
        getattr(lib, fn).restype = None
    lib.hc_stage_l0_partial.argtypes = [ctypes.c_uint64]
    lib.hc_stage_l0_bucket_scale.argtypes = [ctypes.c_uint32]
    l0_partial, _ = measure(lib.hc_stage_l0_partial, 0x9E3779B97F4A7C15)
    duty_sum_p4, _ = measure(lib.hc_stage_duty_sum_p, 4)
    step = 61
    scale_sample = [measure(lib.hc_stage_l0_bucket_scale, 2 * j + 1)[0] for j in range(0, 32768, step)]
    bucket_scales = sum(scale_sample) * 32768 / len(scale_sample)
    g2_add, _ = measure(lib.hc_stage_g2_add)
    final1, _ = measure(lib.hc_stage_group_final, 1)
    qmul = measure(lib.hc_stage_group_final, 2)[0] - final1
    s_quad = miller_chunk(0, 1)
    nch = G // C
    # a P-chunk hexad of c duties costs base + c * per_duty (62 squarings, 68
    # line products per duty): the level-0 launch shape (G, C) varies with the
    # launch size (tbls_plan.h l0_shape), so the kernels' models are per
    # chunk and per duty
    chunk8 = miller_chunk(8, 0)
    chunk_per_duty = (chunk8 - chunk2) / 4
    chunk_base = chunk2 - 4 * chunk_per_duty
    # per-kernel probes (one item of each kernel of the level-0 chain)
    for fn in ("hc_k_decode_sigs", "hc_k_subgroup_sigs"):
        getattr(lib, fn).restype = ctypes.c_int
    for fn in ("hc_k_hash_map", "hc_k_hash_sswu", "hc_k_hash_clear_setup", "hc_k_hash_clear_x1", "hc_k_hash_clear_x2",
               "hc_k_hash_clear_fin", "hc_k_g2_affine", "hc_k_rlc_g1_l0", "hc_k_msm_entry"):
        getattr(lib, fn).restype = None
    lib.hc_k_rlc_g1_l0.argtypes = [ctypes.c_uint64]
    lib.hc_k_msm_entry.argtypes = [ctypes.c_uint32]
    k_decode, st = measure(lib.hc_k_decode_sigs, sigs[0])
    assert st == 0
    k_subgroup, st = measure(lib.hc_k_subgroup_sigs, sigs[0])
    assert st == 1
    k_hash_map, _ = measure(lib.hc_k_hash_map, msg, len(msg))
    k_hash_sswu, _ = measure(lib.hc_k_hash_sswu)
    lib.hc_k_hash_clear_setup(msg, len(msg))
    k_clear_x1, _ = measure(lib.hc_k_hash_clear_x1)
    k_clear_x2, _ = measure(lib.hc_k_hash_clear_x2)
    k_clear_fin, _ = measure(lib.hc_k_hash_clear_fin)
    k_g2_aff, _ = measure(lib.hc_k_g2_affine)
    k_g1_l0, _ = measure(lib.hc_k_rlc_g1_l0, 0x9E3779B97F4A7C15)
    k_msm_entry = sum(measure(lib.hc_k_msm_entry, k)[0] for k in range(4)) / 4
    # Montgomery's trick over a workgroup (bls_batchinv.h): its per-value cost
    # replaces one fp_inv in every batched kernel (k_hash_map's SSWU
    # denominator, k_hash_affine, k_rlc_duty_sum, k_aggregate)
    for fn in ("hc_fp_inv_once", "hc_batch_inv_cost"):
        getattr(lib, fn).restype = None
    lib.hc_batch_inv_cost.argtypes = [ctypes.c_int, ctypes.c_int]
    fp_inv_cost, _ = measure(lib.hc_fp_inv_once)
    binv_n = 256 * 8
    binv_item = measure(lib.hc_batch_inv_cost, binv_n, 4)[0] / binv_n
    saved = fp_inv_cost - binv_item  # per batched inversion
    k_hash_map -= saved
    k_g2_aff -= saved
    agg -= saved
    duty_sum_p4 -= saved
    duty_sum4 -= saved
    rlc_partial -= saved  # (k_rlc_partial2_list: the n2 inversion batched; the G1 product from the key's table)
    hash_ -= 2 * saved
    # batched subgroup test (k_sgb.hip) of the launch this model prices, 16
    # batches of 10k DVs = 640,000 partials: the triple schedule in groups of
    # SGB_TRI_M = 16384 (18 combinations with digits uniform mod 13 taken
    # three at a time, 2196/2197 of the digit triples non-zero): per partial
    # 6 * 2196 / 2197 mixed additions into buckets; per group and triple of
    # combinations the first pass's 84 sums P and 72 sums E of 13 bucket sums
    # and 12 sums E of 7 or 6, the second pass's 12 sums of 13 and 6 of 14 (one
    # addition less than terms each, the empty buckets' trivial ones counted in
    # full), per combination the running sums over 6 of them and one
    # psi(Q) == [x]Q test on a Jacobian Q (the affine test with its 5 mixed
    # additions full).  (Launches below tbg_config.sgb_tri_partials run the
    # paired schedule in groups of 1,024: 9 * 168 / 169 additions per partial
    # and 9 * 12 * 12 fold additions per group.)
    madd, _ = measure(lib.hc_k_msm_entry, 0)  # k = 0: psi^0, one mixed addition
    sgb_m, sgb_k = 16384, 18
    sgb_bucket = sgb_k / 3 * 2196 / 2197 * madd
    sgb_fold1 = 84 * 12 + 6 * (12 * 12 + 6 + 5)  # P; per v: E(v, a >= 1, +-), E(v, 0, +), E(v, 0, -)
    sgb_fold2 = 12 * 12 + 6 * 13
    sgb_fold = sgb_k / 3 * (sgb_fold1 + sgb_fold2) * g2_add / sgb_m
    sgb_combine = sgb_k * 12 * g2_add / sgb_m  # the running sums over the 6 folded sums
    sgb_test = sgb_k * (k_subgroup + 5 * (g2_add - madd)) / sgb_m
    sgb_per_partial = sgb_bucket + sgb_fold + sgb_combine + sgb_test
    decode_sgb = k_decode + sgb_per_partial
    l0_per_group = nch * chunk2 + nch * qmul
    l0_per_launch = bucket_scales + (32768 + 2048 + 128 + 8) * g2_add + lines_h + s_quad + final1
    launch_dvs = 16 * 10000  # bench default: 16 batches of 10k DVs per launch
    unit_3of4_l0_alone = (4 * decode + hash_ + lines_h + 4 * l0_partial + duty_sum_p4 + l0_per_group / G + agg
                          + l0_per_launch / launch_dvs)
    # the bucket-MSM chain with the batched subgroup test (before the fused level 0)
    unit_3of4_l0_msm = unit_3of4_l0_alone - 4 * decode + 4 * decode_sgb
    # Fused level 0 (round 7; bls_rlc.h top, bls_l0tail.h): with the
    # batched subgroup test on, S comes from that test's sums.  Per partial:
    # one more mixed addition (the unweighted sum T, k_sgb_bucket) and the
    # 10 + 8-window key product (no bucket additions); per launch the sums of
    # the 18 Q_k slots and T's slices over the groups (one addition per
    # point) and the Horner chain -- since round 16, in launches of at least
    # TBG_L0_TAIL_PARTIALS partials, the S role of k_rlc_g1_l0's own grid, a
    # per-launch term of that kernel; k_l0f_* in smaller launches.  Probes:
    # tests/l0fused/l0fused_host.cpp built with TBG_COUNT_OPS.
    flib = twin_build.lib("l0fused_count")
    flib.l0f_hc_count_get.restype = ctypes.c_ulonglong

    def fmeasure(fn, *a):
        flib.l0f_hc_count_reset()
        r = fn(*a)
        return flib.l0f_hc_count_get(), r

    assert flib.l0f_hc_probe_setup(pks[0], sigs[0]) == 0
    digit_sets = [[6] * 18, [-6] * 18, [1, -2, 3, -4, 5, -6, 0, 2, -1, 4, -3, 6, -5, 1, 0, -2, 3, -6]]
    l0f_g1 = sum(fmeasure(flib.l0f_hc_probe_g1, (ctypes.c_int32 * 18)(*c))[0] for c in digit_sets) / len(digit_sets)
    l0f_horner, _ = fmeasure(flib.l0f_hc_probe_horner)
    n_sg = -(-4 * launch_dvs // sgb_m)
    l0f_reduce = n_sg * (sgb_k + sgb_m // 32) * g2_add
    l0f_per_launch = l0f_reduce + l0f_horner + lines_h + s_quad + final1
    sgb_bucket_t = sgb_bucket + madd
    decode_sgb_fused = decode_sgb + madd
    # Per-duty key side (round 11; bls_rlc.h rlc_duty_keys_l0f, k_rlc_g1_l0 one
    # lane per duty in launches of at least l0_duty_partials partials): P_d in
    # Straus' joint form, the 18 doublings once per duty, and the affine
    # conversion k_rlc_duty_sum<DSUM_L0_P> ran.  Probes: tests/l0straus/
    # l0straus_host.cpp built with TBG_COUNT_OPS, four distinct keys and the
    # digit sets above (7-of-10: ten candidates, keys repeating with other digits).
    slib = twin_build.lib("l0straus_count")
    slib.ls_count_get.restype = ctypes.c_ulonglong
    assert slib.ls_probe_setup(b"".join(pks), len(pks)) == 0

    def duty_probe(fn, n):
        pid = (ctypes.c_uint32 * n)(*[k % len(pks) for k in range(n)])
        c18 = (ctypes.c_int32 * (18 * n))(*[digit_sets[k % 3][(j + k // 3) % 18] for k in range(n) for j in range(18)])
        u4 = (ctypes.c_uint32 * (4 * n))()
        slib.ls_digits(c18, n, u4)
        slib.ls_count_reset()
        assert fn(pid, u4, n) == 0
        return slib.ls_count_get()

    l0s_duty4, l0s_partials4 = duty_probe(slib.ls_probe_duty, 4), duty_probe(slib.ls_probe_partials, 4)
    l0s_duty10, l0s_partials10 = duty_probe(slib.ls_probe_duty, 10), duty_probe(slib.ls_probe_partials, 10)
    l0s_to_affine = duty_sum_p4 - (l0s_partials4 - 4 * l0f_g1)  # k_rlc_duty_sum<DSUM_L0_P> less its three additions
    l0f_partial = l0f_g1  # per-partial form (launches below l0_duty_partials): its key product; P_d by k_rlc_duty_sum
    l0f_duty4 = l0s_duty4 + l0s_to_affine  # per-duty form: k_rlc_g1_l0 whole
    unit_3of4_l0_per_partial = (4 * decode_sgb_fused + hash_ + lines_h + 4 * l0f_partial + duty_sum_p4 + l0_per_group / G
                                + agg + l0f_per_launch / launch_dvs)
    unit_3of4_l0 = unit_3of4_l0_per_partial - (4 * l0f_partial + duty_sum_p4) + l0f_duty4
    # every candidate but the first of each group is randomised: (4 G - 1) / G per duty
    unit_3of4_rlc = (4 * decode + hash_ + lines_h + (4 * G - 1) / G * rlc_partial + duty_sum4 + group_lines8 / G
                     + rlc_check_per_group / G + agg)
    unit_3of4_v1 = 4 * decode + hash_ + 4 * verify + agg
    unit_3of4 = 4 * decode + hash_ + lines_h + 4 * (lines_sig + verify_quad) + agg
    model = {
        "generator": "tools/count_work.py",
        "mads_per_fp_mul": 392,
        "rlc_schedule": {"group": G, "chunk": C},
        "mads": {"decode_sig": decode, "hash_to_g2": hash_, "lines_sig": lines_sig, "lines_h": lines_h,
                 "lines_h_jacobian_steps": lines_h_jacobian, "verify_quad_item": verify_quad, "verify_item_single_lane": verify,
                 "rlc_partial": rlc_partial, "rlc_duty_sum_4": duty_sum4, "rlc_group_lines": group_lines8,
                 "rlc_miller_chunk": chunk2, "rlc_miller_chunk_folded": chunk2f, "rlc_group_final": final4,
                 "rlc_check_per_group": rlc_check_per_group,
                 "aggregate_3of4_all4": agg,
                 "l0_partial": l0_partial, "l0_duty_sum_4": duty_sum_p4, "l0_per_group": l0_per_group,
                 "l0_per_launch": round(l0_per_launch), "l0_bucket_scales": round(bucket_scales),
                 "g2_add": g2_add, "quad_mul": qmul, "l0_s_quad": s_quad, "final_exp_quad": final1,
                 "l0_chunk_base": round(chunk_base), "l0_chunk_per_duty": round(chunk_per_duty),
                 "unit_3of4_l0": round(unit_3of4_l0), "l0_launch_dvs": launch_dvs,
                 "unit_3of4_l0_bucket_msm": round(unit_3of4_l0_msm),
                 "l0f_partial": round(l0f_partial), "l0f_key_product": round(l0f_g1), "l0f_horner": l0f_horner,
                 "l0f_duty_4": round(l0f_duty4), "l0f_duty_4_per_partial_form": round(4 * l0f_partial + duty_sum_p4),
                 "l0f_duty_10_jacobian": l0s_duty10, "l0f_duty_10_jacobian_per_partial_form": l0s_partials10,
                 "l0f_duty_4_jacobian": l0s_duty4, "l0f_duty_4_jacobian_per_partial_form": l0s_partials4,
                 "unit_3of4_l0_per_partial_form": round(unit_3of4_l0_per_partial),
                 "l0_duty_partials": L0_DUTY_PARTIALS,  # unit_3of4_l0 holds from this many partials per launch
                 "l0f_per_launch": round(l0f_per_launch),
                 "unit_3of4_l0_subgroup_alone": round(unit_3of4_l0_alone),
                 "decode_sig_batched_subgroup": round(decode_sgb), "sgb_per_partial": round(sgb_per_partial),
                 "unit_3of4_rlc": round(unit_3of4_rlc), "unit_3of4_each": unit_3of4,
                 "unit_3of4_single_lane_schedule": unit_3of4_v1},
        "fp_mul_equiv": {k: round(v / 392, 1) for k, v in
                         {"decode_sig": decode, "hash_to_g2": hash_, "lines_sig": lines_sig,
                          "verify_quad_item": verify_quad, "verify_item_single_lane": verify,
                          "rlc_partial": rlc_partial, "rlc_duty_sum_4": duty_sum4,
                          "rlc_group_lines": group_lines8, "rlc_miller_chunk": chunk2,
                          "rlc_miller_chunk_folded": chunk2f, "rlc_group_final": final4,
                          "aggregate_3of4_all4": agg, "l0_partial": l0_partial, "l0_duty_sum_4": duty_sum_p4,
                          "l0_per_group": l0_per_group, "l0_per_launch": l0_per_launch,
                          "unit_3of4_l0": unit_3of4_l0, "unit_3of4_rlc": unit_3of4_rlc,
                          "decode_sig_batched_subgroup": decode_sgb,
                          "unit_3of4_each": unit_3of4, "unit_3of4_reference_schedule": unit_3of4_v1}.items()},
        "verify_hbm_bytes_per_launch": None,
        "batched_inversion": {"fp_inv": fp_inv_cost, "per_value_in_workgroups_of_256": round(binv_item, 1)},
        # u32 mul-adds per item of each kernel of the level-0 chain (bench.py
        # prices the dominant kernel of its per-kernel profile with these)
        "kernels": {
            "k_decode_sigs": {"per": "partial", "mads": round(k_decode)},
            "k_subgroup_sigs": {"per": "partial", "mads": round(k_subgroup)},
            "k_sgb_bucket": {"per": "partial", "mads": round(sgb_bucket_t)},  # (with the fused level 0's sum T)
            "k_sgb_tri_fold": {"per": "partial", "mads": round(sgb_fold)},
            "k_sgb_combine": {"per": "partial", "mads": round(sgb_combine)},
            "k_sgb_test": {"per": "partial", "mads": round(sgb_test)},
            "k_hash_map": {"per": "message", "mads": round(k_hash_map)},
            "k_hash_sswu": {"per": "message", "mads": round(k_hash_sswu)},
            "k_hash_clear_x1": {"per": "message", "mads": round(k_clear_x1)},
            "k_hash_clear_x2": {"per": "message", "mads": round(k_clear_x2)},
            "k_hash_clear_fin": {"per": "message", "mads": round(k_clear_fin)},
            "k_hash_affine": {"per": "message", "mads": round(k_g2_aff)},
            "k_lines_h": {"per": "message", "mads": round(lines_h)},
            # fused, one lane per duty (3-of-4 with four candidates): 18 doublings + 70 additions + the conversion.
            # This prices launches of at least TBG_L0_DUTY_PARTIALS partials -- bench.py's per-kernel pass
            # profiles a 16-batch launch, 640,000 partials.  A smaller launch (the driver shape's 7 + 7 + 6
            # batches, config 4, a lone batch) runs k_rlc_g1_l0_per_partial and k_rlc_duty_sum<DSUM_L0_P>:
            # price its kernel with those two entries and its unit with unit_3of4_l0_per_partial_form.
            # From TBG_L0_TAIL_PARTIALS = 131,072 partials per launch either form's grid also holds the S role
            # (bls_l0tail.h): the column sums and the Horner chain, per launch.  Smaller launches run k_l0f_* instead.
            "k_rlc_g1_l0": {"per": "duty", "mads": round(l0f_duty4), "from_partials_per_launch": L0_DUTY_PARTIALS,
                            "plus_per_launch": round(l0f_reduce) + l0f_horner},
            "k_rlc_g1_l0_per_partial": {"per": "partial", "mads": round(l0f_g1),
                                        "below_partials_per_launch": L0_DUTY_PARTIALS,
                                        "plus_per_launch": round(l0f_reduce) + l0f_horner},
            "k_l0f_reduce": {"per": "launch", "mads": round(l0f_reduce), "below_partials_per_launch": 131072},
            "k_l0f_horner": {"per": "launch", "mads": l0f_horner, "below_partials_per_launch": 131072},
            # without the batched subgroup test: the bucket MSM (k_rlc_g1_l0 then costs k_rlc_g1_l0_msm)
            "k_rlc_g1_l0_msm": {"per": "partial", "mads": round(k_g1_l0)},
            "k_msm_bucket_part": {"per": "partial", "mads": round(4 * k_msm_entry)},
            "k_msm_bucket": {"per": "launch", "mads": round(bucket_scales + 32768 * (4 - 1) * g2_add)},
            "k_rlc_duty_sum<DSUM_L0_P>": {"per": "duty", "mads": round(duty_sum_p4)},
            # the level-0 P-chunk products on hexads (bls_hex.h) + the one S hexad
            "k_miller_hex<MILLER_L0>": {"per": "chunk", "mads": round(chunk_base), "plus": {"duty": round(chunk_per_duty)},
                                        "plus_per_launch": s_quad},
            "k_l0_fold": {"per": "chunk", "mads": round(qmul), "plus": {"group": -round(qmul)}},
            "k_l0_final": {"per": "launch", "mads": round(final1)},
            "k_aggregate<true>": {"per": "duty", "mads": round(agg)},
            "k_aggregate<false>": {"per": "duty", "mads": round(agg)},
        },
    }
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "work_model.json"), "w") as f:
        json.dump(model, f, indent=1)
    print(json.dumps(model, indent=1))


if __name__ == "__main__":
    main()
