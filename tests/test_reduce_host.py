"""Host-side checks of tests/_reduce_cases.py: the cases and references of the reduction / row-exchange parity suite
(tests/test_reduce_gpu.py) must themselves stay inside the rules they hold the kernels to.  No GPU needed."""

import os
import re

import numpy as np
import pytest

import _reduce_cases as rc


def _sum_problems(kind):
    """(name, Ar, Br, goff, terms per output, prior or None) of every sum-reduction case of the suite, in `kind` inputs."""
    for da, db in rc.OUTER_DIMS:
        for mode in rc.OUTER_MODES:
            Ar, Br = rc.outer_rows(rc.outer_inputs(da, db, mode, kind))
            yield f"group_outer {da}x{db} {mode}", Ar, Br, rc.GOFF, None, None
        Ar, Br = rc.outer_rows(rc.outer_inputs(da, db, "identity", kind))
        yield f"group_outer {da}x{db} accumulate", Ar, Br, rc.GOFF, None, rc.outer_prior(da, db, kind)
    for K in rc.MATMUL_K:
        for M, N in rc.MATMUL_MN:
            A, B = rc.matmul_inputs(K, M, N, kind)
            yield f"matmul K={K} {M}x{N}", A, B, np.array([0, K]), K + rc.matmul_slices(K, M, N), None
    for d in rc.SEG_D:
        for clamp in (False, True):
            Ar, Br, off = rc.seg_rows(rc.seg_inputs(d, rc.SEG_LENGTHS, kind, clamp=clamp))
            yield f"segment_axpy d={d} clamp={clamp}", Ar, Br, off, None, None
    for nseg in rc.SEG_NSEG:
        for d in rc.SEG_NSEG_D:
            Ar, Br, off = rc.seg_rows(rc.seg_inputs(d, rc.seg_lengths(nseg), kind))
            yield f"segment_axpy d={d} nseg={nseg}", Ar, Br, off, None, None
    for N in rc.COLSUM_N:
        for d in rc.COLSUM_D:
            if N > 513 and d > rc.COLSUM_BIG_D:
                continue
            inp = rc.colsum_inputs(N, d, kind)
            for masked in (False, True):
                Ar, Br, off = rc.colsum_rows(inp, masked)
                yield f"colsum N={N} d={d} masked={masked}", Ar, Br, off, None, inp["prior"][None, None, :]
    for n in rc.DOT_N:
        yield (f"dot n={n}", *rc.dot_rows(*rc.dot_inputs(n, kind)), None, None)


def test_derived_cases_have_the_shapes_they_are_named_for():
    cases = {name: (len(keys), R) for name, keys, R in rc.group_edges_cases()}
    assert cases["E=1 R=1"] == (1, 1) and cases["R+1 > E"] == (50, 100003) and cases["E=70000 R=5"] == (70000, 5)
    assert all(cases[f"E=300 R={R}"] == (300, R) for R in (2, 3, 256, 257))
    for nseg in rc.SEG_NSEG:
        lengths = rc.seg_lengths(nseg)
        assert len(lengths) == nseg and min(lengths) >= 0
    assert rc.seg_lengths(9) == rc.SEG_LENGTHS and 0 in rc.seg_lengths(4097) and rc.seg_lengths(4097).count(1000) == 1
    assert rc.seg_lengths(4097)[0] == 0 and rc.seg_lengths(9)[-1] == 0          # empty leading and trailing segments


def test_exact_integer_cases_stay_below_two_to_the_24():
    """Every partial sum of an exact-integer case, in any order, is bounded by sum |terms| (+ |prior|): below 2^24, so it is
    exact in fp32 — asserted from each case's own inputs."""
    count = 0
    for name, Ar, Br, goff, _, prior in _sum_problems("int"):
        assert Ar.dtype == np.float32 and Br.dtype == np.float32
        assert np.abs(Ar).max(initial=0) <= 3 and np.abs(Br).max(initial=0) <= 3, name
        assert rc.magnitude_ok(Ar, Br, goff, prior), f"{name}: sum |terms| reaches 2^24"
        count += 1
    assert count > 100
    A, _ = rc.matmul_inputs(40000, 17, 129, "int")
    assert set(np.unique(A)) == {-1.0, 0.0, 1.0}                              # the integers shrink at K = 40000
    w = rc.seg_inputs(7, rc.SEG_LENGTHS, "int")["w"]
    assert np.abs(w).max() <= 2


def test_references_hold_a_scrambled_float32_evaluation_to_their_own_rules():
    """A plain numpy float32 evaluation in a scrambled order: equal to the int64 sums in exact-integer mode, inside the derived
    bound in rounding mode (so neither check rejects a correct kernel for the order it sums in)."""
    worst, rows = 0.0, 0
    for seed, (name, Ar, Br, goff, _, _) in enumerate(_sum_problems("int")):
        got = rc.scrambled_f32(Ar, Br, goff, seed)
        assert np.array_equal(got.astype(np.int64), rc.exact_sums(Ar, Br, goff)) and (got == np.rint(got)).all(), name
        rows += got.size
    for seed, (name, Ar, Br, goff, n, _) in enumerate(_sum_problems("normal")):
        ref, mag, terms = rc.float_sums(Ar, Br, goff)
        b = rc.bound(mag, terms if n is None else n)
        err = np.abs(rc.scrambled_f32(Ar, Br, goff, seed).astype(np.float64) - ref)
        assert (err <= b).all(), f"{name}: a float32 evaluation misses the bound by {np.max(err - b):.3e}"
        worst = max(worst, float(np.max(err / np.where(b > 0, b, 1.0))))
    assert rows > 5000 and 0.0 < worst < 1.0
    print(f"worst err / bound of a scrambled float32 evaluation: {worst:.3f}")


def test_bound_counts_the_accumulated_prior_and_empty_groups_are_zero():
    Ar, Br = rc.outer_rows(rc.outer_inputs(17, 129, "gather", "normal"))
    ref, mag, n = rc.float_sums(Ar, Br, rc.GOFF)
    assert (ref[0] == 0).all() and (ref[-1] == 0).all() and (mag[0] == 0).all()          # the two empty groups
    assert (rc.bound(mag, n)[0] == 0).all()                                               # ... must come out as exact zeros
    prior = rc.outer_prior(17, 129, "normal")
    assert (rc.bound(mag, n, accumulated=ref + prior) > rc.bound(mag, n))[1:-1].all()
    assert rc.matmul_slices(512, 17, 129) == 1 and rc.matmul_slices(513, 17, 129) > 1 and rc.matmul_slices(40000, 3, 5) > 100


def test_group_reference_is_a_stable_grouping():
    for name, keys, R in rc.group_edges_cases():
        perm, goff = rc.group_reference(keys, R)
        assert keys.min() >= 0 and keys.max() < R, name
        assert np.array_equal(np.sort(perm), np.arange(len(keys))), name
        assert np.array_equal(np.diff(goff), np.bincount(keys, minlength=R)), name
        for r in np.unique(keys)[:50]:
            assert np.array_equal(perm[goff[r]:goff[r + 1]], np.nonzero(keys == r)[0]), name   # stable: ascending ids per key
    names = [c[0] for c in rc.group_edges_cases()]
    keys = dict((c[0], c[1]) for c in rc.group_edges_cases())
    assert len(set(names)) == len(names) == 10
    assert (np.diff(keys["descending, duplicates"]) <= 0).all() and len(np.unique(keys["descending, duplicates"])) == 7
    assert set(np.unique(keys["relations 0, 3, 6 absent"])) == {1, 2, 4, 5}
    assert len(np.unique(keys["all equal"])) == 1


def test_out_of_range_grouping_check_accepts_a_clamped_sort_and_can_fail():
    keys, R = rc.out_of_range_keys()
    assert (keys == -1).any() and (keys == R).any() and (keys == 1 << 40).any() and ((keys >= 0) & (keys < R)).sum() > 200
    clamped = np.where((keys >= 0) & (keys < R), keys, R - 1)
    perm, goff = rc.group_reference(clamped, R)
    rc.check_out_of_range_grouping(keys, R, perm, goff)
    with pytest.raises(AssertionError):
        rc.check_out_of_range_grouping(keys, R, perm[::-1].copy(), goff)
    with pytest.raises(AssertionError):
        rc.check_out_of_range_grouping(keys, R, np.zeros_like(perm), goff)
    with pytest.raises(AssertionError):
        rc.check_out_of_range_grouping(keys, R, perm, np.concatenate([goff[:-1], [len(keys) - 1]]))


def test_segment_probes_tell_the_ascending_fold_from_other_orders():
    assert tuple(rc.fold_f32(p) for p in rc.SEG_PROBES) == rc.SEG_PROBE_SUMS == (0.0, 0.0, 1.0)
    first = rc.SEG_PROBES[0]
    assert rc.fold_f32(first, "ends") == 2.0 and rc.fold_f32(first, "neighbours") == 1.0
    for order in ("descending", "ends", "neighbours", "stride2", "swapped pairs"):
        sums = tuple(rc.fold_f32(p, order) for p in rc.SEG_PROBES)
        assert sums != rc.SEG_PROBE_SUMS, f"the probes cannot tell a {order} fold from the ascending one"
    for d in (1, 130):
        inp = rc.probe_inputs(d)
        want = np.repeat(np.asarray(rc.SEG_PROBE_SUMS, dtype=np.float32)[:, None], d, axis=1)
        assert np.array_equal(rc.seg_fold(inp), want)


def test_segment_fold_is_exact_on_integers_and_inside_the_bound_on_power_of_two_weights():
    for d in (7, 260):
        inp = rc.seg_inputs(d, rc.SEG_LENGTHS, "int", clamp=True)
        assert np.array_equal(rc.seg_fold(inp).astype(np.int64), rc.exact_sums(*rc.seg_rows(inp))[:, 0, :])
        inp = rc.seg_inputs(d, rc.SEG_LENGTHS, "pow2")
        mant, _ = np.frexp(inp["w"])
        assert (np.abs(mant) == 0.5).all() and np.abs(inp["w"]).min() >= 0.125 and np.abs(inp["w"]).max() <= 8.0
        assert (inp["w"] < 0).any() and (inp["w"] > 0).any()
        ref, mag, n = rc.float_sums(*rc.seg_rows(inp))
        fold = rc.seg_fold(inp)
        assert (np.abs(fold - ref[:, 0, :]) <= rc.bound(mag, n)[:, 0, :]).all()
        assert (fold[0] == 0).all() and (fold[-1] == 0).all()                             # empty segments: zeros
        assert inp["iw"].max() < rc.SEG_NW and not np.array_equal(inp["iw"], inp["ix"])
        assert len(np.unique(inp["ix"])) < len(inp["ix"])                                 # repeated rows
    bad = rc.seg_inputs(7, rc.SEG_LENGTHS, "normal", clamp=True)
    assert (bad["ix"] == -5).any() and (bad["ix"] == rc.SEG_NX + 5).any() and bad["iw"].min() >= 0 and bad["iw"].max() < rc.SEG_NW


def test_group_outer_inputs_and_permutation():
    for da, db in ((0, 130), (17, 129)):
        for mode in rc.OUTER_MODES:
            inp = rc.outer_inputs(da, db, mode, "int")
            assert (inp["A"] is None) == (da == 0) and (inp["ib"] is not None) == (mode == "gather")
            for tab, idx in (("A", "ia"), ("B", "ib")):
                if inp[idx] is not None:                                                   # in range, with repeated rows
                    assert 0 <= inp[idx].min() and inp[idx].max() < inp[tab].shape[0] < len(inp[idx])
            want = rc.exact_sums(*rc.outer_rows(inp), rc.GOFF)
            assert want.shape == (len(rc.GROUP_SIZES), max(da, 1), db)
            order = np.random.default_rng(da + db).permutation(len(rc.GROUP_SIZES))
            pin, pgoff = rc.outer_permuted(inp, order)
            assert np.array_equal(rc.exact_sums(*rc.outer_rows(pin), pgoff), want[order])
    inp = rc.outer_inputs(0, 1, "identity", "int")
    assert np.array_equal(rc.exact_sums(*rc.outer_rows(inp), rc.GOFF)[:, 0, 0],
                          [int(inp["B"][s:e].sum()) for s, e in zip(rc.GOFF[:-1], rc.GOFF[1:])])


def test_row_exchange_references():
    rows, extra = rc.rows_tables(37, 16, 4, "host")
    assert rows.dtype == np.uint8 and rows.shape == (37, 16) and extra.shape == (37, 4)
    big = rc.random_bytes(1, "nan", (4096, 4)).view(np.float32)
    assert np.isnan(big).any()                                                            # NaN bit patterns do occur
    idx = rc.pack_indices(5, 37, "host", bad=True)
    assert (idx == -1).any() and (idx == 37).any()
    before = np.full((5, 20), rc.SENTINEL, dtype=np.uint8)
    msg = rc.pack_reference(rows, extra, idx, before)
    for i, r in enumerate(idx):
        want = np.concatenate([rows[r], extra[r]]) if 0 <= r < 37 else before[i]
        assert np.array_equal(msg[i], want)
    assert rc.pack_indices(4, 37, "rep")[0] == rc.pack_indices(4, 37, "rep")[1]           # repeated indices
    perm = rc.unpack_indices(37, 37, "host")
    assert np.array_equal(np.sort(perm), np.arange(37))
    packed = rc.pack_reference(rows, extra, perm, np.zeros((37, 20), dtype=np.uint8))
    blank = np.full_like(rows, rc.SENTINEL), np.full_like(extra, rc.SENTINEL)
    r2, x2 = rc.unpack_reference(*blank, perm, packed)
    assert np.array_equal(r2, rows) and np.array_equal(x2, extra)                         # unpack after pack restores
    part = rc.unpack_indices(5, 37, "host", bad=True)
    r3, x3 = rc.unpack_reference(*blank, part, packed[:5])
    listed = part[(part >= 0) & (part < 37)]
    others = np.setdiff1d(np.arange(37), listed)
    assert (r3[others] == rc.SENTINEL).all() and (x3[others] == rc.SENTINEL).all() and len(np.unique(listed)) == len(listed)


def test_score_case_has_a_hub_and_self_pairs():
    for d in rc.SCORE_D:
        embs, src, dst, w = rc.score_pairs_case(d)
        assert embs.shape == (rc.SCORE_N, d) and len(src) == len(dst) == len(w) == rc.SCORE_P
        assert int(((src == 7) | (dst == 7)).sum()) == rc.SCORE_HUB
        assert int((src == dst).sum()) >= 50 and src.max() < rc.SCORE_N and dst.min() >= 0


def test_gpu_suite_skips_nothing():
    """No case is skipped or expected to fail; the only conditional inside a test is the size guard on the large colsum shape."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_reduce_gpu.py")) as f:
        text = f.read()
    assert not re.search(r"pytest\.skip|mark\.skip|\bskipif\b|\bxfail\b|\bimportorskip\b", text)
    assert re.search(r"^pytestmark = pytest\.mark\.gpu$", text, re.M)
