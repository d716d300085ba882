"""Host-side checks of tests/_edge_outer_cases.py: the cases, references and bounds of the weight-gradient contraction's parity
suite (tests/test_edge_outer_gpu.py) must themselves satisfy the conditions they rest on — and the two host routines that
build ghf_edge_outer's work lists (autograd._slice_tables, autograd._ident_slices) must keep the ABI's rules.  No GPU needed."""

import numpy as np
import pytest

import _edge_outer_cases as ec
import _reduce_cases as rc
from graph_hypernetwork_forge_amd import autograd, synth


def test_the_table_holds_the_lengths_and_empty_relations_it_is_named_for():
    g = ec.graph("crafted")
    assert (g["N"], g["R"]) == (150, 7)
    assert np.diff(g["goff"]).tolist() == [0, 1, 961, 0, 4096, 193, 0]
    lengths = lambda r: (g["slice_tab"][g["slice_off"][r]:g["slice_off"][r + 1], 2]                      # noqa: E731
                         - g["slice_tab"][g["slice_off"][r]:g["slice_off"][r + 1], 1]).tolist()
    assert lengths(1) == [1] and lengths(4) == [4096] and lengths(5) == [192, 1]
    assert lengths(2) == [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129]
    assert max(np.diff(ec.graph("short")["goff"])) == 129 and np.diff(ec.graph("short")["goff"])[[0, 3 + 3]].tolist() == [0, 0]
    for name in ec.CUTS:
        g = ec.graph(name)
        ec.check_slice_rules(g["slice_tab"], g["slice_off"], g["goff"])
        assert g["src"].min() >= 0 and g["dst"].min() >= 0 and max(g["src"].max(), g["dst"].max()) < g["N"]
    assert len(ec.WALK_CUTS) == 5 and sum(len(c) for c in ec.WALK_CUTS) == ec.WALK_SLICES > 256
    assert all(32 <= n <= 64 for c in ec.WALK_CUTS for n in c) and len({n for c in ec.WALK_CUTS for n in c}) > 20


def test_the_edges_hold_the_shapes_they_are_named_for():
    g = ec.graph("crafted")
    src, dst, goff = g["src"], g["dst"], g["goff"]
    pairs = list(zip(src.tolist(), dst.tolist()))
    for r in (2, 4, 5):
        a, b = int(goff[r]), int(goff[r + 1])
        assert (src[a:b] == dst[a:b]).any(), f"relation {r} has no self-loop"
        assert any(pairs[e] == pairs[e - 1] for e in range(a + 1, b)), f"relation {r} has no duplicated edge"
        assert (src[a:b] == g["N"] - 1).any(), f"relation {r} never reads the last row as a source"
    a, b = int(goff[2]), int(goff[3])
    assert 4 * int((dst[a:b] == ec.HUB).sum()) >= b - a, "the hub holds less than a quarter of relation 2"
    last = int(g["slice_tab"][int(g["slice_off"][2]) + 3][2]) - 1
    assert g["slice_tab"][int(g["slice_off"][2]) + 3][2] - g["slice_tab"][int(g["slice_off"][2]) + 3][1] == 33
    assert (src[last], dst[last]) == (ec.LONE_SRC, ec.LONE_DST)
    ends = np.concatenate([src, dst])
    assert (ends == ec.LONE_SRC).sum() == 1 and (ends == ec.LONE_DST).sum() == 1, "the lone rows are read elsewhere too"
    assert len(np.unique(ends)) == g["N"], "a row no edge reads"


@pytest.mark.parametrize("d", ec.WIDTHS)
def test_exact_integer_cases_are_exact_on_both_chains(d):
    """sum |terms| < 2^24 for dW and db (any order is exact in fp32), and the two-piece cut of the integers has lo = 0."""
    g = ec.graph("crafted")
    h, G = ec.inputs("int", d)
    Ar, Br = ec.rows(g, h, G)
    assert rc.magnitude_ok(Ar, Br, g["goff"]) and rc.magnitude_ok(ec.ones(g), Br, g["goff"])
    assert np.abs(h).max() == 3 and np.abs(G).max() == 3
    if d <= 128:
        assert np.array_equal(ec.int_sums(Ar, Br, g["goff"]), rc.exact_sums(Ar, Br, g["goff"]))
    for x in (h, G):
        xs, hi, lo = ec.cut(x, ec.shift(x))
        assert (hi == xs).all() and (lo == 0).all() and np.abs(xs).max() == 3 * 2.0 ** 12


@pytest.mark.parametrize("kind", ("grid_h", "grid_g"))
@pytest.mark.parametrize("d", ec.PIECE_WIDTHS)
def test_grid_cases_are_exact_and_need_their_lo_pieces(d, kind):
    g = ec.graph("crafted")
    h, G = ec.inputs(kind, d)
    ok = ec.grid_ok(g, h, G)
    print(f"grid {kind} d={d}: lo != 0 in {ok['lo_share']:.3f} of the fine entries, sum|pieces||b| = 2^{np.log2(ok['units']):.2f} units")
    assert ok["reproduced"], "hi + lo does not reproduce every scaled entry"
    assert ok["lo_share"] > 0.75, "most fine entries should need their lo piece"
    assert ok["units"] < rc.LIMIT, "a partial sum may leave the exact range"
    assert ok["db_exact"][[0, 1, 3, 5, 6]].all() and (kind == "grid_g" or ok["db_exact"].all())
    fine = h if kind == "grid_h" else G
    k = fine.astype(np.float64) * 2.0 ** ec.FINE_BITS
    assert (k == np.rint(k)).all() and np.abs(k).max() == 2 ** ec.FINE_BITS - 1 > 2 ** 11, "not the fine grid"
    tern = G if kind == "grid_h" else h
    assert set(np.unique(tern).tolist()) == {-1.0, 0.0, 1.0}
    a, b = int(g["goff"][4]), int(g["goff"][5])
    Ar, Br = ec.rows(g, h, G)
    assert ((Ar[a:b] != 0).astype(np.float64).T @ (Br[a:b] != 0).astype(np.float64)).max() >= 64, "the long relation's outputs sum few terms"


@pytest.mark.parametrize("kind,lost", (("grid_h", "lh"), ("grid_g", "hl")))
@pytest.mark.parametrize("d", (128, 384))
def test_the_emulated_chain_is_exact_on_the_grid_cases_and_a_lost_piece_is_not(d, kind, lost):
    g = ec.graph("crafted")
    h, G = ec.inputs(kind, d)
    ref = ec.float_reference(kind, d, "crafted")
    dW, db = ec.emulate_pieces(g, h, G)
    keep = ec.grid_ok(g, h, G)["db_exact"]
    assert np.array_equal(dW.astype(np.float64), ref["dW"]) and np.array_equal(db.astype(np.float64)[keep], ref["db"][keep])
    broken, _ = ec.emulate_pieces(g, h, G, drop=lost)
    moved = np.abs(broken.astype(np.float64) - ref["dW"]).max(axis=(1, 2))
    print(f"grid {kind} d={d}: without the {lost} product the relations move by {moved}")
    assert (moved[[1, 2, 4, 5]] > 0).all(), "a lost cross product would go unseen in some relation"


@pytest.mark.parametrize("name", tuple(ec.CUTS))
@pytest.mark.parametrize("d", ec.PIECE_WIDTHS)
def test_the_emulated_pieces_chain_meets_the_derived_bound(d, name):
    g = ec.graph(name)
    h, G = ec.inputs("normal", d, name)
    ref = ec.float_reference("normal", d, name)
    dW, db = ec.emulate_pieces(g, h, G)
    b = ec.pieces_bound(g, ref, ec.shift(h), ec.shift(G))
    err = np.abs(dW.astype(np.float64) - ref["dW"])
    print(f"err/bound emulated pieces chain d={d} {name}: {float(np.max(err / np.where(b > 0, b, 1.0))):.4f}")
    assert (err <= b).all()
    _, bb = ec.exact_bounds(g, ref)
    assert (np.abs(db.astype(np.float64) - ref["db"]) <= bb).all()
    empty = np.diff(g["goff"]) == 0
    assert (b[empty] == 0).all() and (dW[empty] == 0).all() and (bb[empty] == 0).all()


def test_a_lost_piece_hides_under_the_bound_in_the_long_relation_only():
    """Why the rounding check has a second table: at 4,096 edges the derived bound is wider than what one lost product costs; at
    129 edges and fewer it is not (so the short table's rounding check sees a chain that drops a product)."""
    d = 128
    for name, seen in (("crafted", False), ("short", True)):
        g = ec.graph(name)
        h, G = ec.inputs("normal", d, name)
        ref = ec.float_reference("normal", d, name)
        b = ec.pieces_bound(g, ref, ec.shift(h), ec.shift(G))
        dW, _ = ec.emulate_pieces(g, h, G, drop="lh")
        over = (np.abs(dW.astype(np.float64) - ref["dW"]) > b).any(axis=(1, 2))
        r = int(np.argmax(np.diff(g["goff"])))
        assert bool(over[r]) == seen, f"{name}: relation {r} of {np.diff(g['goff'])[r]} edges"


@pytest.mark.parametrize("d", ec.BITS_WIDTHS)
def test_rescaled_inputs_stay_normal(d):
    """h 2^a, G 2^b: every input, every product and the last bit of every product is a normal fp32 number, so the power of two
    passes through both chains exactly."""
    h, G = ec.inputs("clamped", d)
    assert np.abs(h).min() >= 2.0 ** -6 and np.abs(G).min() >= 2.0 ** -6
    tiny = float(np.finfo(np.float32).tiny)
    for a, b in ec.RESCALES:
        ha, Gb = np.ldexp(h, a), np.ldexp(G, b)
        assert ha.dtype == np.float32 and (np.ldexp(ha.astype(np.float64), -a) == h).all() and (np.ldexp(Gb.astype(np.float64), -b) == G).all()
        assert float(np.abs(ha).min()) * float(np.abs(Gb).min()) * 2.0 ** -24 > tiny
        assert float(np.abs(ha).max()) * float(np.abs(Gb).max()) * 2.0 ** 13 < 2.0 ** 100
        assert abs(ec.shift(ha)) < 100 and abs(ec.shift(Gb)) < 100 and ec.shift(ha) == ec.shift(h) - a


def test_top_entries_are_a_power_of_two_and_one_ulp_below():
    h, _ = ec.inputs("normal", 128)
    for value in (np.float32(8.0), np.nextafter(np.float32(8.0), np.float32(0.0))):
        x = ec.top_entry(h, value)
        assert np.abs(x).max() == value and ec.shift(x) == (10 if value == 8.0 else 11)


@pytest.mark.parametrize("name", tuple(ec.GUARD_CASES))
def test_guard_cases_count_what_they_are_named_for(name):
    groups = ec.GUARD_CASES[name]
    for d in (128, 256):
        X = ec.rows_with_maxima(groups, d, name)
        m = np.abs(X).max(axis=1)
        want = sorted(float(np.ldexp(mant, ex or 0)) for k, ex, mant in groups for _ in range(k))
        assert sorted(m.tolist()) == [np.float32(w) for w in want], "a row's largest magnitude is not its group's"
        far, nz = ec.guard_counts(X)
        assert nz == 64 and (m == 0).sum() == 16 and far == (56 if ec.GUARD_TRIPS[name] else 55)
        assert (8 * far >= 7 * nz) == ec.GUARD_TRIPS[name]
        assert (8 * far >= 7 * (nz + 16)) is False, "zero rows counted as nonzero would not change this case"
        for side in ("h", "G"):
            h, G = ec.guard_inputs(groups, side, d, name)
            assert ec.guard_trips(h, G) == ec.GUARD_TRIPS[name]
            assert ec.guard_counts(G if side == "h" else h) == (0, 80)
    X = ec.rows_with_maxima(ec.GUARD_CASES["a row 14 exponents down does not count"], 128, "x")
    m = np.sort(np.abs(X).max(axis=1))
    assert m[-1] / m[16 + 55] > 2.0 ** 14.9, "the uncounted row is nearly 2^-15 of the largest: only the exponents say 14"
    X = ec.rows_with_maxima(ec.GUARD_CASES["a row 15 exponents down counts"], 128, "x")
    m = np.sort(np.abs(X).max(axis=1))
    assert m[-1] / m[16 + 55] < 2.0 ** 14.1


def test_the_large_guard_case_needs_the_grid_stride_loop():
    X = ec.rows_with_maxima(ec.GUARD_BIG, 128, "big")
    assert X.shape == (ec.GUARD_BIG_N, 128) and ec.GUARD_BIG_N > 3 * 40 * 256        # 40 workgroups of 256 rows, four trips
    assert ec.guard_counts(X) == (33001, 36000) and 8 * 33001 >= 7 * 36000
    zero = np.nonzero(np.abs(X).max(axis=1) == 0)[0]
    assert len(zero) == 4000 and len(set((zero // 256).tolist())) > 100, "the zero rows should be spread over the workgroups"


def test_rows_beyond_four_gib_wrap_onto_other_touched_rows():
    c = ec.big_rows_case()
    ids, g = c["ids"], c["g"]
    assert ec.BIG_N * 128 * 4 >= 1 << 32 and ids.max() < ec.BIG_N and len(set(ids.tolist())) == 128
    assert 2 * int((ids >= 1 << 23).sum()) >= len(ids)
    wrapped = (ids * 128 * 4) % (1 << 32) // (128 * 4)
    hit = np.searchsorted(ids, wrapped)
    assert (ids[hit] == wrapped).all(), "a wrapped offset lands on an untouched row"
    far = ids >= 1 << 23
    assert (c["h"][hit[far]] != c["h"][far]).any(axis=1).all() and (c["G"][hit[far]] != c["G"][far]).any(axis=1).all()
    used = np.unique(np.concatenate([g["src"], g["dst"]]))
    assert 2 * int((ids[used] >= 1 << 23).sum()) >= len(used) - 8 and len(used) > 120
    Ar, Br = ec.rows(g, c["h"], c["G"])
    assert rc.magnitude_ok(Ar, Br, g["goff"])
    ec.check_slice_rules(g["slice_tab"], g["slice_off"], g["goff"])


# ---- the host routines that build the work lists ------------------------------------------------------------------------
def test_train_plan_slices_keep_the_rules(monkeypatch):
    """build_train_plan's table for a 1,000-edge graph with SLICE_EDGES patched to 96: remainders of every length class."""
    monkeypatch.setattr(autograd, "SLICE_EDGES", 96)
    R = 9
    rel = np.sort(synth.randint(91, "eo_plan_rel", 1000, R - 2) + 1)         # relations 0 and R - 1 stay empty
    goff = np.searchsorted(rel, np.arange(R + 1)).tolist()
    tab, soff, order = autograd._slice_tables(goff, R)
    ec.check_slice_rules(tab, soff, goff, order)
    lengths = [b - a for _, a, b in tab]
    assert max(lengths) == 96 and len([n for n in lengths if n != 96]) >= R - 3 and len(tab) > R
    assert autograd._slice_tables([0] * (R + 1), R) == ([], [0] * (R + 1), [])
    one = autograd._slice_tables([0, 0, 96, 96 + 97], 3)
    assert one[0] == [(1, 0, 96), (2, 96, 192), (2, 192, 193)] and one[1] == [0, 0, 1, 3]


@pytest.mark.parametrize("N", (1, 255, 256, 257, 65536 + 1, 100003, 4096 * 1024 + 5))
def test_input_projection_slices_keep_the_rules(N):
    tab = autograd._ident_slices(N)
    ec.check_slice_rules(tab, [0, len(tab)], [0, N])
    step = tab[0][2] - tab[0][1]
    assert step <= autograd.SLICE_EDGES and (N <= step or step % ec.TILE == 0)
    assert N % step == 0 or tab[-1][2] - tab[-1][1] == N % step
