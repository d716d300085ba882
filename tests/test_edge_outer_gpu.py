"""Exact parity suite of the weight-gradient contraction, called directly through _native.edge_outer: ghf_edge_outer and
ghf_edge_outer_scaled (csrc/backward.hip) — the exact fp32 chain (edge_outer_kernel, edge_outer_guarded_kernel), the two-piece
chain (edge_outer_h_kernel, with and without 32-bit byte offsets), the range guard's counters and the slice reduction.

Cases, edge tables, references and bounds live in tests/_edge_outer_cases.py (checked on the CPU by
tests/test_edge_outer_host.py; the bounds are derived in its docstring).  No check here has a tuned tolerance:
  exact-integer  bit-equal to int64 sums, at every width on both chains;
  grid-exact     inputs whose two-piece products are exact: bit-equal to the float64 sums and to the exact chain;
  rounding       synth.normal against float64 under the derived bounds, on the crafted table and on one of short relations; the
                 worst err / bound of every check is printed ("err/bound <kernel> ...", run with -s);
  bits           relabelled relations, pre-gathered rows, inputs rescaled by powers of two, the scaled entry point;
  range guard    the four counters of the workspace against numpy counts, and the bits of the chain the counters choose;
  rows beyond 4 GiB of h and G (the instance without 32-bit byte offsets)."""

import numpy as np
import pytest
import torch

import _edge_outer_cases as ec
import _reduce_cases as rc
from graph_hypernetwork_forge_amd import _native, autograd, synth
from graph_hypernetwork_forge_amd.plan import build_plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_TABLES = {}


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(g, h, G, **kw):
    """(dW, db) of _native.edge_outer on the tables of g (kept on the device once per table)."""
    key = id(g["slice_tab"]), id(g["src"])
    if key not in _TABLES:
        _TABLES[key] = (g, tuple(dev(g[k]) for k in ("src", "dst", "slice_tab", "slice_off")))
    return _native.edge_outer(dev(h), dev(G), *_TABLES[key][1], g["R"], **kw)


def scales(x):
    """The row scales of x's split form (what ghf_edge_outer_scaled reads)."""
    x = dev(x)
    return _native.split_row_scales(_native.split_rows(x, _native.WLAYOUT_SPLIT2H), x.size(0), x.size(1))


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def check_exact(got, want, what):
    want32 = torch.from_numpy(np.asarray(want).astype(np.float32)).reshape(got.shape)
    assert (want32.double().numpy() == np.asarray(want).reshape(got.shape)).all(), f"{what}: the reference is no fp32 number"
    assert torch.equal(got.cpu(), want32), f"{what}: {int((got.cpu() != want32).sum())} of {want32.numel()} sums differ from the exact sums"


def check_bound(kernel, what, got, ref, b):
    g = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    assert np.isfinite(g).all(), f"{kernel} {what}: non-finite values"
    err = np.abs(g - ref)
    print(f"err/bound {kernel} {what}: {float(np.max(err / np.where(b > 0, b, 1.0))):.4f}")
    worst = np.unravel_index(int(np.argmax(err - b)), err.shape)
    assert (err <= b).all(), f"{kernel} {what}: err {err[worst]:.3e} > bound {b[worst]:.3e} at {worst}"


def chain_name(d, exact):
    return "edge_outer fp32" if exact or d == 64 else "edge_outer pieces"


# ---- exact cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", ec.WIDTHS)
def test_exact_integers_on_both_chains(d):
    g = ec.graph("crafted")
    h, G = ec.inputs("int", d)
    Ar, Br = ec.rows(g, h, G)
    want, want_b = ec.int_sums(Ar, Br, g["goff"]), ec.int_sums(ec.ones(g), Br, g["goff"])
    for exact in (False, True):
        dW, db = run(g, h, G, exact=exact)
        assert dW.shape == (g["R"], 2 * d, d) and db.shape == (g["R"], d)
        check_exact(dW, want, f"{chain_name(d, exact)} d={d} dW")
        check_exact(db, want_b, f"{chain_name(d, exact)} d={d} db")


@pytest.mark.parametrize("kind", ("grid_h", "grid_g"))
@pytest.mark.parametrize("d", ec.PIECE_WIDTHS)
def test_grid_exact_cases_need_every_piece_product(d, kind):
    """One tensor on a 15-bit grid, the other in {-1, 0, 1} (tests/test_edge_outer_host.py asserts the exactness condition from
    these inputs): the two-piece chain is exact, so it equals the float64 sums and the fp32 chain bit for bit.  db is summed
    from G itself: bit-equal where sum |G| allows it, under the fp32 bound in the relations where it does not."""
    g = ec.graph("crafted")
    h, G = ec.inputs(kind, d)
    ref = ec.float_reference(kind, d, "crafted")
    got, fp32 = run(g, h, G), run(g, h, G, exact=True)
    check_exact(got[0], ref["dW"], f"edge_outer pieces {kind} d={d} dW")
    check_exact(fp32[0], ref["dW"], f"edge_outer fp32 {kind} d={d} dW")
    keep = ec.db_exact(g, G)
    assert keep[[0, 1, 3, 5, 6]].all()
    for out in (got[1], fp32[1]):
        check_exact(out[dev(np.nonzero(keep)[0])], ref["db"][keep], f"edge_outer {kind} d={d} db")
        assert (np.abs(out.cpu().numpy().astype(np.float64) - ref["db"]) <= ec.exact_bounds(g, ref)[1]).all()


# ---- rounding ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(ec.CUTS))
@pytest.mark.parametrize("d", ec.WIDTHS)
def test_rounding_stays_under_the_derived_bounds(d, name):
    g = ec.graph(name)
    h, G = ec.inputs("normal", d, name)
    ref = ec.float_reference("normal", d, name)
    bW, bb = ec.exact_bounds(g, ref)
    for exact in (False, True):
        dW, db = run(g, h, G, exact=exact)
        pieces = not exact and d != 64
        check_bound(chain_name(d, exact), f"d={d} {name} dW", dW, ref["dW"], ec.pieces_bound(g, ref, ec.shift(h), ec.shift(G)) if pieces else bW)
        check_bound(chain_name(d, exact), f"d={d} {name} db", db, ref["db"], bb)
        assert same(run(g, h, G, exact=exact), (dW, db)), "two calls, two results"
        empty = dev(np.nonzero(np.diff(g["goff"]) == 0)[0])
        assert not dW[empty].any() and not db[empty].any(), "an empty relation's gradients are not zero"


# ---- bits that must not move -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", (False, True))
@pytest.mark.parametrize("d", ec.BITS_WIDTHS)
def test_bits_do_not_depend_on_relation_labels_or_row_numbering(d, exact):
    g = ec.graph("crafted")
    h, G = ec.inputs("normal", d)
    base = run(g, h, G, exact=exact)
    order = np.array([4, 6, 2, 0, 5, 1, 3])
    moved = run(ec.relabelled(g, order), h, G, exact=exact)
    assert same(moved, (base[0][dev(order)], base[1][dev(order)])), "the bits depend on where a relation stands in the table"
    g2, h2, G2 = ec.pregathered(g, h, G)
    assert same(run(g2, h2, G2, exact=exact), base), "the bits depend on which rows the edges name"


@pytest.mark.parametrize("exact", (False, True))
@pytest.mark.parametrize("d", ec.BITS_WIDTHS)
def test_powers_of_two_pass_through_exactly(d, exact):
    """h 2^a, G 2^b gives 2^(a+b) times dW and 2^b times db, bit for bit: a wrong up- or down-scale shows in the exponent."""
    g = ec.graph("short")
    h, G = ec.inputs("clamped", d)
    base = run(g, h, G, exact=exact)
    assert base[0].abs().max() > 1 and base[1].abs().max() > 1
    for a, b in ec.RESCALES:
        got = run(g, np.ldexp(h, a), np.ldexp(G, b), exact=exact)
        want = tuple((x.double() * 2.0 ** k).float() for x, k in zip(base, (a + b, b)))           # (db sums G alone)
        assert all((w.double() == x.double() * 2.0 ** k).all() for w, x, k in zip(want, base, (a + b, b))), "the scaled result leaves fp32"
        assert same(got, want), f"d={d} exact={exact}: h 2^{a}, G 2^{b} is not 2^{a + b} times dW and 2^{b} times db"


@pytest.mark.parametrize("d", (128, 384))
def test_scaled_entry_point_gives_the_plain_bits_at_exponent_boundaries(d):
    """ghf_edge_outer_scaled reads each tensor's scale off the row scales: the same bits as the plain call when a tensor's largest
    entry is exactly a power of two, or one ulp below one."""
    g = ec.graph("short")
    h0, G0 = ec.inputs("normal", d)
    for value in (np.float32(8.0), np.nextafter(np.float32(8.0), np.float32(0.0)), np.float32(-8.0)):
        for h, G in ((ec.top_entry(h0, value), G0), (h0, ec.top_entry(G0, value))):
            ws = torch.zeros(len(g["slice_tab"]) * (2 * 128 * 128 + 128) + 64, device=DEV)
            got = run(g, h, G, h_scales=scales(h), G_scales=scales(G), workspace=ws)
            assert same(got, run(g, h, G)), f"d={d}: the scaled call differs with {value!r} as the largest entry"
            assert ws[-64:].view(torch.int32)[2:6].tolist() == [0, ec.N, 0, ec.N]
            assert not same(got, run(g, h, G, exact=True))


# ---- range guard -------------------------------------------------------------------------------------------------------
def guarded(g, h, G, trips):
    """The scaled call: its four counters against the numpy counts, its bits against the chain the counters choose."""
    ns = len(g["slice_tab"])
    ws = torch.zeros(ns * (2 * 128 * 128 + 128) + 64, device=DEV)
    got = run(g, h, G, h_scales=scales(h), G_scales=scales(G), workspace=ws)
    counters = ws.view(torch.int32)[ns * (2 * 128 * 128 + 128) + 2:][:4].tolist()          # (ghf.h: ghf_edge_outer_scaled)
    assert counters == [*ec.guard_counts(h), *ec.guard_counts(G)], "far-down / nonzero rows of h, of G"
    assert ec.guard_trips(h, G) == trips
    fp32, pieces = run(g, h, G, exact=True), run(g, h, G)
    assert not torch.equal(fp32[0], pieces[0]), "the two chains agree on this case: it cannot tell which one ran"
    assert same(got, fp32 if trips else pieces), f"the call did not run on the {'fp32' if trips else 'two-piece'} chain"


@pytest.mark.parametrize("side", ("h", "G"))
@pytest.mark.parametrize("name", tuple(ec.GUARD_CASES))
def test_range_guard_counts_and_decides(name, side):
    g = ec.small_graph(80, ec.GUARD_CUTS, "guard")
    guarded(g, *ec.guard_inputs(ec.GUARD_CASES[name], side, 128, name), ec.GUARD_TRIPS[name])


def test_range_guard_at_two_tiles_per_row():
    name = "56 of 64 far down"
    guarded(ec.small_graph(80, ec.GUARD_CUTS, "guard"), *ec.guard_inputs(ec.GUARD_CASES[name], "G", 256, name), True)


@pytest.mark.parametrize("side", ("h", "G"))
def test_range_guard_counts_forty_workgroups_of_rows(side):
    """N = 40,000: 40 workgroups, four trips of their grid-stride loop, atomics from every wave."""
    g = ec.small_graph(ec.GUARD_BIG_N, ec.GUARD_CUTS, "guard_big")
    guarded(g, *ec.guard_inputs(ec.GUARD_BIG, side, 128, "big"), True)


def test_tripped_guard_walks_three_hundred_slices():
    """More slices than edge_outer_guarded_kernel has workgroups: its walking loop, and the LDS it reuses from slice to slice."""
    g = ec.small_graph(80, ec.WALK_CUTS, "walk")
    assert len(g["slice_tab"]) == ec.WALK_SLICES
    guarded(g, *ec.guard_inputs(ec.GUARD_CASES["56 of 64 far down"], "G", 128, "walk"), True)


# ---- rows beyond 4 GiB -------------------------------------------------------------------------------------------------
def test_rows_beyond_four_gib():
    """h and G of 2^23 + 64 rows at d = 128 (4 GiB + 32 KiB each): edge_outer_h_kernel<false>.  Half of the touched rows start
    beyond byte 2^32; an offset kept in 32 bits lands on another touched row (tests/test_edge_outer_host.py)."""
    if torch.cuda.mem_get_info()[0] < 16e9:
        pytest.skip("needs 16 GB of free device memory")
    c = ec.big_rows_case()
    g, ids = c["g"], dev(c["ids"])
    small = run(g, c["h"], c["G"])
    Ar, Br = ec.rows(g, c["h"], c["G"])
    check_exact(small[0], ec.int_sums(Ar, Br, g["goff"]), "compact rows dW")
    big = dict(g, src=c["ids"][g["src"]], dst=c["ids"][g["dst"]], N=ec.BIG_N)
    h, G = (torch.zeros(ec.BIG_N, 128, device=DEV).index_copy_(0, ids, dev(x)) for x in (c["h"], c["G"]))
    assert h.numel() * 4 >= 1 << 32
    try:
        for exact in (False, True):
            got = run(big, h, G, exact=exact)
            assert same(got, small), f"exact={exact}: rows beyond 4 GiB give other bits than the same rows compacted"
    finally:
        del h, G
        _TABLES.clear()
        torch.cuda.empty_cache()


# ---- the plan builder's own tables ---------------------------------------------------------------------------------------
def test_train_plan_tables_of_short_slices(monkeypatch):
    """build_train_plan with SLICE_EDGES = 96 on 1,000 edges: its tables keep the ABI's rules and give the exact sums."""
    monkeypatch.setattr(autograd, "SLICE_EDGES", 96)
    d, N, R = 128, ec.N, 6
    ei = np.stack([synth.randint(92, "eo_tp_s", 1000, N), synth.randint(92, "eo_tp_d", 1000, N)])
    rel = synth.randint(92, "eo_tp_r", 1000, R - 1)
    tp = autograd.build_train_plan(dev(ei), dev(rel), build_plan(dev(ei), dev(rel), [""] * R, N, d, DEV), d, DEV)
    g = dict(src=tp.src_by_rel.cpu().numpy(), dst=tp.dst_by_rel.cpu().numpy(), goff=tp.goff.cpu().numpy(),
             slice_tab=tp.slice_tab.cpu().numpy(), slice_off=tp.slice_off.cpu().numpy(), N=N, R=R)
    ec.check_slice_rules(g["slice_tab"], g["slice_off"], g["goff"], tp.slice_order.cpu().tolist())
    assert sorted(zip(g["src"].tolist(), g["dst"].tolist())) == sorted(zip(ei[0].tolist(), ei[1].tolist()))
    h, G = ec.inputs("int", d)
    Ar, Br = ec.rows(g, h, G)
    for exact in (False, True):
        dW, db = run(g, h, G, exact=exact, order=tp.slice_order)
        check_exact(dW, ec.int_sums(Ar, Br, g["goff"]), f"train plan exact={exact} dW")
        check_exact(db, ec.int_sums(ec.ones(g), Br, g["goff"]), f"train plan exact={exact} db")
