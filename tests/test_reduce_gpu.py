"""Exact parity suite of the gradient-reduction and row-exchange kernels, called directly through _native: ghf_group_edges,
ghf_group_outer (and matmul_tn / matmul_nn on top of it), ghf_segment_axpy, ghf_colsum, ghf_dot, ghf_rows_pack /
ghf_rows_unpack — and HyperGNN.score_edges' backward, which chains the first three.

Cases, input builders and references live in tests/_reduce_cases.py (checked on the CPU by tests/test_reduce_host.py).  Three
kinds of check, none with a tuned tolerance:
  exact-integer  small-integer inputs, every partial sum exact in fp32 in any order: torch.equal against int64 numpy sums;
  rounding       synth.normal inputs against float64 under |err| <= (n + 2) 2^-24 sum|a_i||b_i| (+ 2^-24 |result| when the call
                 accumulates); the worst err / bound of every check is printed ("err/bound <kernel> ...", run with -s);
  order          the same call twice gives the same bits; ghf_segment_axpy equals the host's ascending float32 fold bit for bit
                 (power-of-two weights) and the literal probes; ghf_group_outer's C[g] does not depend on where group g stands
                 in the table nor on gathering through ia / ib."""

import numpy as np
import pytest
import torch

import _reduce_cases as rc
from test_hip_parity import _grad_check
from graph_hypernetwork_forge_amd import HyperGNN, _native, autograd
from oracle import hypergnn_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def past_16(a):
    """`a` on the device as a view that starts one float past a 16-byte boundary."""
    t = dev(a)
    flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    view = flat[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def check_exact(got, want, what):
    """Bit equality with int64 sums (every one of them below 2^24: the float32 of it is the integer itself)."""
    want32 = torch.from_numpy(np.asarray(want).astype(np.float32)).reshape(got.shape)
    assert torch.equal(got.cpu(), want32), f"{what}: {int((got.cpu() != want32).sum())} of {want32.numel()} sums differ from the int64 sums"


def check_bound(kernel, what, got, ref, b):
    g = got.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
    assert np.isfinite(g).all(), f"{kernel} {what}: non-finite values"
    err = np.abs(g - ref)
    print(f"err/bound {kernel} {what}: {float(np.max(err / np.where(b > 0, b, 1.0))):.4f}")
    worst = np.unravel_index(int(np.argmax(err - b)), err.shape)
    assert (err <= b).all(), f"{kernel} {what}: err {err[worst]:.3e} > bound {b[worst]:.3e} at {worst}"


# ---- ghf_group_edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,keys,R", rc.group_edges_cases(), ids=[c[0] for c in rc.group_edges_cases()])
def test_group_edges_is_a_stable_sort(name, keys, R):
    want_perm, want_goff = rc.group_reference(keys, R)
    perm, goff = _native.group_edges(dev(keys), R)
    assert perm.dtype == torch.int64 and goff.dtype == torch.int64
    assert np.array_equal(perm.cpu().numpy(), want_perm), f"{name}: perm is not np.argsort(kind='stable')"
    assert np.array_equal(goff.cpu().numpy(), want_goff), f"{name}: goff is not np.searchsorted"
    again = _native.group_edges(dev(keys), R)
    assert torch.equal(again[0], perm) and torch.equal(again[1], goff)


def test_group_edges_out_of_range_keys_give_a_grouping_and_no_error():
    keys, R = rc.out_of_range_keys()
    perm, goff = _native.group_edges(dev(keys), R)
    torch.cuda.synchronize()
    rc.check_out_of_range_grouping(keys, R, perm.cpu().numpy(), goff.cpu().numpy())


# ---- ghf_group_outer ---------------------------------------------------------------------------------------------------
def run_outer(inp, goff, out=None):
    return _native.group_outer(dev(inp["A"]), dev(inp["ia"]), dev(inp["B"]), dev(inp["ib"]), dev(goff), out)


@pytest.mark.parametrize("da,db", rc.OUTER_DIMS)
def test_group_outer_exact_integers(da, db):
    for mode in rc.OUTER_MODES:
        inp = rc.outer_inputs(da, db, mode, "int")
        Ar, Br = rc.outer_rows(inp)
        want = rc.exact_sums(Ar, Br, rc.GOFF)
        got = run_outer(inp, rc.GOFF)
        assert got.shape == (len(rc.GROUP_SIZES), max(da, 1), db)
        check_exact(got, want, f"group_outer {da}x{db} {mode}")
        assert torch.equal(run_outer(inp, rc.GOFF), got)
        prior = rc.outer_prior(da, db, "int")
        assert rc.magnitude_ok(Ar, Br, rc.GOFF, prior)
        out = dev(prior)
        assert run_outer(inp, rc.GOFF, out=out) is out
        check_exact(out, want + prior.astype(np.int64), f"group_outer {da}x{db} {mode} accumulate")


@pytest.mark.parametrize("da,db", rc.OUTER_DIMS)
def test_group_outer_rounding(da, db):
    for mode in rc.OUTER_MODES:
        inp = rc.outer_inputs(da, db, mode, "normal")
        ref, mag, n = rc.float_sums(*rc.outer_rows(inp), rc.GOFF)
        got = run_outer(inp, rc.GOFF)
        check_bound("group_outer", f"{da}x{db} {mode}", got, ref, rc.bound(mag, n))
        assert torch.equal(run_outer(inp, rc.GOFF), got), f"group_outer {da}x{db} {mode}: two calls, two results"
        prior = rc.outer_prior(da, db, "normal")
        out = run_outer(inp, rc.GOFF, out=dev(prior))
        check_bound("group_outer", f"{da}x{db} {mode} accumulate", out, ref + prior, rc.bound(mag, n, accumulated=ref + prior))
        assert torch.equal(run_outer(inp, rc.GOFF, out=dev(prior)), out), f"group_outer {da}x{db} {mode} accumulate: two calls, two results"


@pytest.mark.parametrize("da,db", rc.OUTER_DIMS)
def test_group_outer_bits_do_not_depend_on_position_or_gather(da, db):
    """The inner order over k is the MFMA's; what is required: C[g] has the same bits wherever group g stands in the table and
    whatever its neighbours are, and gathering through ia / ib gives the bits of the identity call on pre-gathered rows."""
    for seed, mode in enumerate(rc.OUTER_MODES):
        inp = rc.outer_inputs(da, db, mode, "normal")
        C = run_outer(inp, rc.GOFF)
        order = np.random.default_rng(100 + seed).permutation(len(rc.GROUP_SIZES))
        assert (order != np.arange(len(order))).any()
        moved, goff = rc.outer_permuted(inp, order)
        assert torch.equal(run_outer(moved, goff), C[dev(order)]), f"group_outer {da}x{db} {mode}: bits depend on the group's place"
        assert torch.equal(run_outer(rc.outer_pregathered(inp), rc.GOFF), C), f"group_outer {da}x{db} {mode}: gather changes the bits"


# ---- matmul_tn / matmul_nn ---------------------------------------------------------------------------------------------
@pytest.fixture
def matmul_calls(monkeypatch):
    """Counts what a matmul_tn runs: the slices of its ghf_group_outer call and whether ghf_colsum summed partial products."""
    seen = {"slices": [], "colsum": 0}
    outer, colsum = _native.group_outer, _native.colsum

    def spy_outer(*a, **k):
        out = outer(*a, **k)
        seen["slices"].append(out.size(0))
        return out

    def spy_colsum(*a, **k):
        seen["colsum"] += 1
        return colsum(*a, **k)

    monkeypatch.setattr(_native, "group_outer", spy_outer)
    monkeypatch.setattr(_native, "colsum", spy_colsum)
    return seen


@pytest.mark.parametrize("K", rc.MATMUL_K)
def test_matmul_exact_integers(K, matmul_calls):
    for M, N in rc.MATMUL_MN:
        A, B = rc.matmul_inputs(K, M, N, "int")
        goff = np.array([0, K])
        assert rc.magnitude_ok(A, B, goff)
        want = rc.exact_sums(A, B, goff)[0]
        got = _native.matmul_tn(dev(A), dev(B))
        assert got.shape == (M, N)
        check_exact(got, want, f"matmul_tn K={K} {M}x{N}")
        assert torch.equal(_native.matmul_tn(dev(A), dev(B)), got)
        check_exact(_native.matmul_nn(dev(A.T), dev(B)), want, f"matmul_nn K={K} {M}x{N}")
        assert matmul_calls["slices"][-3:] == [rc.matmul_slices(K, M, N)] * 3
    # the single-slice return up to 512 rows, the slice step and ghf_colsum over the partial products beyond
    assert matmul_calls["colsum"] == 3 * len(rc.MATMUL_MN) * (K > 512)


@pytest.mark.parametrize("K", rc.MATMUL_K)
def test_matmul_rounding(K):
    for M, N in rc.MATMUL_MN:
        A, B = rc.matmul_inputs(K, M, N, "normal")
        ref, mag, _ = rc.float_sums(A, B, np.array([0, K]))
        b = rc.bound(mag, K + rc.matmul_slices(K, M, N))                       # two levels: K rows, then the slices
        tn, nn = _native.matmul_tn(dev(A), dev(B)), _native.matmul_nn(dev(A.T), dev(B))
        check_bound("matmul_tn", f"K={K} {M}x{N}", tn, ref[0], b[0])
        check_bound("matmul_nn", f"K={K} {M}x{N}", nn, ref[0], b[0])
        assert torch.equal(_native.matmul_tn(dev(A), dev(B)), tn), f"matmul_tn K={K} {M}x{N}: two calls, two results"
        assert torch.equal(_native.matmul_nn(dev(A.T), dev(B)), nn), f"matmul_nn K={K} {M}x{N}: two calls, two results"


# ---- ghf_segment_axpy --------------------------------------------------------------------------------------------------
def run_seg(inp, X=None):
    return _native.segment_axpy(dev(inp["w"]), dev(inp["iw"]), dev(inp["X"]) if X is None else X, dev(inp["ix"]), dev(inp["off"]))


def seg_into(inp, X, out):
    """ghf_segment_axpy into a caller's `out` (the wrapper allocates its own)."""
    w, iw, ix, off = dev(inp["w"]), dev(inp["iw"]), dev(inp["ix"]), dev(inp["off"])
    _native._check(_native.load().ghf_segment_axpy(w.data_ptr(), iw.data_ptr(), X.data_ptr(), ix.data_ptr(), off.data_ptr(),
                                                   off.numel() - 1, X.size(0), X.size(1), out.data_ptr(), _native._stream()),
                   "ghf_segment_axpy")
    return out


@pytest.mark.parametrize("d", rc.SEG_D)
def test_segment_axpy_exact_integers_and_rounding(d):
    for clamp in (False, True):                            # ix with -5 and nx + 5: the reference reads np.clip(ix, 0, nx - 1)
        inp = rc.seg_inputs(d, rc.SEG_LENGTHS, "int", clamp=clamp)
        assert rc.magnitude_ok(*rc.seg_rows(inp))
        got = run_seg(inp)
        assert got.shape == (len(rc.SEG_LENGTHS), d)
        check_exact(got, rc.exact_sums(*rc.seg_rows(inp))[:, 0, :], f"segment_axpy d={d} clamp={clamp}")
        inp = rc.seg_inputs(d, rc.SEG_LENGTHS, "normal", clamp=clamp)
        ref, mag, n = rc.float_sums(*rc.seg_rows(inp))
        got = run_seg(inp)
        check_bound("segment_axpy", f"d={d} clamp={clamp}", got, ref[:, 0, :], rc.bound(mag, n)[:, 0, :])
        assert torch.equal(run_seg(inp), got)


@pytest.mark.parametrize("d", rc.SEG_D)
def test_segment_axpy_sums_in_ascending_order(d):
    """fmaf(w, x, acc), e ascending: with weights +-2^k every product is exact and the host's float32 fold has the same bits."""
    inp = rc.seg_inputs(d, rc.SEG_LENGTHS, "pow2")
    assert torch.equal(run_seg(inp).cpu(), torch.from_numpy(rc.seg_fold(inp))), f"segment_axpy d={d}: not the ascending fold"
    got = run_seg(rc.probe_inputs(d)).cpu()
    want = torch.tensor(rc.SEG_PROBE_SUMS, dtype=torch.float32)[:, None].expand(-1, d)
    assert torch.equal(got, want), f"segment_axpy d={d}: probes give {got[:, 0].tolist()}, the ascending fold {list(rc.SEG_PROBE_SUMS)}"


@pytest.mark.parametrize("nseg", rc.SEG_NSEG)
def test_segment_axpy_segment_counts(nseg):
    for d in rc.SEG_NSEG_D:
        inp = rc.seg_inputs(d, rc.seg_lengths(nseg), "int")
        assert rc.magnitude_ok(*rc.seg_rows(inp))
        got = run_seg(inp)
        assert got.shape == (nseg, d)
        check_exact(got, rc.exact_sums(*rc.seg_rows(inp))[:, 0, :], f"segment_axpy d={d} nseg={nseg}")
        inp = rc.seg_inputs(d, rc.seg_lengths(nseg), "pow2")
        assert torch.equal(run_seg(inp).cpu(), torch.from_numpy(rc.seg_fold(inp))), f"segment_axpy d={d} nseg={nseg}: not the fold"


def test_segment_axpy_misaligned_rows_take_the_scalar_instance_with_the_same_bits():
    """d = 256 with X, then out, one float past a 16-byte boundary: the per-column chain is the same, so are the bits."""
    inp = rc.seg_inputs(256, rc.SEG_LENGTHS, "pow2")
    aligned = run_seg(inp)
    assert torch.equal(aligned.cpu(), torch.from_numpy(rc.seg_fold(inp)))
    X = past_16(inp["X"])
    assert torch.equal(run_seg(inp, X=X), aligned)
    out = past_16(np.full(aligned.shape, np.nan, dtype=np.float32))
    assert torch.equal(seg_into(inp, dev(inp["X"]), out), aligned)
    out = past_16(np.full(aligned.shape, np.nan, dtype=np.float32))
    assert torch.equal(seg_into(inp, X, out), aligned)
    inp = rc.seg_inputs(256, rc.SEG_LENGTHS, "int", clamp=True)
    check_exact(run_seg(inp, X=past_16(inp["X"])), rc.exact_sums(*rc.seg_rows(inp))[:, 0, :], "segment_axpy d=256 misaligned")


# ---- ghf_colsum --------------------------------------------------------------------------------------------------------
def colsum_checks(N, d, place):
    """Exact-integer and rounding checks of one shape, masked or not, into a fresh or a prefilled `out`; X through `place`."""
    tag = f"N={N} d={d}"
    for masked in (False, True):
        inp = rc.colsum_inputs(N, d, "int")
        rows = rc.colsum_rows(inp, masked)
        assert rc.magnitude_ok(*rows, prior=inp["prior"])
        want = rc.exact_sums(*rows)[0, 0]
        X, mask = place(inp["X"]), (dev(inp["mask"]) if masked else None)
        got = _native.colsum(X, mask=mask)
        check_exact(got, want, f"colsum {tag} masked={masked}")
        assert torch.equal(_native.colsum(X, mask=mask), got)
        out = dev(inp["prior"])
        assert _native.colsum(X, mask=mask, out=out) is out
        check_exact(out, want + inp["prior"].astype(np.int64), f"colsum {tag} masked={masked} accumulate")
        inp = rc.colsum_inputs(N, d, "normal")
        ref, mag, n = rc.float_sums(*rc.colsum_rows(inp, masked))
        X, mask = place(inp["X"]), (dev(inp["mask"]) if masked else None)
        got = _native.colsum(X, mask=mask)
        check_bound("colsum", f"{tag} masked={masked}", got, ref[0, 0], rc.bound(mag, n)[0, 0])
        assert torch.equal(_native.colsum(X, mask=mask), got), f"colsum {tag} masked={masked}: two calls, two results"
        total = ref[0, 0] + inp["prior"]
        got = _native.colsum(X, mask=mask, out=dev(inp["prior"]))
        check_bound("colsum", f"{tag} masked={masked} accumulate", got, total, rc.bound(mag, n, accumulated=total)[0, 0])
        assert torch.equal(_native.colsum(X, mask=mask, out=dev(inp["prior"])), got), \
            f"colsum {tag} masked={masked} accumulate: two calls, two results"


@pytest.mark.parametrize("N", rc.COLSUM_N)
def test_colsum(N):
    for d in rc.COLSUM_D:
        if N > 513 and d > rc.COLSUM_BIG_D:                # the three-level tree runs at d <= 4 only
            continue
        colsum_checks(N, d, dev)


@pytest.mark.parametrize("N", rc.COLSUM_N)
def test_colsum_misaligned_rows(N):
    """X one float past a 16-byte boundary at d % 4 == 0: the scalar kernel, whose tree has another shape — bound and exact
    integers only."""
    for d in rc.COLSUM_D4:
        if N > 513 and d > rc.COLSUM_BIG_D:
            continue
        colsum_checks(N, d, past_16)


# ---- ghf_dot -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rc.DOT_N)
def test_dot(n):
    X, Y = rc.dot_inputs(n, "int")
    assert rc.magnitude_ok(*rc.dot_rows(X, Y))
    got = _native.dot(dev(X), dev(Y))
    assert got.shape == (1,)
    check_exact(got, rc.exact_sums(*rc.dot_rows(X, Y)).reshape(1), f"dot n={n}")
    X, Y = rc.dot_inputs(n, "normal")
    ref, mag, terms = rc.float_sums(*rc.dot_rows(X, Y))
    got = _native.dot(dev(X), dev(Y))
    check_bound("dot", f"n={n}", got, ref.reshape(1), rc.bound(mag, terms).reshape(1))
    assert torch.equal(_native.dot(dev(X), dev(Y)), got)


# ---- ghf_rows_pack / ghf_rows_unpack -----------------------------------------------------------------------------------
def pack_into(tables, idx, out):
    """ghf_rows_pack into a caller's message buffer (the wrapper allocates its own)."""
    rows, extra, rb, xb = _native._row_tables(tables)
    _native._check(_native.load().ghf_rows_pack(rows.data_ptr(), rb, _native._ptr(extra), xb, idx.data_ptr(), idx.numel(), rows.size(0),
                                                out.data_ptr(), _native._stream()), "ghf_rows_pack")
    return out


def same_bytes(t, a):
    return torch.equal(t.cpu(), torch.from_numpy(a))


@pytest.mark.parametrize("row_bytes,extra_bytes", rc.ROW_SHAPES)
def test_rows_pack_and_unpack_are_index_select_on_bytes(row_bytes, extra_bytes):
    for n in rc.ROW_N:
        nrows, name = rc.rows_count(n), f"{row_bytes}.{extra_bytes}.{n}"
        rows, extra = rc.rows_tables(nrows, row_bytes, extra_bytes, name)
        host = [t for t in (rows, extra) if t is not None]
        tables = [dev(t) for t in host]
        blank = np.full((n, row_bytes + extra_bytes), rc.SENTINEL, dtype=np.uint8)
        # pack: repeated indices, against index_select on the uint8 views
        idx = rc.pack_indices(n, nrows, name)
        msg = _native.rows_pack(tables, dev(idx))
        assert msg.dtype == torch.uint8 and msg.shape == (n, row_bytes + extra_bytes)
        assert torch.equal(msg, torch.cat([t.index_select(0, dev(idx)) for t in tables], dim=1)), f"rows_pack {name}"
        assert same_bytes(msg, rc.pack_reference(rows, extra, idx, blank))
        # ... out-of-range entries keep the sentinel
        bad = rc.pack_indices(n, nrows, name, bad=True)
        assert same_bytes(pack_into(tables, dev(bad), dev(blank)), rc.pack_reference(rows, extra, bad, blank)), f"rows_pack {name} bad ids"
        # unpack: distinct indices into sentinel tables; rows not listed keep the sentinel
        for flag in (False, True):
            to = rc.unpack_indices(n, nrows, name, bad=flag)
            dst = [torch.full_like(t, rc.SENTINEL) for t in tables]
            _native.rows_unpack(dst, dev(to), msg)
            want = rc.unpack_reference(np.full_like(rows, rc.SENTINEL), None if extra is None else np.full_like(extra, rc.SENTINEL),
                                       to, msg.cpu().numpy())
            assert all(same_bytes(t, w) for t, w in zip(dst, want)), f"rows_unpack {name} bad={flag}"
        assert all(same_bytes(t, h) for t, h in zip(tables, host))                # the source tables are untouched
    # unpack after pack over a permutation restores the tables
    nrows = 1031
    rows, extra = rc.rows_tables(nrows, row_bytes, extra_bytes, f"{row_bytes}.{extra_bytes}.perm")
    tables = [dev(t) for t in (rows, extra) if t is not None]
    perm = dev(rc.unpack_indices(nrows, nrows, "perm"))
    dst = [torch.full_like(t, rc.SENTINEL) for t in tables]
    _native.rows_unpack(dst, perm, _native.rows_pack(tables, perm))
    assert all(torch.equal(a, b) for a, b in zip(dst, tables))


# ---- autograd level: HyperGNN.score_edges ------------------------------------------------------------------------------
def small_model():
    return HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=16, num_layers=1).to(DEV).eval().requires_grad_(False)


@pytest.mark.parametrize("d", rc.SCORE_D)
def test_score_edges_gradient_with_a_hub_node(d):
    """group_edges with node ids as keys (R = N), then segment_axpy over a 3000-pair segment, against float64 autograd of the
    oracle's score_triple in the reference's call form."""
    embs, src, dst, w = rc.score_pairs_case(d)
    model, grads = small_model(), []
    for _ in range(2):
        eg = dev(embs).requires_grad_(True)
        s = model.score_edges(eg, dev(src), dev(dst))
        (s * dev(w)).sum().backward()
        grads.append(eg.grad)
    e64 = torch.from_numpy(embs).double().requires_grad_(True)
    s64 = O.score_triple(e64[torch.from_numpy(src)], e64[torch.from_numpy(dst)])
    (s64 * torch.from_numpy(w).double()).sum().backward()
    _grad_check(f" score_edges / d embs (d={d})", grads[0].cpu().numpy(), e64.grad.numpy())
    assert torch.equal(grads[0], grads[1])
    untouched = np.setdiff1d(np.arange(rc.SCORE_N), np.concatenate([src, dst]))
    assert float(grads[0][dev(untouched)].abs().sum()) == 0.0


@pytest.mark.parametrize("d", rc.SCORE_D)
def test_score_edges_with_zero_pairs(d):
    """Nothing to group: the forward is an empty tensor and the backward a [N, d] gradient of zeros, as the reference's
    score_triple(embs[src], embs[dst]) gives."""
    eg = dev(rc.score_pairs_case(d)[0]).requires_grad_(True)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    s = small_model().score_edges(eg, none, none)
    assert s.shape == (0,) and s.dtype == torch.float32
    s.sum().backward()
    assert eg.grad.shape == (rc.SCORE_N, d) and eg.grad.dtype == torch.float32 and float(eg.grad.abs().sum()) == 0.0
    folded = autograd._fold_rows(torch.zeros(0, d, device=DEV), none, rc.SCORE_N)
    assert folded.shape == (rc.SCORE_N, d) and folded.dtype == torch.float32 and float(folded.abs().sum()) == 0.0
