"""Case tables, input builders and numpy references of the gradient-reduction and row-exchange kernels:
ghf_group_edges (csrc/plan.hip), ghf_group_outer / matmul_tn / matmul_nn, ghf_segment_axpy, ghf_colsum, ghf_dot
(csrc/backward.hip), ghf_rows_pack / ghf_rows_unpack (csrc/exchange.hip).  No GPU import: tests/test_reduce_host.py checks
everything here on the CPU, tests/test_reduce_gpu.py runs the kernels against it.

Every sum reduction is stated ONE way: rows Ar [n, a] and Br [n, b] cut into groups by an offset table, output
C[g] = Ar[g's rows]^T Br[g's rows].  (group_outer: the gathered rows; matmul_tn: one group of K rows; segment_axpy: a = 1,
Ar = the gathered weights; colsum: Ar = ones; dot: a = b = 1.)  Three kinds of check hang off that statement:

 exact-integer   entries in {-3..3}, weights in {-2..2}: every partial sum in ANY order is an integer below 2^24, exact in
                 fp32, so whatever order a kernel sums in, its result must be bit-equal to the int64 sums (`exact_sums`).  One
                 dropped, doubled or misplaced term cannot hide.  `magnitude_ok` asserts the 2^24 from the case's own inputs.
 rounding        synth.normal inputs against float64 (`float_sums`), under a bound that is derived, not tuned: an output that
                 sums n products in any order, each product and each addition rounded once (u = 2^-24), is off by at most
                 gamma_n sum|a_i||b_i| <= (n + 2) u sum|a_i||b_i| for n u << 1 (Higham, Accuracy and Stability, §3.1), the sum
                 of magnitudes taken in float64 from the inputs; one more u |result| for the addition onto `out` when the
                 call accumulates (`bound`).
 order           ghf_segment_axpy documents its order (e ascending) and its chain is fmaf(w, x, acc): with weights +-2^k the
                 product is exact, and `seg_fold` reproduces the kernel bit for bit on the host.  `SEG_PROBES` are literal
                 columns whose ascending fold is 0, 0, 1 and whose other orders are not.
"""

import numpy as np

from graph_hypernetwork_forge_amd import synth

U = 2.0 ** -24
LIMIT = 2 ** 24


def ints(seed, name, shape, lo, hi):
    """float32 integers in {lo..hi}."""
    n = int(np.prod(shape))
    return (synth.randint(seed, name, n, hi - lo + 1) + lo).astype(np.float32).reshape(shape)


def values(kind, seed, name, shape, lo=-3, hi=3):
    """kind "int": integers in {lo..hi}; "normal": synth.normal."""
    return ints(seed, name, shape, lo, hi) if kind == "int" else synth.normal(seed, name, tuple(shape))


# ---- the one statement of a sum reduction, and its references ----------------------------------------------------------
def contract(Ar, Br, goff, dtype):
    """C[g] = Ar[goff[g]:goff[g+1]]^T Br[goff[g]:goff[g+1]] in `dtype`: [G, a, b]."""
    out = np.zeros((len(goff) - 1, Ar.shape[1], Br.shape[1]), dtype=dtype)
    for g in range(len(goff) - 1):
        s, e = int(goff[g]), int(goff[g + 1])
        if e > s:
            out[g] = Ar[s:e].astype(dtype).T @ Br[s:e].astype(dtype)
    return out


def exact_sums(Ar, Br, goff):
    """int64 sums of integer-valued rows (the exact-integer reference)."""
    assert (Ar == np.rint(Ar)).all() and (Br == np.rint(Br)).all(), "exact-integer mode needs integer inputs"
    return contract(Ar, Br, goff, np.int64)


def float_sums(Ar, Br, goff):
    """(float64 sums, float64 sums of magnitudes, products per output [G, 1, 1]) — the rounding-mode reference."""
    n = np.diff(np.asarray(goff, dtype=np.int64)).astype(np.float64)[:, None, None]
    return contract(Ar, Br, goff, np.float64), contract(np.abs(Ar), np.abs(Br), goff, np.float64), n


def bound(mag, n, accumulated=None):
    """(n + 2) 2^-24 sum|a||b|, plus 2^-24 |result| when the sums were added onto a prior `out` (pass the result)."""
    b = (np.asarray(n, dtype=np.float64) + 2.0) * U * mag
    return b if accumulated is None else b + U * np.abs(np.asarray(accumulated, dtype=np.float64))


def magnitude_ok(Ar, Br, goff, prior=None):
    """Exact-integer condition: sum |terms| (plus |prior| when accumulating) < 2^24 for every output."""
    mag = contract(np.abs(Ar), np.abs(Br), goff, np.float64)              # (integers far below 2^53: exact in float64)
    if prior is not None:
        mag = mag + np.abs(prior.reshape(mag.shape)).astype(np.float64)
    return float(mag.max(initial=0)) < LIMIT


def scrambled_f32(Ar, Br, goff, seed):
    """A plain numpy float32 evaluation with every group's rows in a scrambled order (what the references must survive).
    Small groups: the float32 products summed by numpy's own (pairwise) reduction over the scrambled rows.  Large groups: a
    float32 matrix product of the scrambled rows — the order inside it is then the BLAS library's blocking, not the scramble's:
    still another order than any kernel's, which is all this evaluation is for."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(goff) - 1, Ar.shape[1], Br.shape[1]), dtype=np.float32)
    for g in range(len(goff) - 1):
        s, e = int(goff[g]), int(goff[g + 1])
        if e > s:
            p = s + rng.permutation(e - s)
            small = (e - s) * Ar.shape[1] * Br.shape[1] < 1 << 18
            if small:
                out[g] = (Ar[p, :, None] * Br[p, None, :]).sum(axis=0, dtype=np.float32)
            else:
                out[g] = Ar[p].T @ Br[p]
    return out


# ---- ghf_group_edges ---------------------------------------------------------------------------------------------------
def group_edges_cases():
    """(name, keys int64 [E], R) — every key in range."""
    r = lambda name, E, R: synth.randint(71, name, E, R)                   # noqa: E731
    cases = [("E=1 R=1", np.zeros(1, dtype=np.int64), 1),
             ("R+1 > E", r("ge_wide", 50, 100003), 100003),
             ("E=70000 R=5", r("ge_long", 70000, 5), 5)]
    cases += [(f"E=300 R={R}", r(f"ge_{R}", 300, R), R) for R in (2, 3, 256, 257)]
    cases.append(("all equal", np.full(300, 4, dtype=np.int64), 7))
    cases.append(("descending, duplicates", np.sort(r("ge_desc", 300, 7))[::-1].copy(), 7))
    cases.append(("relations 0, 3, 6 absent", np.array([1, 2, 4, 5], dtype=np.int64)[r("ge_absent", 300, 4)], 7))
    return cases


def group_reference(keys, R):
    """(perm, goff) of a stable sort by key."""
    perm = np.argsort(keys, kind="stable").astype(np.int64)
    return perm, np.searchsorted(keys[perm], np.arange(R + 1), side="left").astype(np.int64)


def out_of_range_keys():
    """300 keys for R = 7 of which some are -1, R and 2^40."""
    keys = synth.randint(72, "ge_bad", 300, 7)
    keys[5::17] = -1
    keys[6::19] = 7
    keys[7::23] = 1 << 40
    keys[0], keys[299] = 1 << 40, -1
    return keys, 7


def check_out_of_range_grouping(keys, R, perm, goff):
    """What a grouping of out-of-range keys must still satisfy; where those keys land is not pinned."""
    E = len(keys)
    assert perm.shape == (E,) and goff.shape == (R + 1,)
    assert np.array_equal(np.sort(perm), np.arange(E)), "perm is not a permutation of 0..E-1"
    assert goff[0] == 0 and goff[R] == E and (np.diff(goff) >= 0).all(), "goff is not a non-decreasing 0..E table"
    pos = np.empty(E, dtype=np.int64)
    pos[perm] = np.arange(E)
    ok = (keys >= 0) & (keys < R)
    k = keys[ok]
    assert ((goff[k] <= pos[ok]) & (pos[ok] < goff[k + 1])).all(), "an in-range key lies outside its group's range"


# ---- ghf_group_outer ---------------------------------------------------------------------------------------------------
# Each wave takes a quarter of a group rounded up to a multiple of 4; the whole-tile path needs 16 edges per wave: from 64 on.
GROUP_SIZES = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 67, 255, 256, 257, 1031, 0)
GOFF = np.concatenate([[0], np.cumsum(GROUP_SIZES)]).astype(np.int64)
# da == 0 (A = None), partial row and column tiles, a whole tile next to a partial one, a second and a third o_base launch
OUTER_DIMS = ((0, 1), (0, 130), (1, 16), (15, 24), (16, 128), (17, 129), (20, 20), (48, 144), (16, 272))
OUTER_MODES = ("identity", "gather", "ia_only")           # both None; both given, repeated rows; ia given and ib None
OUTER_TABLE_ROWS = (97, 113)                              # rows of A / B when gathered through ia / ib: fewer than edges


def outer_inputs(da, db, mode, kind, seed=0):
    """dict(A or None, ia or None, B, ib or None) for the GROUP_SIZES table; da == 0 is A = None (ia unused)."""
    E = int(GOFF[-1])
    tag = f"{da}x{db}.{mode}.{kind}.{seed}"
    has_ia = da > 0 and mode in ("gather", "ia_only")
    has_ib = mode == "gather"
    na, nb = (OUTER_TABLE_ROWS[0] if has_ia else E), (OUTER_TABLE_ROWS[1] if has_ib else E)
    return dict(A=values(kind, 73, "go_a." + tag, (na, da)) if da > 0 else None,
                ia=synth.randint(73, "go_ia." + tag, E, na) if has_ia else None,
                B=values(kind, 73, "go_b." + tag, (nb, db)),
                ib=synth.randint(73, "go_ib." + tag, E, nb) if has_ib else None)


def outer_rows(inp):
    """(Ar [E, max(da, 1)], Br [E, db]): the rows each edge contributes (A = None: ones)."""
    B = inp["B"] if inp["ib"] is None else inp["B"][inp["ib"]]
    if inp["A"] is None:
        return np.ones((B.shape[0], 1), dtype=np.float32), B
    return (inp["A"] if inp["ia"] is None else inp["A"][inp["ia"]]), B


def outer_pregathered(inp):
    """The identity call on pre-gathered rows: the same C, bit for bit, as the call that gathers through ia / ib."""
    Ar, Br = outer_rows(inp)
    return dict(A=None if inp["A"] is None else np.ascontiguousarray(Ar), ia=None, B=np.ascontiguousarray(Br), ib=None)


def outer_prior(da, db, kind):
    """What `accumulate` adds onto: an integer pattern (exact-integer mode) or normals."""
    shape = (len(GROUP_SIZES), max(da, 1), db)
    return ints(74, f"go_c.{da}x{db}", shape, -50, 50) if kind == "int" else synth.normal(74, f"go_c.{da}x{db}", shape)


def outer_permuted(inp, order):
    """The same groups standing in the order `order` in the table: (inputs, goff).  C'[k] must be C[order[k]], bit for bit."""
    edges = np.concatenate([np.arange(GOFF[g], GOFF[g + 1]) for g in order] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    goff = np.concatenate([[0], np.cumsum([GROUP_SIZES[g] for g in order])]).astype(np.int64)
    out = dict(inp)
    for tab, idx in (("A", "ia"), ("B", "ib")):
        if inp[idx] is not None:
            out[idx] = inp[idx][edges]
        elif inp[tab] is not None:
            out[tab] = inp[tab][edges]
    return out, goff


# ---- matmul_tn / matmul_nn ---------------------------------------------------------------------------------------------
MATMUL_K = (1, 511, 512, 513, 2049, 40000)
MATMUL_MN = ((17, 129), (16, 128), (3, 5))


def matmul_inputs(K, M, N, kind):
    """A [K, M], B [K, N]; the integers shrink to {-1, 0, 1} at K = 40000."""
    lo, hi = (-1, 1) if K >= 40000 else (-3, 3)
    return values(kind, 75, f"mm_a.{K}.{M}.{kind}", (K, M), lo, hi), values(kind, 75, f"mm_b.{K}.{N}.{kind}", (K, N), lo, hi)


def matmul_slices(K, M, N):
    """How many row slices matmul_tn cuts K into (its documented rule: one slice up to 512 rows, else ~2000 workgroups of at
    least 256 rows); the two-level sum adds the slices' partial products, so its bound counts K + slices terms."""
    tiles = ((M + 15) // 16) * ((N + 127) // 128)
    step = K if K <= 512 else max(256, ((K * tiles + 2047) // 2048 + 3) & ~3)
    return (K + step - 1) // step


# ---- ghf_segment_axpy --------------------------------------------------------------------------------------------------
# VW = 1 (d < 128 or odd), 2 (even d from 128), 4 (d % 4 == 0 from 256), each with and without a second column pass
SEG_D = (1, 7, 64, 126, 128, 130, 254, 256, 258, 260, 516, 1028)
SEG_LENGTHS = (0, 0, 1, 2, 3, 4, 5, 1000, 0)
SEG_NSEG = (1, 3, 4, 5, 4097)
SEG_NSEG_D = (7, 130, 260)
SEG_NW, SEG_NX = 211, 157                                 # rows of w and of X: iw != ix, both with repeats


def seg_lengths(nseg):
    """Segment lengths for `nseg` segments: the table itself at its own length; short mixes of empty and full segments
    around the workgroup's four waves; the table cycled (the long segment once) for many workgroups."""
    small = {1: (5,), 3: (0, 5, 0), 4: (3, 0, 0, 1000), 5: (0, 2, 1000, 0, 1), len(SEG_LENGTHS): SEG_LENGTHS}
    if nseg in small:
        return small[nseg]
    return tuple(SEG_LENGTHS[i % 9] if (i < 9 or i % 9 != 7) else 6 for i in range(nseg))


def seg_inputs(d, lengths, kind, clamp=False):
    """dict(w, iw, X, ix, off).  kind "int": w in {-2..2}, X in {-3..3}; "normal"; "pow2": w = +-2^k, k in [-3, 3], X normal.
    clamp: some ix are -5 and nx + 5 (the kernel clamps them into [0, nx)); iw always stays in range."""
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    E = int(off[-1])
    tag = f"{d}.{len(lengths)}.{kind}"
    if kind == "int":
        w = ints(76, "sa_w." + tag, (SEG_NW,), -2, 2)
    elif kind == "pow2":
        w = (np.ldexp(1.0, synth.randint(76, "sa_k." + tag, SEG_NW, 7) - 3) * (1 - 2 * synth.randint(76, "sa_s." + tag, SEG_NW, 2))).astype(np.float32)
    else:
        w = synth.normal(76, "sa_w." + tag, (SEG_NW,))
    X = values("int" if kind == "int" else "normal", 76, "sa_x." + tag, (SEG_NX, d))
    iw, ix = synth.randint(76, "sa_iw." + tag, E, SEG_NW), synth.randint(76, "sa_ix." + tag, E, SEG_NX)
    if clamp:
        ix[::7] = -5
        ix[3::11] = SEG_NX + 5
    return dict(w=w, iw=iw, X=X, ix=ix, off=off)


def seg_rows(inp):
    """(Ar [E, 1] = w[iw], Br [E, d] = X[clip(ix)], off)."""
    return inp["w"][inp["iw"]][:, None], inp["X"][np.clip(inp["ix"], 0, inp["X"].shape[0] - 1)], inp["off"]


def seg_fold(inp):
    """The kernel's own chain on the host: acc = fl(acc + fl(w x)), e ascending, float32 throughout.  Bit-equal to
    fmaf(w, x, acc) when every product is exact (weights +-2^k)."""
    Ar, Br, off = seg_rows(inp)
    lengths = np.diff(off)
    acc = np.zeros((len(lengths), Br.shape[1]), dtype=np.float32)
    for t in range(int(lengths.max(initial=0))):
        live = np.nonzero(lengths > t)[0]
        e = off[live] + t
        acc[live] = acc[live] + (Ar[e] * Br[e]).astype(np.float32)
    return acc


SEG_PROBES = ((2.0 ** 24, 1.0, 1.0, -2.0 ** 24), (2.0 ** 24, 1.0, -2.0 ** 24), (1.0, 2.0 ** 24, -2.0 ** 24, 1.0))
SEG_PROBE_SUMS = (0.0, 0.0, 1.0)                          # ascending float32 folds


def fold_f32(seq, order="ascending"):
    """float32 sum of a short sequence in a named order (what the probes can tell apart)."""
    x = [np.float32(v) for v in seq]
    if order == "descending":
        x = x[::-1]
    elif order == "ends":                                 # (first + last) + (second + second last) ...
        x = [np.float32(x[i] + x[-1 - i]) if i != len(x) - 1 - i else x[i] for i in range((len(x) + 1) // 2)]
    elif order == "neighbours":                           # (x0 + x1) + (x2 + x3) ...
        x = [np.float32(x[i] + x[i + 1]) if i + 1 < len(x) else x[i] for i in range(0, len(x), 2)]
    elif order == "stride2":                              # (x0 + x2 + ...) + (x1 + x3 + ...)
        x = [fold_f32(x[0::2]), fold_f32(x[1::2])]
    elif order == "swapped pairs":                        # x1, x0, x3, x2, ...
        x = [x[i ^ 1] if (i ^ 1) < len(x) else x[i] for i in range(len(x))]
    acc = np.float32(0.0)
    for v in x:
        acc = np.float32(acc + v)
    return float(acc)


def probe_inputs(d):
    """The three probes as three segments, w = 1, every column of X the probe's sequence."""
    col = np.concatenate([np.asarray(p, dtype=np.float32) for p in SEG_PROBES])
    off = np.concatenate([[0], np.cumsum([len(p) for p in SEG_PROBES])]).astype(np.int64)
    return dict(w=np.ones(1, dtype=np.float32), iw=np.zeros(len(col), dtype=np.int64),
                X=np.repeat(col[:, None], d, axis=1).copy(), ix=np.arange(len(col), dtype=np.int64), off=off)


# ---- ghf_colsum --------------------------------------------------------------------------------------------------------
COLSUM_N = (1, 511, 512, 513, 262145)                     # one, two, three tree levels
COLSUM_D = (1, 3, 4, 1021, 1028)                          # 1028: a second column tile of one vector
COLSUM_BIG_D = 4                                          # the large N runs at d <= 4 only
COLSUM_D4 = tuple(d for d in COLSUM_D if d % 4 == 0)      # widths whose aligned call takes the float4 kernel


def colsum_inputs(N, d, kind):
    """dict(X, mask (normals: the kernel reads its sign), prior (what `out` holds before an accumulating call))."""
    tag = f"{N}.{d}.{kind}"
    return dict(X=values(kind, 77, "cs_x." + tag, (N, d)), mask=synth.normal(77, "cs_m." + tag, (N, d)),
                prior=values(kind, 77, "cs_o." + tag, (d,), -50, 50))


def colsum_rows(inp, masked):
    """(Ar = ones [N, 1], Br = X (where mask > 0), [0, N])."""
    X = inp["X"]
    Br = np.where(inp["mask"] > 0, X, np.float32(0.0)) if masked else X
    return np.ones((X.shape[0], 1), dtype=np.float32), Br, np.array([0, X.shape[0]], dtype=np.int64)


# ---- ghf_dot -----------------------------------------------------------------------------------------------------------
DOT_N = (1, 255, 256, 8191, 8192, 8193, 64 * 8192 + 1)


def dot_inputs(n, kind):
    """(X in {-3..3}, Y in {-2..2}) or two normal vectors."""
    return values(kind, 78, f"dot_x.{n}.{kind}", (n,)), values(kind, 78, f"dot_y.{n}.{kind}", (n,), -2, 2)


def dot_rows(X, Y):
    return X[:, None], Y[:, None], np.array([0, len(X)], dtype=np.int64)


# ---- ghf_rows_pack / ghf_rows_unpack -----------------------------------------------------------------------------------
# (row_bytes, extra_bytes): a message row is row_bytes + extra_bytes long — with a 4-byte scale behind a split row every
# second message row starts 4-byte aligned only
ROW_SHAPES = ((16, 0), (16, 4), (512, 4), (1024, 0), (1040, 8), (2048, 4))
ROW_N = (0, 1, 3, 4, 5, 33000)                            # 33000 > 4 * 8192: the grid-stride loop
SENTINEL = 0xA5


def rows_count(n):
    """Rows of the tables a message of n rows is cut from: few (pack repeats them), or a few more than n (unpack's are distinct)."""
    return 37 if n <= 5 else n + 7


def random_bytes(seed, name, shape):
    """Random bytes (NaN bit patterns included)."""
    n = int(np.prod(shape))
    return synth.raw_u64(seed, name, (n + 7) // 8).view(np.uint8)[:n].reshape(shape).copy()


def rows_tables(nrows, row_bytes, extra_bytes, name):
    """(rows [nrows, row_bytes], extra [nrows, extra_bytes] or None) uint8."""
    return (random_bytes(79, f"rp_r.{name}", (nrows, row_bytes)),
            random_bytes(79, f"rp_x.{name}", (nrows, extra_bytes)) if extra_bytes else None)


def pack_reference(rows, extra, idx, before):
    """The message after a pack into a buffer holding `before`: index_select of the listed rows, entries outside
    [0, nrows) left as they were."""
    out = before.copy()
    ok = (idx >= 0) & (idx < rows.shape[0])
    out[ok, :rows.shape[1]] = rows[idx[ok]]
    if extra is not None:
        out[ok, rows.shape[1]:] = extra[idx[ok]]
    return out


def unpack_reference(rows, extra, idx, packed):
    """The tables after an unpack of `packed` to the (distinct) rows idx; entries outside [0, nrows) skipped."""
    rows, extra = rows.copy(), None if extra is None else extra.copy()
    ok = (idx >= 0) & (idx < rows.shape[0])
    rows[idx[ok]] = packed[ok, :rows.shape[1]]
    if extra is not None:
        extra[idx[ok]] = packed[ok, rows.shape[1]:]
    return rows, extra


def pack_indices(n, nrows, name, bad=False):
    """n indices with repeats (pack); bad: some are -1 and nrows."""
    idx = synth.randint(80, f"rp_i.{name}", n, nrows)
    if n >= 2:
        idx[1] = idx[0]
    if bad:
        idx[0::5] = -1
        idx[2::7] = nrows
    return idx


def unpack_indices(n, nrows, name, bad=False):
    """n distinct indices (unpack); bad: some are -1 and nrows."""
    idx = np.argsort(synth.raw_u64(80, f"rp_p.{name}", nrows), kind="stable")[:n].astype(np.int64)
    if bad:
        idx[0::5] = -1
        idx[2::7] = nrows
    return idx


# ---- autograd level: HyperGNN.score_edges ------------------------------------------------------------------------------
SCORE_D = (20, 256, 260)
SCORE_N, SCORE_P, SCORE_HUB = 400, 6000, 3000


def score_pairs_case(d):
    """(embs [N, d], src, dst [P], weights [P]): node 7 sits in SCORE_HUB of the pairs, 50 pairs are self pairs."""
    embs = synth.normal(81, f"se_e.{d}", (SCORE_N, d))
    src, dst = synth.randint(81, f"se_s.{d}", SCORE_P, SCORE_N), synth.randint(81, f"se_d.{d}", SCORE_P, SCORE_N)
    src[src == 7] = 8
    dst[dst == 7] = 9
    src[0:2 * (SCORE_HUB // 2):2] = 7                     # half of the hub's pairs as source ...
    dst[1:2 * (SCORE_HUB // 2):2] = 7                     # ... half as destination
    src[-50:] = dst[-50:]                                 # self pairs (not the hub's)
    return embs, src, dst, synth.normal(81, f"se_w.{d}", (SCORE_P,))
