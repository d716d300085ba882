"""Case tables, input builders and numpy references of the weight-gradient contraction: ghf_edge_outer and
ghf_edge_outer_scaled (csrc/backward.hip).  No GPU import: tests/test_edge_outer_host.py checks everything here on the CPU,
tests/test_edge_outer_gpu.py runs the kernels against it.

The problem is stated ONE way, the reduction suite's (tests/_reduce_cases.py): for relation r over its edges
    Ar = [h[src] | h[dst]]  [n, 2d],   Br = G[dst]  [n, d],   dW[r] = Ar^T Br,   db[r] = 1^T Br,
so `_reduce_cases.contract` over the relations' offsets gives every reference (`rows`).  src, dst, slice_tab and slice_off are
built here by hand (`graph`): the ABI allows any cut that stays inside a relation and leaves no slice empty, and the plan
builder only ever cuts at multiples of its slice length.

Kinds of check:
 exact-integer   h, G in {-3..3}: bit-equal to the int64 sums on both chains.  The pieces chain is exact too: an integer times
                 the tensor's 2^s is an fp16 number, lo = 0, and every partial sum is an integer multiple of 2^(sx+sg) below
                 2^24 of them.
 grid-exact      one tensor on a fine grid (k 2^-15, |k| < 2^15: fifteen bits, four more than an fp16 piece holds), the other in
                 {-1, 0, 1}.  hi + lo reproduce every entry, every product of pieces is a multiple of the grid unit, and as long
                 as sum (|hi| + |lo|) |b| stays below 2^24 units every partial sum in any order is exact: the pieces chain must be
                 bit-equal to the float64 sums and to the exact chain.  A lost hi*lo or lo*hi product cannot hide here (`grid_ok`
                 asserts all of this from the inputs, `cut` is split2h in numpy).
 rounding        synth.normal against float64 under derived bounds.
                 Exact chain (d = 64 or exact=True): an output sums n = edges + slices terms, each product and addition rounded
                 once:  |err| <= (n + 2) 2^-24 sum|a||b|  (Higham §3.1; _reduce_cases.bound).  db likewise with a = 1.
                 Pieces chain: with X = x 2^sx, Y = g 2^sg the kernel sums hi_x hi_y + hi_x lo_y + lo_x hi_y in fp32.  Per operand
                 |X - hi - lo| <= 2^-22 |X| + 2^-25 (the second term is the fp16 subnormal grid, where lo stops being a relative
                 rounding), so what the three products miss of X Y is
                     lo_x lo_y + eps_x Y + X eps_y  <=  3 * 2^-22 |X Y| + 2^-25 (|X| + |Y|)  =  12 u |X Y| + 2^-25 (|X| + |Y|),
                 u = 2^-24.  The three products of fp16 numbers are exact in fp32; 3 n of them are accumulated in fp32 and the S
                 slices' partial sums added: (3 n + S) u sum|X Y| to first order, and 2 u for the second-order terms as in
                 gamma_n <= (n + 2) u.  Scaled back by the exact 2^-(sx+sg):
                     |err| <= (3 n + S + 14) 2^-24 sum|a||b| + 2^-25 (2^-sx sum|b| + 2^-sg sum|a|)       (`pieces_bound`),
                 n the relation's edges, S its slices.  `emulate_pieces` is that chain in numpy (the cut, float32 accumulation
                 per 32-edge tile, the slices in table order) and must itself stay under the bound.  At 4,096 edges the bound is
                 too loose to see a lost piece (that is what the grid-exact cases are for), so the rounding check also runs on a
                 second table whose relations hold at most 129 edges.
 bits            relabelled relations, pre-gathered rows, power-of-two rescaling, ghf_edge_outer_scaled: same bits.
 range guard     the four counters against numpy counts from the row maxima's exponents (`guard_counts`), and the chain taken.
"""

import functools

import numpy as np

import _reduce_cases as rc
from graph_hypernetwork_forge_amd import synth

WIDTHS = (64, 128, 256, 384, 512, 640, 1024)
PIECE_WIDTHS = tuple(d for d in WIDTHS if d % 128 == 0)   # the widths whose default chain is the two-piece one
BITS_WIDTHS = (64, 128, 384)
N, R = 150, 7
TILE = 32                                                 # edges per tile of both kernels
R2_CUTS = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129)
CUTS = {"crafted": ((), (1,), R2_CUTS, (), (4096,), (192, 1), ()),
        "short": ((), (1,), (31, 33, 65), (97,), (129,), (64, 63, 1), ())}       # no relation above 129 edges
HUB, LONE_SRC, LONE_DST = 7, 99, 98                       # rows 98 and 99 are used by one edge only
SEED = 90
FINE_BITS = 15


# ---- edges and slice tables ---------------------------------------------------------------------------------------------
def tables(cuts):
    """(goff [R+1], slice_tab [S, 3] = (relation, first edge, end edge), slice_off [R+1]) of per-relation slice lengths."""
    tab, soff, goff, e = [], [0], [0], 0
    for r, lens in enumerate(cuts):
        for n in lens:
            tab.append((r, e, e + n))
            e += n
        soff.append(len(tab))
        goff.append(e)
    return (np.array(goff, dtype=np.int64), np.array(tab, dtype=np.int64).reshape(-1, 3), np.array(soff, dtype=np.int64))


def check_slice_rules(tab, soff, goff, order=None):
    """The ABI's rules for a work list (ghf.h, ghf_edge_outer): relations ascending, relation r's slices are
    tab[soff[r]:soff[r+1]] and tile goff[r]..goff[r+1] without gap or overlap, none empty, `order` a permutation."""
    tab, soff, goff = np.asarray(tab, dtype=np.int64).reshape(-1, 3), np.asarray(soff), np.asarray(goff)
    assert soff[0] == 0 and soff[-1] == len(tab) and (np.diff(soff) >= 0).all() and len(soff) == len(goff)
    assert (np.diff(tab[:, 0]) >= 0).all(), "relations do not ascend"
    assert (tab[:, 2] > tab[:, 1]).all(), "an empty slice"
    for r in range(len(goff) - 1):
        sl = tab[soff[r]:soff[r + 1]]
        assert (sl[:, 0] == r).all(), "a slice stands in another relation's range of the table"
        ends = np.concatenate([[goff[r]], sl[:, 2]])
        assert (sl[:, 1] == ends[:-1]).all() and ends[-1] == goff[r + 1], "the slices do not tile their relation"
    if order is not None:
        assert sorted(int(k) for k in order) == list(range(len(tab))), "order is not a permutation of the slices"


@functools.lru_cache(maxsize=None)
def graph(name):
    """dict(src, dst [E], goff, slice_tab, slice_off, N, R) of the table `name`: self-loops, duplicated edges, a hub
    destination holding a quarter of relation 2, row N - 1 as a source, and a slice (relation 2's fourth) whose last edge
    reads rows used nowhere else."""
    cuts = CUTS[name]
    goff, tab, soff = tables(cuts)
    E = int(goff[-1])
    src, dst = np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64)
    for r in range(len(cuts)):
        a, b = int(goff[r]), int(goff[r + 1])
        src[a:b], dst[a:b] = (synth.randint(SEED, f"eo_{end}.{name}.{r}", b - a, N - 2) for end in ("src", "dst"))
        k = np.arange(a, b)
        loops, dups = k[(k - a) % 13 == 3], k[((k - a) % 17 == 5)]
        dst[loops] = src[loops]
        src[dups], dst[dups] = src[dups - 1], dst[dups - 1]
    src, dst = src + 2 * (src >= LONE_DST), dst + 2 * (dst >= LONE_DST)      # (every row but the lone two)
    src[goff[:-1][np.diff(goff) > 1] + 1] = N - 1
    a2, b2 = int(goff[2]), int(goff[3])
    dst[a2:b2:4] = HUB
    last = int(tab[int(soff[2]) + 3][2]) - 1                 # the last edge of relation 2's fourth slice
    src[last], dst[last] = LONE_SRC, LONE_DST
    return dict(src=src, dst=dst, goff=goff, slice_tab=tab, slice_off=soff, N=N, R=len(cuts))


def rows(g, h, G):
    """(Ar [E, 2d] = [h[src] | h[dst]], Br [E, d] = G[dst]): the rows each edge contributes."""
    return np.concatenate([h[g["src"]], h[g["dst"]]], axis=1), G[g["dst"]]


def ones(g):
    return np.ones((len(g["src"]), 1), dtype=np.float32)


def int_sums(Ar, Br, goff):
    """_reduce_cases.exact_sums (int64) of integer rows, through float64 products: numpy multiplies int64 matrices without its
    matrix library (a minute at d = 1024), and integer sums this far below 2^53 are the same numbers in float64."""
    assert (Ar == np.rint(Ar)).all() and (Br == np.rint(Br)).all(), "exact-integer mode needs integer inputs"
    assert rc.contract(np.abs(Ar), np.abs(Br), goff, np.float64).max(initial=0) < 2.0 ** 52
    return rc.contract(Ar, Br, goff, np.float64).astype(np.int64)


def counts(g):
    """(edges, slices) of every relation as float64 [R, 1, 1]."""
    return (np.diff(g["goff"]).astype(np.float64)[:, None, None], np.diff(g["slice_off"]).astype(np.float64)[:, None, None])


# ---- inputs -------------------------------------------------------------------------------------------------------------
def inputs(kind, d, name="crafted"):
    """(h, G) [N, d] float32.  "int": {-3..3}; "normal"; "grid_h": h on the fine grid and G in {-1, 0, 1}; "grid_g": the
    roles swapped; "clamped": normals with every magnitude at least 2^-6 (the rescaling check keeps every product normal)."""
    tag = f"{kind}.{d}.{name}"
    if kind == "int":
        return rc.ints(SEED, "eo_h." + tag, (N, d), -3, 3), rc.ints(SEED, "eo_g." + tag, (N, d), -3, 3)
    if kind == "normal":
        return synth.normal(SEED, "eo_h." + tag, (N, d)), synth.normal(SEED, "eo_g." + tag, (N, d))
    if kind == "clamped":
        h, G = inputs("normal", d, name)
        f = lambda x: (np.sign(x) + (x == 0)) * np.maximum(np.abs(x), np.float32(2.0 ** -6))     # noqa: E731
        return f(h).astype(np.float32), f(G).astype(np.float32)
    fine, tern = fine_grid("eo_f." + tag, d), ternary("eo_t." + tag, d)
    return (fine, tern) if kind == "grid_h" else (tern, fine)


def fine_grid(name, d):
    """k 2^-FINE_BITS, k uniform in (-2^FINE_BITS, 2^FINE_BITS); one entry is the largest k, so the tensor's scale is known."""
    top = (1 << FINE_BITS) - 1
    k = synth.randint(SEED, name, N * d, 2 * top + 1) - top
    k[0] = top
    return (k.astype(np.float64) * 2.0 ** -FINE_BITS).astype(np.float32).reshape(N, d)


def ternary(name, d):
    """{-1, 0, 1}: one entry in 16 kept, a third of those zero (an output of the 4,096-edge relation then sums ~170 terms)."""
    t = (synth.randint(SEED, name + ".v", N * d, 3) - 1).reshape(N, d)
    t = np.where(synth.randint(SEED, name + ".k", N * d, 16).reshape(N, d) == 0, t, 0)
    t[0, 0] = 1
    return t.astype(np.float32)


# ---- the two-piece cut and the pieces chain on the host -------------------------------------------------------------------
def shift(x):
    """split2h_shift of the tensor's largest magnitude: 13 - its exponent (clamped to +-100)."""
    m = np.array([np.abs(x).max()], dtype=np.float32)
    e = int((m.view(np.uint32)[0] >> 23) & 255) - 127
    return int(np.clip(13 - e, -100, 100))


def cut(x, s):
    """(scaled, hi, lo) as float32: scaled = x 2^s, hi = fp16(scaled), lo = fp16(scaled - hi) — split2h, cast for cast."""
    xs = (x.astype(np.float32) * np.float32(2.0 ** s)).astype(np.float32)
    hi = xs.astype(np.float16).astype(np.float32)
    lo = (xs - hi).astype(np.float32).astype(np.float16).astype(np.float32)
    return xs, hi, lo


def emulate_pieces(g, h, G, drop=None):
    """(dW [R, 2d, d], db [R, d]) float32 as the two-piece kernel forms them: one scale per tensor, the three piece products
    (lo*hi, hi*lo, hi*hi) accumulated in float32 tile by tile, the slice's sum scaled by 2^-sx 2^-sg, the slices added in table
    order; db in float32 from G itself.  drop = "lh" / "hl" leaves out the lo_x*hi_g / hi_x*lo_g product (what a lost MFMA does)."""
    d, sx, sg = h.shape[1], shift(h), shift(G)
    (_, hh, hl), (_, gh, gl) = cut(h, sx), cut(G, sg)
    down = np.float32(2.0 ** -sx) * np.float32(2.0 ** -sg)
    dW, db = np.zeros((g["R"], 2 * d, d), dtype=np.float32), np.zeros((g["R"], d), dtype=np.float32)
    for r, a, b in g["slice_tab"]:
        acc = np.zeros((2 * d, d), dtype=np.float32)
        for t in range(int(a), int(b), TILE):
            s, v = g["src"][t:min(t + TILE, int(b))], g["dst"][t:min(t + TILE, int(b))]
            Ah, Al = np.concatenate([hh[s], hh[v]], axis=1).T, np.concatenate([hl[s], hl[v]], axis=1).T
            if drop != "lh":
                acc += Al @ gh[v]
            if drop != "hl":
                acc += Ah @ gl[v]
            acc += Ah @ gh[v]
        dW[r] += acc * down
        db[r] += G[g["dst"][int(a):int(b)]].sum(axis=0, dtype=np.float32)
    return dW, db


def grid_ok(g, h, G):
    """The grid-exact condition, from the inputs: dict(reproduced: hi + lo is every scaled entry of both tensors; lo_share: the
    share of the fine tensor's nonzero entries whose lo is not 0; units: the largest sum (|hi| + |lo|) |b| over the outputs, in
    units of the products' common grid — every partial sum in any order is exact in fp32 while that is below 2^24; db_exact:
    see there)."""
    out, pieces, grids = dict(reproduced=True, lo_share=0.0), [], []
    for x in (h, G):
        xs, hi, lo = cut(x, shift(x))
        out["reproduced"] = out["reproduced"] and bool((hi + lo == xs).all())
        nz = xs != 0
        out["lo_share"] = max(out["lo_share"], float((lo[nz] != 0).mean()))
        q = np.concatenate([hi[nz], lo[lo != 0]]).astype(np.float64)
        unit = 2.0 ** 30                                      # the coarsest power of two that divides every piece
        while not (q / unit == np.rint(q / unit)).all():
            unit /= 2.0
        grids.append(unit)
        pieces.append((np.abs(hi) + np.abs(lo)).astype(np.float64))
    Ar, Br = rows(g, pieces[0], pieces[1])
    out["units"] = float(rc.contract(Ar, Br, g["goff"], np.float64).max()) / (grids[0] * grids[1])
    out["db_exact"] = db_exact(g, G)
    return out


def db_exact(g, G):
    """[R] bool: the relations whose db = sum G[dst] is exact in fp32 in any order — sum |G| below 2^24 of G's own grid."""
    q = np.abs(G[g["dst"]]).astype(np.float64)
    unit = 2.0 ** 30
    while not (q / unit == np.rint(q / unit)).all():
        unit /= 2.0
    return rc.contract(ones(g), q, g["goff"], np.float64).max(axis=(1, 2)) / unit < rc.LIMIT


# ---- references and bounds ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def float_reference(kind, d, name):
    """dict(dW, db float64; mag, mag_b: the sums of magnitudes; sum_a [R, 2d, 1], sum_b [R, 1, d]) of inputs(kind, d, name)
    on graph(name) — computed once for the checks of a case, never written to (the last two kept: 230 MB each at d = 1024)."""
    g = graph(name)
    h, G = inputs(kind, d, name)
    Ar, Br = rows(g, h, G)
    dW, mag, _ = rc.float_sums(Ar, Br, g["goff"])
    db, mag_b, _ = rc.float_sums(ones(g), Br, g["goff"])
    sum_a = rc.contract(np.abs(Ar), ones(g), g["goff"], np.float64)
    ref = dict(dW=dW, db=db[:, 0, :], mag=mag, mag_b=mag_b[:, 0, :], sum_a=sum_a, sum_b=mag_b)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def exact_bounds(g, ref):
    """(bound of dW, bound of db) on the exact fp32 chain: n = edges + slices terms per output."""
    n, S = counts(g)
    return rc.bound(ref["mag"], n + S), rc.bound(ref["mag_b"], (n + S)[:, :, 0])


def pieces_bound(g, ref, sx, sg):
    """(3 n + S + 14) 2^-24 sum|a||b| + 2^-25 (2^-sx sum|b| + 2^-sg sum|a|): the module docstring's derivation."""
    n, S = counts(g)
    return (3.0 * n + S + 14.0) * rc.U * ref["mag"] + 2.0 ** -25 * (2.0 ** -sx * ref["sum_b"] + 2.0 ** -sg * ref["sum_a"])


# ---- bits that must not move ----------------------------------------------------------------------------------------------
def relabelled(g, order):
    """The same relations, cut alike, standing in the order `order`: dW'[k], db'[k] must be dW[order[k]], db[order[k]]."""
    edges, cuts = [], []
    for r in order:
        edges.append(np.arange(g["goff"][r], g["goff"][r + 1]))
        sl = g["slice_tab"][g["slice_off"][r]:g["slice_off"][r + 1]]
        cuts.append(tuple(int(b - a) for _, a, b in sl))
    edges = np.concatenate(edges).astype(np.int64)
    goff, tab, soff = tables(cuts)
    return dict(src=g["src"][edges], dst=g["dst"][edges], goff=goff, slice_tab=tab, slice_off=soff, N=g["N"], R=g["R"])


def pregathered(g, h, G):
    """(graph, h', G') with a fresh row for every edge end: h' = [h[src]; h[dst]; h], G' = [0; G[dst]; G], edge e reading rows
    e and E + e.  (The tensors themselves ride behind, unused, so that each tensor's largest magnitude — its scale — stays.)"""
    E = len(g["src"])
    e = np.arange(E, dtype=np.int64)
    h2 = np.concatenate([h[g["src"]], h[g["dst"]], h])
    G2 = np.concatenate([np.zeros((E, G.shape[1]), dtype=np.float32), G[g["dst"]], G])
    return dict(g, src=e, dst=E + e, N=len(h2)), np.ascontiguousarray(h2), np.ascontiguousarray(G2)


RESCALES = ((-30, 0), (0, -40), (20, -20), (-30, -30))


def top_entry(x, value):
    """x with its largest magnitude replaced by `value` (which must stay the largest)."""
    x = x.copy()
    i = np.unravel_index(int(np.argmax(np.abs(x))), x.shape)
    x[i] = value
    assert np.abs(x).max() == abs(value) and (np.abs(x) == abs(value)).sum() == 1
    return x


# ---- range guard ----------------------------------------------------------------------------------------------------------
# A row group is (rows, exponent, mantissa): rows whose largest magnitude is mantissa * 2^exponent.  The tensor's largest rows
# stand at exponent 0, far-down rows at -20; 16 all-zero rows ride along (left out of both counters).
GUARD_CASES = {
    "56 of 64 far down": ((8, 0, 1.5), (56, -20, 1.5), (16, None, 0.0)),                      # 56 * 8 = 64 * 7: trips
    "55 of 64 far down": ((9, 0, 1.5), (55, -20, 1.5), (16, None, 0.0)),
    "a row 14 exponents down does not count": ((8, 0, 1.99), (55, -20, 1.5), (1, -14, 1.0), (16, None, 0.0)),
    "a row 15 exponents down counts": ((8, 0, 1.0), (55, -20, 1.5), (1, -15, 1.99), (16, None, 0.0)),
}
GUARD_TRIPS = {"56 of 64 far down": True, "55 of 64 far down": False, "a row 14 exponents down does not count": False,
               "a row 15 exponents down counts": True}
GUARD_BIG = ((2000, 0, 1.25), (33000, -17, 1.75), (999, -14, 1.0), (1, -15, 1.99), (4000, None, 0.0))   # N = 40,000: trips
GUARD_BIG_N = 40000


def rows_with_maxima(groups, d, name):
    """[sum of rows, d] float32 whose rows have the groups' largest magnitudes, the groups' rows interleaved: every row is a
    normal row scaled below 2^exponent with one entry set to +-mantissa 2^exponent."""
    n = sum(k for k, _, _ in groups)
    body = synth.normal(SEED, "eo_gr." + name, (n, d))
    _, e = np.frexp(np.abs(body).max(axis=1))                 # largest magnitude in [2^(e-1), 2^e)
    exps = np.concatenate([np.full(k, 0 if ex is None else ex) for k, ex, _ in groups])
    mant = np.concatenate([np.full(k, m) for k, _, m in groups])
    X = np.ldexp(body, (exps - e)[:, None]).astype(np.float32)               # now below 2^exponent
    X[mant == 0.0] = 0.0
    col = (np.arange(n) * 7) % d
    sign = 1.0 - 2.0 * (np.arange(n) % 2)
    live = mant != 0.0
    X[np.nonzero(live)[0], col[live]] = (sign * np.ldexp(mant, exps))[live].astype(np.float32)
    where = np.argsort(synth.raw_u64(SEED, "eo_gp." + name, n), kind="stable")
    return np.ascontiguousarray(X[where])


def guard_counts(X):
    """(far-down rows, nonzero rows) of a tensor, from the exponents of its rows' largest magnitudes: a nonzero row counts as
    far down when that exponent lies 15 or more below the tensor's."""
    m = np.abs(X).max(axis=1).astype(np.float32)
    nz = m > 0
    e = ((m.view(np.uint32) >> 23) & 255).astype(np.int64) - 127
    far = nz & (e[nz].max() - e >= 15)
    return int(far.sum()), int(nz.sum())


def guard_trips(h, G):
    """Whether the counters send the call to the exact chain: far > 0 and 8 far >= 7 nonzero, for either tensor."""
    return any(far > 0 and 8 * far >= 7 * nz for far, nz in (guard_counts(h), guard_counts(G)))


def guard_inputs(groups, side, d, name):
    """(h, G): the tensor named by `side` ("h" or "G") from the row groups, the other one plain normals."""
    X = rows_with_maxima(groups, d, f"{name}.{side}.{d}")
    other = synth.normal(SEED, f"eo_go.{name}.{side}.{d}", X.shape)
    return (X, other) if side == "h" else (other, X)


@functools.lru_cache(maxsize=None)
def small_graph(n_rows, cuts, name):
    """Random edges over n_rows rows cut as `cuts` says (the guard and large-N cases' tables)."""
    goff, tab, soff = tables(cuts)
    E = int(goff[-1])
    return dict(src=synth.randint(SEED, "eo_ss." + name, E, n_rows), dst=synth.randint(SEED, "eo_sd." + name, E, n_rows),
                goff=goff, slice_tab=tab, slice_off=soff, N=n_rows, R=len(cuts))


GUARD_CUTS = ((40, 33), (), (64, 1, 31))
WALK_SLICES = 300                                         # more slices than the guarded kernel's 256 workgroups
WALK_CUTS = tuple(tuple(32 + (7 * (60 * r + k)) % 33 for k in range(60)) for r in range(5))


# ---- rows beyond 4 GiB ----------------------------------------------------------------------------------------------------
BIG_N = (1 << 23) + 64                                    # d = 128: row 2^23 starts at byte 2^32
BIG_CUTS = ((333, 1), (), (97, 500, 69))


def big_rows_case():
    """dict(graph over the compacted rows 0..127, ids [128]: the rows of the [BIG_N, 128] tensors they stand for, h, G [128, 128]
    integers).  ids = rows 0..63 and 2^23 .. 2^23 + 63: a byte offset kept in 32 bits sends row 2^23 + k to row k, another
    touched row with other values."""
    g = small_graph(128, BIG_CUTS, "big")
    ids = np.concatenate([np.arange(64), (1 << 23) + np.arange(64)]).astype(np.int64)
    h, G = rc.ints(SEED, "eo_bh", (128, 128), -3, 3), rc.ints(SEED, "eo_bg", (128, 128), -3, 3)
    return dict(g=g, ids=ids, h=h, G=G)
