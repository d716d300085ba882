"""Degenerate rows for the layer's tail, h' = LayerNorm(ReLU(agg / max(indeg, 1) + h) * drop): the row catalogue, its
reference, the bounds the comparisons use and the geometry of ghf_tail_bwd's walk over the rows, restated.

Not collected by pytest (test_tail_rows_host.py and test_tail_rows_gpu.py import it).  numpy only, no GPU.

The reference forms pre32 = float32(agg) + float32(h) in float32 — the one rounding every kernel shares, so that each
entry lies on the kernel's side of the ReLU kink — and computes everything after it in float64: ReLU, mask, biased
variance, LayerNorm and the analytic backward (dpre, G = dpre / max(indeg, 1), dgamma, dbeta).

The rows are the ones seeded random data never produces: rows without a live entry, rows without variance, rows whose
mean is 2^10 times their spread, a single live column at every lane / column-group / wave boundary, entries on and
beside the kink (zeros of both signs, subnormals, sums that cancel), rows scaled by 2^-40 .. 2^40, rows the dropout mask
kills.  The comparisons state the tail's contract: the variance is two-pass, a row without variance is beta bit for bit,
the gradient at pre <= 0 is exactly 0, a positive subnormal is live."""

from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import numpy as np

from _util import ATOL, RTOL, assert_close
from graph_hypernetwork_forge_amd import synth

LN_EPS = 1e-5
INDEG = (0, 1, 2, 3, 7, 1 << 20, (1 << 24) + 1, (1 << 31) - 1)
SUBNORMAL = np.float32(2.0 ** -149)                       # the smallest positive float32
MIN_NORMAL = np.float32(2.0 ** -126)
KEEP = np.float32(1.0 / 0.75)                             # a kept entry of a dropout mask at p = 0.25
CONSTS = (0.5, 1.0, 3.0, 1024.0)
SCALES = (-40, -20, 20, 40)
ONE_LIVE_COLUMNS = (0, 3, 4, 63, 64, 255, 256)            # and d - 1
G_RTOL = 3e-7                                             # G against dpre / max(indeg, 1): the kernels multiply by a rounded 1 / c
G_ATOL = 2.0 ** -149                                      # ... and a G below 2^-126 is rounded to a multiple of 2^-149

# ---- ghf_tail_bwd's walk, restated (csrc/backward.hip) -----------------------------------------------------------------
# min(cdiv(N, 4), TB_BLOCKS) workgroups of four waves; a wave of tail_bwd_v4_kernel<LPR, NV> holds 64 / LPR rows per
# visit, a wave of tail_bwd_kernel one row; a workgroup comes back to the rows one grid further on.
TB_BLOCKS = 2048
V4_LPR = {32: 8, 64: 16, 128: 32, 256: 64, 512: 64, 1024: 64}      # the widths of the v4 kernel and their lanes per row
GENERIC_BWD_WIDTHS = (3, 20, 100, 257, 1023)
CS_ROWS = 512                                             # ghf_colsum: rows per workgroup and pass


def tail_bwd_blocks(N: int) -> int:
    return max(min(-(-N // 4), TB_BLOCKS), 1)


def rows_per_visit(d: int, v4: bool = True) -> int:
    """Rows a full grid of ghf_tail_bwd covers in one visit."""
    return TB_BLOCKS * 4 * (64 // V4_LPR[d] if v4 and d in V4_LPR else 1)


def visit_of(N: int, d: int, v4: bool = True) -> np.ndarray:
    """[N]: the visit (0, 1, ...) in which row v of an N-row launch is reached."""
    per_wave = 64 // V4_LPR[d] if v4 and d in V4_LPR else 1
    return np.arange(N) // (tail_bwd_blocks(N) * 4 * per_wave)


def tail_bwd_workspace_floats(N: int, d: int) -> int:
    nb = tail_bwd_blocks(N)
    n1 = -(-nb // CS_ROWS)
    return nb * 2 * d + (n1 + -(-n1 // CS_ROWS)) * 2 * d


def third_visit_N(d: int, v4: bool = True) -> int:
    """The smallest N with a third visit, plus four: the third visit is a short one that ends inside a workgroup."""
    return 2 * rows_per_visit(d, v4) + 5


# ---- the catalogue -----------------------------------------------------------------------------------------------------

class Catalogue(NamedTuple):
    d: int
    names: List[str]
    agg: np.ndarray          # [K, d] float32
    h: np.ndarray            # [K, d] float32
    drop: np.ndarray         # [K, d] float32, 0 or 1 / 0.75 (all ones on the rows whose sums must stay exact)
    gamma: np.ndarray        # [d] float32: a zero, a negative entry, the rest in [0.5, 1.5]
    beta: np.ndarray         # [d] float32, no zero
    indeg: np.ndarray        # [K] int32, INDEG in turn

    @property
    def K(self) -> int:
        return len(self.names)

    @property
    def pre32(self) -> np.ndarray:
        return self.agg + self.h                          # float32 + float32

    def rows(self, prefix: str) -> List[int]:
        return [i for i, n in enumerate(self.names) if n.startswith(prefix)]

    def row(self, name: str) -> int:
        return self.names.index(name)

    def x32(self, dropping: bool) -> np.ndarray:
        """The rows LayerNorm sees, in float32 (a product with 0 or 4/3: one rounding, the kernels' own)."""
        x = np.maximum(self.pre32, np.float32(0.0))
        return x * self.drop if dropping else x


def _seeded_mask(seed: int, tag: str, d: int) -> np.ndarray:
    return ((synth.uniform01(seed, tag, d) < 0.75) * KEEP).astype(np.float32)


def catalogue(d: int, seed: int = 7700) -> Catalogue:
    """Named rows of pre = agg + h at width d, with the layer's gamma / beta, a dropout mask and in-degrees.  Rows given
    directly carry agg = -0.0, which leaves every h as it is (zeros keep their sign)."""
    assert d >= 3
    names: List[str] = []
    aggs, hs, drops = [], [], []
    col = np.arange(d)
    ones = np.ones(d, dtype=np.float32)
    neg0 = np.full(d, -0.0, dtype=np.float32)

    def add(name, h, agg=None, drop=None):
        names.append(name)
        hs.append(np.asarray(h, dtype=np.float32).copy())
        aggs.append(neg0.copy() if agg is None else np.asarray(agg, dtype=np.float32).copy())
        drops.append(ones.copy() if drop is None else np.asarray(drop, dtype=np.float32).copy())

    # no live entry: zeros of both signs, negative normals, a negative subnormal, the negative smallest normal
    dead_vals = np.array([-0.0, 0.0, -1.5, -SUBNORMAL, -3.25, -MIN_NORMAL, -1e-3], dtype=np.float32)
    add("dead", dead_vals[col % dead_vals.size])
    for c in CONSTS:
        add(f"const_{c:g}", np.full(d, c))
    add("offset", 1024.0 + synth.randint(seed, "offset", d, 64) / 8.0)
    for j in sorted({min(j, d - 1) for j in ONE_LIVE_COLUMNS + (d - 1,)}):
        v = np.zeros(d)
        v[j] = 2.5
        add(f"one_live_{j}", v)
    # the kink: O(1) entries between zeros of both signs, +- the smallest subnormal, +- the smallest normal
    special = np.array([0.0, -0.0, SUBNORMAL, -SUBNORMAL, MIN_NORMAL, -MIN_NORMAL], dtype=np.float32)
    body = synth.normal(seed, "kink/body", (d,))
    add("kink_direct", np.where(col % 3 == 0, body, special[(col // 3 + col) % special.size]))
    # ... and reached by cancellation: agg = -h (the sum is +0.0) or agg = -h (1 + 2^-23) (the sum is one ulp of h, either sign)
    hk = synth.normal(seed, "kink/h", (d,))
    hk = np.where(np.abs(hk) < 0.05, np.float32(0.5), hk).astype(np.float32)
    beside = (-hk * np.float32(1.0 + 2.0 ** -23)).astype(np.float32)
    add("kink_cancel", hk, agg=np.where(col % 3 == 0, synth.normal(seed, "kink/agg", (d,), std=0.5), np.where(col % 3 == 1, -hk, beside)),
        drop=_seeded_mask(seed, "kink/mask", d))
    base = synth.normal(seed, "scale/base", (d,))
    for e in SCALES:
        add(f"scale_{e}", base * np.float32(2.0 ** e), drop=_seeded_mask(seed, f"scale/mask{e}", d))
    # rows the mask kills: zero on every live column (kept on the dead ones); the second keeps one live column
    m = np.abs(synth.normal(seed, "masked/h", (d,))) + np.float32(0.1)
    m[1::5] *= np.float32(-1.0)
    dead_mask = np.where(m > 0, np.float32(0.0), KEEP)
    add("masked_all", m, drop=dead_mask)
    one = dead_mask.copy()
    one[int(np.nonzero(m > 0)[0][-1])] = KEEP
    add("masked_one", m, drop=one)
    for i in range(4):
        add(f"filler_{i}", synth.normal(seed, f"filler/h{i}", (d,)), agg=synth.normal(seed, f"filler/agg{i}", (d,)),
            drop=_seeded_mask(seed, f"filler/mask{i}", d))

    gamma = (0.5 + synth.uniform01(seed, "gamma", d)).astype(np.float32)
    gamma[1 % d] = 0.0
    gamma[2 % d] *= -1.0
    u = synth.uniform01(seed, "beta", d)
    beta = (np.where(synth.uniform01(seed, "beta/sign", d) < 0.5, -1.0, 1.0) * (0.1 + 0.4 * u)).astype(np.float32)
    K = len(names)
    indeg = np.array([INDEG[i % len(INDEG)] for i in range(K)], dtype=np.int32)
    return Catalogue(d, names, np.stack(aggs), np.stack(hs), np.stack(drops), gamma, beta, indeg)


# ---- the reference -----------------------------------------------------------------------------------------------------

def tail_ref(agg, h, gamma, beta, drop=None, gout=None, indeg=None, eps: float = LN_EPS) -> Dict[str, np.ndarray]:
    """The tail and its backward: pre32 in float32, the rest in float64.  Keys: pre32, out, rstd, xhat; with `gout` also
    dpre, G (needs indeg), dgamma, dbeta."""
    pre32 = np.asarray(agg, dtype=np.float32) + np.asarray(h, dtype=np.float32)
    gamma, beta = np.asarray(gamma, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    m = np.ones_like(pre32, dtype=np.float64) if drop is None else np.asarray(drop, dtype=np.float64)
    x = np.maximum(pre32.astype(np.float64), 0.0) * m
    mu = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(axis=1, keepdims=True) + eps)
    xhat = (x - mu) * rstd
    res = dict(pre32=pre32, out=xhat * gamma + beta, rstd=rstd, xhat=xhat)
    if gout is not None:
        g = np.asarray(gout, dtype=np.float64)
        gg = g * gamma
        dx = rstd * (gg - gg.mean(axis=1, keepdims=True) - xhat * (gg * xhat).mean(axis=1, keepdims=True))
        res["dpre"] = np.where(pre32 > 0, dx * m, 0.0)
        if indeg is not None:
            res["G"] = res["dpre"] / np.maximum(np.asarray(indeg, dtype=np.float64), 1.0)[:, None]
        res["dgamma"], res["dbeta"] = (g * xhat).sum(axis=0), g.sum(axis=0)
    return res


# ---- exactness of the fp32 mean ----------------------------------------------------------------------------------------

def ulp32(a) -> np.ndarray:
    a = np.abs(np.asarray(a, dtype=np.float32))
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def sum_exact_in_any_order(x) -> bool:
    """Every partial sum of the float32 row, in any order, is a float32: all entries are multiples of one power of two q
    and sum |x| < 2^24 q."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    nz = x[x != 0]
    if not nz.size:
        return True
    q = 2.0 ** np.floor(np.log2(np.abs(nz).min()))
    while not np.all(nz / q == np.round(nz / q)):
        q /= 2.0
        if q < 2.0 ** -160:
            return False
    return float(np.abs(nz).sum() / q) < 2.0 ** 24


def mean_exact(x, d: Optional[int] = None) -> bool:
    """The float32 mean of the row is its true mean under both forms the kernels use — sum / d and sum * (1 / d), float32
    throughout — whatever the order of the additions."""
    x = np.asarray(x, dtype=np.float32)
    d = x.size if d is None else d
    if not sum_exact_in_any_order(x):
        return False
    s = np.float32(x.astype(np.float64).sum())
    true = x.astype(np.float64).sum() / d
    by_div = np.float32(s / np.float32(d))
    by_rcp = np.float32(s * np.float32(np.float32(1.0) / np.float32(d)))
    return float(by_div) == true and float(by_rcp) == true


def exact_mean_rows(cat: Catalogue, dropping: bool) -> List[int]:
    """The rows whose float32 mean is exact under both forms (mean_exact on what LayerNorm sees)."""
    x = cat.x32(dropping)
    return [i for i in range(cat.K) if mean_exact(x[i])]


def zero_variance_rows(cat: Catalogue, dropping: bool) -> List[int]:
    x = cat.x32(dropping)
    return [i for i in range(cat.K) if bool((x[i] == x[i][0]).all())]


def beta_rows(cat: Catalogue, dropping: bool) -> List[int]:
    """Rows that must come out as beta bit for bit: no variance and an exact float32 mean (dead, masked_all under the
    mask, const_c where the mean is exact)."""
    ex = set(exact_mean_rows(cat, dropping))
    return [i for i in zero_variance_rows(cat, dropping) if i in ex]


def mean_ulp_rows(cat: Catalogue, dropping: bool) -> List[int]:
    """const_c and offset where the float32 mean is not exact: the rows that get the extra term of `forward_bound`."""
    ex = set(exact_mean_rows(cat, dropping))
    return [i for i, n in enumerate(cat.names) if (n.startswith("const_") or n == "offset") and i not in ex]


def backward_rows(cat: Catalogue, dropping: bool) -> List[int]:
    """The rows ghf_tail_bwd is run on: every row but the zero-variance ones whose float32 mean is not exact (there
    rstd = 316 turns an ulp of xhat into 1e-4 of dx)."""
    ex = set(exact_mean_rows(cat, dropping))
    zv = set(zero_variance_rows(cat, dropping))
    return [i for i in range(cat.K) if i not in zv or i in ex]


def forward_bound(cat: Catalogue, ref: Dict[str, np.ndarray], dropping: bool) -> np.ndarray:
    """[K, d]: the error allowed per element — _util.assert_close's atol + rtol |ref|, and on the rows of mean_ulp_rows
    two ulps of the mean (a correctly rounded division costs half an ulp, a multiply by a rounded 1 / d up to one and a
    half) carried through (x - mean) rstd gamma: 2 ulp32(max |x|) rstd |gamma|."""
    bound = ATOL + RTOL * np.abs(ref["out"])
    x = cat.x32(dropping)
    for i in mean_ulp_rows(cat, dropping):
        bound[i] += 2.0 * float(ulp32(np.abs(x[i]).max())) * ref["rstd"][i] * np.abs(cat.gamma.astype(np.float64))
    return bound


# ---- float32 restatements of the tail ----------------------------------------------------------------------------------

def tail_f32(cat: Catalogue, dropping: bool, form: str = "div", one_pass: bool = False, eps: float = LN_EPS) -> np.ndarray:
    """The forward in numpy float32: the two-pass tail with the mean as sum / d ("div") or sum * (1 / d) ("rcp"); or, with
    `one_pass`, the variance as E[x^2] - mean^2."""
    f = np.float32
    x = cat.x32(dropping)
    d = f(cat.d)
    scale = (lambda s: (s / d).astype(f)) if form == "div" else (lambda s: (s * f(f(1.0) / d)).astype(f))
    mean = scale(x.sum(axis=1, keepdims=True, dtype=f))
    if one_pass:
        var = np.maximum(scale((x * x).sum(axis=1, keepdims=True, dtype=f)) - mean * mean, f(0.0))
    else:
        t = (x - mean).astype(f)
        var = scale((t * t).sum(axis=1, keepdims=True, dtype=f))
    rstd = (f(1.0) / np.sqrt(var + f(eps), dtype=f)).astype(f)
    return ((x - mean) * rstd * cat.gamma + cat.beta).astype(f)


def tail_bwd_f32(cat: Catalogue, gout, dropping: bool, form: str = "div", eps: float = LN_EPS) -> Dict[str, np.ndarray]:
    """The backward in numpy float32 (two-pass statistics again, as the kernels recompute them): dpre, dgamma, dbeta."""
    f = np.float32
    x = cat.x32(dropping)
    d = f(cat.d)
    scale = (lambda s: (s / d).astype(f)) if form == "div" else (lambda s: (s * f(f(1.0) / d)).astype(f))
    mean = scale(x.sum(axis=1, keepdims=True, dtype=f))
    t = (x - mean).astype(f)
    rstd = (f(1.0) / np.sqrt(scale((t * t).sum(axis=1, keepdims=True, dtype=f)) + f(eps), dtype=f)).astype(f)
    xh = (t * rstd).astype(f)
    g = np.asarray(gout, dtype=f)
    gg = (g * cat.gamma).astype(f)
    s1 = (gg.sum(axis=1, keepdims=True, dtype=f) / d).astype(f)
    s2 = ((gg * xh).sum(axis=1, keepdims=True, dtype=f) / d).astype(f)
    dx = (rstd * (gg - s1 - xh * s2)).astype(f)
    m = cat.drop if dropping else np.ones_like(x)
    return dict(dpre=np.where(cat.pre32 > 0, dx * m, f(0.0)).astype(f), dgamma=(g * xh).sum(axis=0, dtype=f), dbeta=g.sum(axis=0, dtype=f))


def gout_for(K: int, d: int, seed: int = 7701) -> np.ndarray:
    return synth.normal(seed, "gout", (K, d))


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


# ---- derived catalogues and the comparisons ----------------------------------------------------------------------------

def take(cat: Catalogue, idx) -> Catalogue:
    """The catalogue's rows `idx` (repeats allowed), in that order."""
    idx = np.asarray(idx, dtype=np.int64)
    return cat._replace(names=[cat.names[i] for i in idx], agg=cat.agg[idx], h=cat.h[idx], drop=cat.drop[idx], indeg=cat.indeg[idx])


def as_h(cat: Catalogue) -> Catalogue:
    """The same rows handed over as h alone (agg = +0.0): what a fused kernel sees whose aggregate is exactly zero."""
    return cat._replace(agg=np.zeros_like(cat.agg), h=cat.pre32)


def check_forward(got, cat: Catalogue, dropping: bool, what: str, eps: float = LN_EPS) -> Dict[str, float]:
    """`got` [K, d] float32 against the reference on the rows of `cat`: beta_rows bit for bit, mean_ulp_rows inside
    forward_bound, the rest under _util.assert_close.  Returns the figures for the record."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == cat.h.shape, f"{what}: {got.dtype} {got.shape}"
    ref = tail_ref(cat.agg, cat.h, cat.gamma, cat.beta, cat.drop if dropping else None, eps=eps)
    exact, loose = beta_rows(cat, dropping), mean_ulp_rows(cat, dropping)
    for i in exact:
        assert np.array_equal(bits(got[i]), bits(cat.beta)), f"{what}: row {i} ({cat.names[i]}) is not beta bit for bit"
    err = np.abs(got.astype(np.float64) - ref["out"])
    bound = forward_bound(cat, ref, dropping)
    worst = int(np.argmax((err - bound).max(axis=1)))
    fig = dict(bit_rows=len(exact), ulp_rows=len(loose), ulp_err=float(err[loose].max()) if loose else 0.0,
               ulp_share=float((err[loose] / bound[loose]).max()) if loose else 0.0, max_err=float(err.max()))
    print(f"FIG tail {what} rows={cat.K} bit_for_bit={sorted({cat.names[i] for i in exact})} "
          f"mean_ulp={sorted({cat.names[i] for i in loose})} mean_ulp_max_err={fig['ulp_err']:.3e} share={fig['ulp_share']:.3f} "
          f"max_err={fig['max_err']:.3e}")
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    assert (err <= bound).all(), f"{what}: row {worst} ({cat.names[worst]}) leaves its bound by {(err - bound)[worst].max():.3e}"
    plain = [i for i in range(cat.K) if i not in set(loose)]
    assert_close(got[plain], ref["out"][plain], what + ": the rows without the mean-ulp term")
    return fig


def check_backward(dpre, G, dgamma, dbeta, cat: Catalogue, gout, dropping: bool, what: str, eps: float = LN_EPS) -> None:
    """ghf_tail_bwd's outputs on the rows of `cat` (already restricted to backward_rows) against the reference, and the
    exact claims: dpre is nonzero only where pre32 > 0 under a nonzero mask, zero at +-0.0, and a positive subnormal is live."""
    dpre, G = np.asarray(dpre), np.asarray(G)
    assert dpre.dtype == G.dtype == np.float32
    ref = tail_ref(cat.agg, cat.h, cat.gamma, cat.beta, cat.drop if dropping else None, gout, cat.indeg, eps=eps)
    pre = ref["pre32"]
    live = (pre > 0) & ((cat.drop != 0) if dropping else True)
    assert not (dpre[~live] != 0).any(), f"{what}: dpre is nonzero at pre <= 0 or under a zero mask"
    assert not (G[~live] != 0).any(), f"{what}: G is nonzero at pre <= 0 or under a zero mask"
    assert (dpre[pre == 0] == 0).all(), f"{what}: dpre at +-0.0"
    sub = live & (pre < MIN_NORMAL) & (np.abs(ref["dpre"]) > 1e-30)
    assert (dpre[sub] != 0).all(), f"{what}: a positive subnormal pre was treated as dead"
    e = np.abs(dpre.astype(np.float64) - ref["dpre"])
    worst = np.unravel_index(int(np.argmax(e - ATOL - RTOL * np.abs(ref["dpre"]))), e.shape)
    print(f"FIG tail {what} rows={cat.K} dpre_max_err={e.max():.3e} dpre_worst={cat.names[worst[0]]}[{worst[1]}] err={e[worst]:.3e} "
          f"of {ATOL + RTOL * abs(ref['dpre'][worst]):.3e} dgamma_max_err={np.abs(np.asarray(dgamma) - ref['dgamma']).max():.3e} "
          f"subnormal_live={int(sub.sum())} dead_entries={int((~live).sum())}")
    want_G = dpre.astype(np.float64) / np.maximum(cat.indeg.astype(np.float64), 1.0)[:, None]
    assert (np.abs(G.astype(np.float64) - want_G) <= G_ATOL + G_RTOL * np.abs(want_G)).all(), f"{what}: G is not dpre / max(indeg, 1)"
    scale = float(cat.K) ** 0.5                          # the column sums grow like sqrt(rows)
    assert_close(np.asarray(dbeta) / scale, ref["dbeta"] / scale, what + " dbeta")
    assert_close(np.asarray(dgamma) / scale, ref["dgamma"] / scale, what + " dgamma")
    assert_close(dpre, ref["dpre"], what + " dpre")
