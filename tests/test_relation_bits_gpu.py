"""The bits of the relation kernels: ghf_relation_rows, ghf_relation_scores, its two backward calls and ghf_score_softmax_bwd
produce, case by case, exactly the bytes recorded in tests/golden/relation_bits.json.

relation_rows_kernel and rp_sweep_kernel share their arithmetic (csrc/relation_sweep.h), so the cross-check between them
cannot see a change that hits both, and neither the float64-tolerance tests nor the integer-data tests see a reordered
addition.  This test does: the fixture holds a SHA-256 per case over the output tensors' bytes, and equality is exact.

    python tests/test_relation_bits_gpu.py --record [--out PATH] [--commit ID]

records the fixture (on the MI355X, at the build whose bits are to be kept).  Only public _native functions are called.

Inputs come from integer arithmetic alone, identical on any machine and library version: a multiplicative hash of (i, j)
reduced to 16 bits and scaled into [-0.5, 0.5) (exact in fp32; products of two of them are not, so a chain's order shows),
ids from affine maps modulo their range.

Cases, the smallest that reach each branch (geometry from rp_span / rp_wgrad_slab of csrc/relation_predict.hip):
  widths d = 18 (d % 4 != 0: scalar loads and stores), 20 (vectorised, a padded tail of k), 64, 160 (the 192-column
  instantiation), 256; both transposes; bias absent and add_x off in one case per entry point.
  rows:     B = 150, R = 4, queries permuted by i -> 37 i mod 150; relation 0 has 70 rows (two tiles, one partial),
            1 has 5, 2 none, 3 has 75; ix given; one case with a query id out of range (its row is NaN).
  scores:   B = 150, U = 4 (span 1); B = 6422, U = 35, d = 20 (101 tiles, span 4, nine runs, the last of 3 relations).
  row gradients: B = 150, U = 4 (4 splits, the ordered sum); B = 6422, U = 35 (5 splits of 7); B = 32800, U = 3 (513
            tiles, one split, straight to the output).
  weight gradients: B = 150, U = 4 (three slabs, the ordered sum; d = 160: three 64-row bands); B = 40 (one slab, direct);
            with and without dbias.
  softmax backward: N = 50,000, B = 300, d = 128 (the multi-slab case of tests/test_softmax_gpu.py): dq through the
            ordered sum of 12 slab partials."""

import functools
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from _bits import affine, dev, digest, hashed, load_fixture, record_main  # noqa: E402
from graph_hypernetwork_forge_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relation_bits.json")
WIDTHS = (18, 20, 64, 160, 256)
ROWS_X = 997


@functools.lru_cache(maxsize=None)
def rows(d):
    return dev(hashed(ROWS_X, d, 1))


@functools.lru_cache(maxsize=None)
def weights(U, d):
    return dev(hashed(U * d, d, 2).reshape(U, d, d)), dev(hashed(U, d, 3))


@functools.lru_cache(maxsize=None)
def grads(B, U):
    return dev(hashed(B, U, 4))


def case_rows(d, transpose, bias=True, add_x=True, bad=False):
    B, R = 150, 4
    rel_sorted = np.repeat(np.arange(R, dtype=np.int64), (70, 5, 0, 75))
    rel = np.empty(B, dtype=np.int64)
    rel[(37 * np.arange(B)) % B] = rel_sorted
    ix = (np.arange(B, dtype=np.int64) * 7 + 3) % ROWS_X
    if bad:
        ix[111] = ROWS_X                                      # position 3 of relation 0's first tile
    W, b = weights(R, d)
    return (_native.relation_rows(rows(d), dev(rel), W, b if bias else None, ix=dev(ix), add_x=add_x, transpose=transpose),)


def case_scores(B, U, d, transpose, bias=True, add_x=True):
    W, b = weights(U, d)
    return (_native.relation_scores(rows(d), affine(B, 7, 3, ROWS_X), affine(B, 11, 5, ROWS_X), W, b if bias else None,
                                    add_x=add_x, transpose=transpose),)


def case_bwd_rows(B, U, d, transpose, bias=True, add_x=True):
    W, b = weights(U, d)
    return (_native.relation_scores_bwd_rows(rows(d), affine(B, 7, 3, ROWS_X), grads(B, U), W, b if bias else None,
                                             add_x=add_x, transpose=transpose),)


def case_bwd_weights(B, U, d, want_bias=True):
    dW, db = _native.relation_scores_bwd_weights(rows(d), affine(B, 7, 3, ROWS_X), affine(B, 11, 5, ROWS_X), grads(B, U),
                                                 want_bias=want_bias)
    return (dW, db) if want_bias else (dW,)


def case_softmax_bwd():
    N, B, d = 50_000, 300, 128
    c = dev(hashed(N, d, 5))
    iq, target = affine(B, 131, 7, N), affine(B, 977, 11, N)
    scale = d ** -0.5
    _, lse = _native.score_softmax_fwd(c, c, target, iq=iq, scale=scale)
    return _native.score_softmax_bwd(c, c, target, lse, dev(hashed(B, 1, 6).reshape(B)), iq=iq, scale=scale)


def build_cases():
    cases = {}
    for d in WIDTHS:
        for tr in (False, True):
            t = "T" if tr else "N"
            cases[f"rows/d{d}/{t}"] = functools.partial(case_rows, d, tr)
            cases[f"scores/B150_U4/d{d}/{t}"] = functools.partial(case_scores, 150, 4, d, tr)
            cases[f"bwd_rows/B150_U4/d{d}/{t}"] = functools.partial(case_bwd_rows, 150, 4, d, tr)
        cases[f"bwd_weights/B150_U4/d{d}"] = functools.partial(case_bwd_weights, 150, 4, d)
    for tr in (False, True):
        t = "T" if tr else "N"
        cases[f"scores/B6422_U35/d20/{t}"] = functools.partial(case_scores, 6422, 35, 20, tr)
        cases[f"bwd_rows/B6422_U35/d20/{t}"] = functools.partial(case_bwd_rows, 6422, 35, 20, tr)
        cases[f"bwd_rows/B32800_U3/d20/{t}"] = functools.partial(case_bwd_rows, 32800, 3, 20, tr)
    cases["rows/d20/N/no_bias"] = functools.partial(case_rows, 20, False, bias=False)
    cases["rows/d20/T/no_add_x"] = functools.partial(case_rows, 20, True, add_x=False)
    cases["rows/d20/N/bad_id"] = functools.partial(case_rows, 20, False, bad=True)
    cases["rows/d18/T/bad_id"] = functools.partial(case_rows, 18, True, bad=True)
    cases["scores/B150_U4/d20/N/no_bias"] = functools.partial(case_scores, 150, 4, 20, False, bias=False)
    cases["scores/B150_U4/d20/T/no_add_x"] = functools.partial(case_scores, 150, 4, 20, True, add_x=False)
    cases["bwd_rows/B150_U4/d20/N/no_bias"] = functools.partial(case_bwd_rows, 150, 4, 20, False, bias=False)
    cases["bwd_rows/B150_U4/d20/T/no_add_x"] = functools.partial(case_bwd_rows, 150, 4, 20, True, add_x=False)
    cases["bwd_weights/B150_U4/d20/no_dbias"] = functools.partial(case_bwd_weights, 150, 4, 20, want_bias=False)
    cases["bwd_weights/B150_U4/d160/no_dbias"] = functools.partial(case_bwd_weights, 150, 4, 160, want_bias=False)
    cases["bwd_weights/B40_U4/d20"] = functools.partial(case_bwd_weights, 40, 4, 20)
    cases["bwd_weights/B40_U4/d160/no_dbias"] = functools.partial(case_bwd_weights, 40, 4, 160, want_bias=False)
    cases["softmax_bwd/N50000_B300/d128"] = case_softmax_bwd
    return cases


CASES = build_cases()


@functools.lru_cache(maxsize=None)
def recorded():
    return load_fixture(FIXTURE)


def test_the_fixture_names_exactly_these_cases():
    assert sorted(recorded()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_output_bytes_are_the_recorded_ones(name):
    out = CASES[name]()
    if name.endswith("bad_id"):                              # the NaN row is there (and hashed with its neighbours)
        assert bool(torch.isnan(out[0][111]).all()) and int(torch.isnan(out[0]).any(dim=1).sum()) == 1
    else:
        assert all(bool(torch.isfinite(t).all()) for t in out)
    got = digest(out)
    print(f"{name}: {got}")
    assert got == recorded()[name]


if __name__ == "__main__":
    record_main(FIXTURE, CASES)
