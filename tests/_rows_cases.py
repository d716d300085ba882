"""Threshold rows for the range guard of the two-fp16-piece rows (csrc/common.h: range_tiny, range_raise), shared by
test_rows_bits_gpu.py (the kernels) and test_rows_host.py (the proof, in numpy, that the rows are what they claim).

A row of d values is cut after scaling its largest magnitude into [2^13, 2^14); an element is "far down" (tiny) when it is
nonzero and below 2^-14 of the largest, and the guard fires when tiny > 0 and tiny * 8 >= nonzero.  With BIG = 1:

    fires: nz = 16 * ((d - 8) // 16) nonzero entries, nz / 8 of them FAR = 2^-20, the others 1; d - nz (>= 8) zeros.
           tiny * 8 == nz exactly: `>` in place of `>=`, or zeros counted as nonzero, and it no longer fires.
    holds: as `fires`, but two of the far entries are EDGE = 2^-14 — exactly 0.5 once scaled, which is not tiny: tiny * 8 ==
           nz - 16.  `<= 0.5` in place of `< 0.5` makes them tiny, and it fires.

Entries come in adjacent pairs (2k, 2k + 1) of one magnitude; `signed` rows give a pair the signs (+, -), so that the row and
every aligned group of four sum to zero exactly (the LayerNorm backward's mean(gamma g') term vanishes).  Not collected by
pytest and free of the GPU."""

import numpy as np

BIG, EDGE, FAR = np.float32(1.0), np.float32(2.0 ** -14), np.float32(2.0 ** -20)
KINDS = ("fires", "holds")
WIDTHS = (32, 64, 100, 128, 192, 256, 384, 512, 640, 768, 896, 1024)   # every row width a case of test_rows_bits_gpu.py cuts


def threshold_row(d: int, kind: str, signed: bool = False) -> np.ndarray:
    assert kind in KINDS and d >= 32 and d % 2 == 0
    nz = 16 * ((d - 8) // 16)
    far = nz // 8
    row = np.zeros(d, dtype=np.float32)
    row[:nz] = BIG
    at = 16 * np.arange(far // 2) + 2                                # first element of every far pair: one pair in sixteen entries
    row[at] = row[at + 1] = FAR
    if kind == "holds":
        row[at[0]] = row[at[0] + 1] = EDGE
    if signed:
        row[1::2] *= np.float32(-1.0)
    return row


def guard_counts(row: np.ndarray):
    """(tiny, nonzero) as csrc/common.h counts them, in numpy: the row scaled by the power of two that lifts its largest
    magnitude into [2^13, 2^14)."""
    a = np.abs(np.asarray(row, dtype=np.float32))
    mx = float(a.max())
    if mx == 0.0:
        return 0, 0
    s = min(max(13 - int(np.floor(np.log2(mx))), -100), 100)
    xs = a * np.float32(2.0 ** s)
    return int(((xs != 0) & (xs < np.float32(0.5))).sum()), int((xs != 0).sum())


def guard_fires(row: np.ndarray) -> bool:
    tiny, nz = guard_counts(row)
    return tiny > 0 and tiny * 8 >= nz
