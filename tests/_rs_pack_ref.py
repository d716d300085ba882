"""ghf_weights_pack_rs restated in numpy from its contract (include/ghf.h: the relation-stationary layer's operands and the
range guard; csrc/common.h: the two-fp16-piece cut), and the matrices that pin the guard's per-tile rule.  Shared by
test_wide_rows_host.py (the proof that the restatement and the matrices are what they claim) and test_wide_rows_gpu.py (the
kernel, byte for byte).  Not collected by pytest and free of the GPU.

Per relation r, over both natural [k][n] matrices W_msg[r] and W_self[r] (k: input row, n: output column):

    s    = clamp(13 - floor(log2(largest magnitude of the two)), -100, 100)       (an all-zero relation: 100)
    xs   = x * 2^s                        exact in float32; the largest lies in [2^13, 2^14)
    hi   = float16(xs)                    round to nearest even
    lo   = float16(xs - float32(hi))
    w2h  = [r][half: msg, self][piece: hi, lo][n][k] fp16   — the matrix TRANSPOSED: the contraction index contiguous —
           then R float32 2^-s.

Guard word: GHF_RANGE_WEIGHTS when some aligned 32 x 32 tile of some matrix has tiny > 0 and tiny * 8 >= nonzero (tiny: 0 <
|xs| < 0.5); GHF_RANGE_WEAK_W when some relation has an input row whose L1 norm is below d * 2^-16 of the largest row norm of
[W_msg; W_self] (a half that is zero throughout takes no part)."""

import numpy as np

from _rows_cases import BIG, KINDS, threshold_row

RANGE_WEIGHTS, RANGE_WEAK_W = 2, 4
TILE = 32


def shifts(Wm: np.ndarray, Ws: np.ndarray) -> np.ndarray:
    R = Wm.shape[0]
    mx = np.maximum(np.abs(Wm).reshape(R, -1).max(axis=1), np.abs(Ws).reshape(R, -1).max(axis=1)).astype(np.float64)
    s = np.full(R, 100, dtype=np.int64)
    nz = mx >= 2.0 ** -126                                            # (zero and subnormal: exponent field 0, shift clamped)
    s[nz] = np.clip(13 - np.floor(np.log2(mx[nz])).astype(np.int64), -100, 100)
    return s


def scaled(W: np.ndarray, s: np.ndarray) -> np.ndarray:
    """xs [R, k, n] float32."""
    up = np.ldexp(np.float32(1.0), s).astype(np.float32)[:, None, None]
    return (np.asarray(W, dtype=np.float32) * up).astype(np.float32)


def pieces(xs: np.ndarray):
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def pack_rs(Wm: np.ndarray, Ws: np.ndarray) -> np.ndarray:
    """The ghf_weights_rs_bytes(R, d) bytes of ghf_weights_pack_rs(Wm, Ws) as uint8."""
    R, d, _ = Wm.shape
    s = shifts(Wm, Ws)
    out = np.empty((R, 2, 2, d, d), dtype=np.float16)
    for half, W in enumerate((Wm, Ws)):
        hi, lo = pieces(scaled(W, s))
        out[:, half, 0] = hi.transpose(0, 2, 1)
        out[:, half, 1] = lo.transpose(0, 2, 1)
    inv = np.ldexp(np.float32(1.0), -s).astype(np.float32)
    return np.concatenate([out.reshape(-1).view(np.uint8), inv.view(np.uint8)])


def tile_counts(xs: np.ndarray):
    """(tiny, nonzero) [R, d / 32, d / 32] per aligned 32 x 32 tile of xs [R, d, d]."""
    R, d, _ = xs.shape
    a = np.abs(xs).reshape(R, d // TILE, TILE, d // TILE, TILE)
    return ((a != 0) & (a < np.float32(0.5))).sum(axis=(2, 4)), (a != 0).sum(axis=(2, 4))


def guard_word(Wm: np.ndarray, Ws: np.ndarray) -> int:
    R, d, _ = Wm.shape
    s = shifts(Wm, Ws)
    word = 0
    for W in (Wm, Ws):
        tiny, nz = tile_counts(scaled(W, s))
        if bool(((tiny > 0) & (tiny * 8 >= nz)).any()):
            word |= RANGE_WEIGHTS
    norms = [np.abs(W.astype(np.float64)).sum(axis=2) for W in (Wm, Ws)]              # [R, k] per half
    for r in range(R):
        thr = max(n[r].max() for n in norms) * d / 65536.0
        if any(n[r].max() > 0 and n[r].min() < thr for n in norms):
            word |= RANGE_WEAK_W
    return word


# ---- inputs -------------------------------------------------------------------------------------------------------------

def _hashed(n, m, salt):
    """fp32 [n, m] in [-0.5, 0.5) from integer arithmetic alone (tests/_bits.py: hashed, restated free of torch)."""
    i = np.arange(n, dtype=np.uint64)[:, None]
    j = np.arange(m, dtype=np.uint64)[None, :]
    h = (i * np.uint64(2654435761) + j * np.uint64(40503) + np.uint64(salt) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h = ((h * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)
    return ((h.astype(np.int64) - 32768).astype(np.float32) / np.float32(65536.0))


def ordinary_weights(d: int):
    """(W_msg, W_self) [3, d, d]: relation 0 at 2^-3, relation 1 with its largest entry (3.0) in W_self alone, relation 2 all
    zero in W_msg (the shape of the backward's passes: one half is not there)."""
    Wm, Ws = (_hashed(3 * d, d, salt).reshape(3, d, d).copy() for salt in (81, 82))
    Wm[0] *= np.float32(0.25)
    Ws[0] *= np.float32(0.25)
    Ws[1, d - 1, d - 3] = 3.0
    Wm[2] = 0.0
    return Wm, Ws


GUARD_CASES = ("self_last_fires", "msg_interior_fires", "msg_interior_holds")


def guard_tile(kind: str) -> np.ndarray:
    """A 32 x 32 tile at the guard's threshold (tests/_rows_cases.py: a threshold row of 1024 entries, row by row): the largest
    entry is 1; `fires` has tiny * 8 == nonzero exactly, `holds` two entries at exactly 0.5 once scaled in place of two tiny."""
    assert kind in KINDS
    return threshold_row(TILE * TILE, kind).reshape(TILE, TILE)


def guard_weights(d: int, case: str):
    """(W_msg, W_self, (half, relation, k0, n0), expected word) for a name of GUARD_CASES: ordinary_weights(d) with relation 1
    rescaled so that its largest magnitude is 1 (the tile's) and one tile of it replaced."""
    where, kind = case.rsplit("_", 1)
    Wm, Ws = ordinary_weights(d)
    Ws[1, d - 1, d - 3] = np.float32(0.25)
    Wm[1], Ws[1] = np.abs(Wm[1]) + np.float32(0.25), np.abs(Ws[1]) + np.float32(0.25)      # magnitudes in [0.25, 0.75]: far from tiny
    nb = d // TILE
    half, k0, n0 = (1, (nb - 1) * TILE, (nb - 1) * TILE) if where == "self_last" else (0, (nb // 2) * TILE, TILE)
    (Ws if half else Wm)[1, k0:k0 + TILE, n0:n0 + TILE] = guard_tile(kind)
    assert float(max(np.abs(Wm[1]).max(), np.abs(Ws[1]).max())) == float(BIG)
    return Wm, Ws, (half, 1, k0, n0), RANGE_WEIGHTS if kind == "fires" else 0
