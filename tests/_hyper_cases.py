"""Crafted shapes for the hypernetwork kernels (csrc/weightgen.hip, csrc/weightgen_bwd.hip, csrc/text_encoder.hip,
ghf_weights_pack) and float64 restatements of what they compute.  Host only: numpy and synth, no GPU import.

The case tables name the route of the launcher every entry is meant to reach; `realised` re-derives that route from the
launcher's own rules (restated here in Python) and asserts it, so a table entry cannot drift away from its purpose when a
threshold in the launcher moves.  tests/test_hypernet_host.py checks the tables and the restatements against the oracle on
the CPU; tests/test_hypernet_gpu.py runs every entry through the kernels.
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from graph_hypernetwork_forge_amd import synth

HEADS = ("W_msg", "W_self", "bias")
LOG_SCALES = {"W_msg": -0.5, "W_self": 0.25, "bias": -1.0}     # off the 0.01 initialisation, one value per head
LAST_GAIN, LAST_BIAS_STD = 30.0, 0.3

# layout constants of include/ghf.h (restated: this module must not load the library)
NATURAL, FRAG16, SPLIT2H = 0, 1, 3


# ---------------------------------------------------------------------------------------------------------------------
# bounds (the issue's: tests/_util.py and test_hip_parity._grad_check, the absolute terms relative to the tensor's scale)
# ---------------------------------------------------------------------------------------------------------------------

def _ratio(got, ref, atol_rel, rtol, l2_bound, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = np.abs(got - ref)
    bound = atol_rel * max(scale, 1e-30) + rtol * np.abs(ref)
    l2 = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
    return max(float((err / bound).max()) if ref.size else 0.0, float(l2 / l2_bound))


def fwd_ratio(got, ref, what="") -> float:
    """Largest error as a fraction of the forward bound: |got - ref| <= 1e-5 max|ref| + 1e-4 |ref|, relative L2 <= 1e-5."""
    return _ratio(got, ref, 1e-5, 1e-4, 1e-5, what)


def grad_ratio(got, ref, what="") -> float:
    """... of the gradient bound: |got - ref| <= 1e-4 max|ref| + 2e-4 |ref|, relative L2 <= 5e-5."""
    return _ratio(got, ref, 1e-4, 2e-4, 5e-5, what)


def text_fwd_ratio(got, ref, what="") -> float:
    """... of the text encoder's forward bound: |got - ref| <= 1e-6 + 1e-4 |ref|, relative L2 <= 1e-5."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    l2 = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
    return max(float((np.abs(got - ref) / (1e-6 + 1e-4 * np.abs(ref))).max()), float(l2 / 1e-5))


# ---------------------------------------------------------------------------------------------------------------------
# the launcher's rules, restated (csrc/weightgen.hip: launch_weightgen_batched; csrc/weightgen_bwd.hip)
# ---------------------------------------------------------------------------------------------------------------------

WG_MAX_WIDTH, WG_MAX_HIDDEN, WG_MAX_L = 1024, 7, 8
WG_HU, WG_UNROLL, WG_LANES = 8, 8, 64
WGB_W, WGB_OR, WGB_RT, WGB_HT = 256, 256, 64, 32
NJT_OF = {32: 2, 64: 4, 128: 8, 256: 16}


def cover(w: int) -> int:
    nc = 32
    while nc < w:
        nc <<= 1
    return nc


def nsplit(n: int) -> int:
    return (n + WGB_OR - 1) // WGB_OR


def weightgen_bwd_supported(T: int, Hh: int, nh: int) -> bool:
    return 0 < T <= WGB_W and (nh == 0 or 0 < Hh <= WGB_W) and 0 <= nh <= WG_MAX_HIDDEN


def layout_supported(layout: int, d_in: int, d_out: int) -> bool:
    if layout == FRAG16:
        return d_in == d_out and d_in % 16 == 0
    if layout == SPLIT2H:
        return d_in == d_out and d_in % 32 == 0 and 2 * d_in * d_out * 4 <= 128 * 1024
    return layout == NATURAL


def derive(T: int, Hh: int, nh: int, d_in: int, d_out: int, R: int, layout: int = NATURAL, aligned: bool = True) -> Dict:
    """What the launchers do with this shape: every quantity a table entry may promise."""
    Hl = Hh if nh else T
    n_mat = d_in * d_out
    mfma = Hl % 16 == 0 and aligned
    if layout in (NATURAL, SPLIT2H):
        fwd = "mfma3" if mfma else "simple"                   # merged launch of all heads | vector ALU, head by head
    else:
        fwd = "mfma_frag16" if mfma else "simple_frag16"      # per head; the bias head: natural order, same pipe
    mtiles = (n_mat + 15) // 16
    out = dict(Hl=Hl, hl16=Hl % 16, fwd=fwd, njt=NJT_OF.get(Hl, 0) if fwd == "mfma3" else None,
               r_rem16=R % 16, r_tiles16=(R + 15) // 16, mtiles=mtiles, last_wg_waves=mtiles % 4 or 4,
               bias_rem16=d_out % 16, n_mat_rem4=n_mat % 4, d_out_rem4=d_out % 4,
               t_rem64=T % WG_LANES, hh_rem8=Hh % WG_HU if nh else None, r_rem8=R % WG_UNROLL,
               pack=layout == SPLIT2H, fused=weightgen_bwd_supported(T, Hh, nh))
    if out["fused"]:
        ns, nsb = nsplit(n_mat), nsplit(d_out)
        out.update(nc_out=cover(Hl), nc_hid=cover(max(T, Hh) if nh else T), nsplit=ns, nsplit_bias=nsb,
                   last_range=n_mat - WGB_OR * (ns - 1), last_range_bias=d_out - WGB_OR * (nsb - 1),
                   r_rem64=R % WGB_RT, r_tiles64=(R + WGB_RT - 1) // WGB_RT, r_rem32=R % WGB_HT,
                   r_tiles32=(R + WGB_HT - 1) // WGB_HT, t_over_h=bool(nh) and T > Hh)
    return out


@dataclass(frozen=True)
class WGShape:
    name: str
    T: int
    Hh: int                 # 0: no hidden layers
    nh: int
    d_in: int
    d_out: int
    R: int
    promise: Tuple[Tuple[str, object], ...]
    seed: int

    @property
    def dims(self):
        return (self.T, self.Hh, self.nh, self.d_in, self.d_out)

    @property
    def shape(self):
        return (self.T, self.Hh, self.nh, self.d_in, self.d_out, self.R)


def _wg(name, shape, seed, **promise) -> WGShape:
    return WGShape(name, *shape, tuple(sorted(promise.items())), seed)


# name, (T, Hh, nh, d_in, d_out, R), seed, the route the entry promises.  Seeds start at 1101 + position; an entry whose seed
# put a hidden unit within 2^-18 of the ReLU kink, or whose float32 oracle missed half a bound (tests/test_hypernet_host.py),
# moved on in steps of 100: hl256_r15, t_over_h, w256_r65 (eight steps), c3_shape (two).
WG_SHAPES: List[WGShape] = [
    _wg("hl32_r17", (32, 32, 1, 16, 16, 17), 1101, fwd="mfma3", njt=2, r_rem16=1, r_tiles16=2, fused=True),
    _wg("hl64_r33", (48, 64, 2, 16, 16, 33), 1102, fwd="mfma3", njt=4, r_rem16=1, r_tiles16=3, r_rem32=1, fused=True),
    _wg("hl128_r16", (64, 128, 2, 32, 32, 16), 1103, fwd="mfma3", njt=8, r_rem16=0, r_tiles16=1, nsplit=4, fused=True),
    _wg("hl256_r15", (64, 256, 1, 16, 16, 15), 1204, fwd="mfma3", njt=16, r_rem16=15, r_tiles16=1, fused=True, nc_out=256,
        nc_hid=256),
    _wg("hl48_r31", (32, 48, 2, 8, 8, 31), 1105, fwd="mfma3", njt=0, r_rem16=15, r_tiles16=2, fused=True, nc_out=64),
    _wg("simple_odd", (24, 40, 1, 5, 7, 3), 1106, fwd="simple", hl16=8, n_mat_rem4=3, d_out_rem4=3, fused=True),
    _wg("simple_wide", (65, 100, 3, 12, 20, 18), 1107, fwd="simple", t_rem64=1, hh_rem8=4, r_rem8=2, fused=True,
        nc_out=128, nc_hid=128),
    _wg("depth7", (16, 16, 7, 16, 16, 9), 1108, fwd="mfma3", njt=0, fused=True, nc_hid=32),
    _wg("t_over_h", (200, 48, 2, 8, 8, 40), 1209, fwd="mfma3", njt=0, fused=True, t_over_h=True, nc_out=64, nc_hid=256,
        r_tiles32=2, r_rem32=8),
    _wg("w256_r65", (256, 256, 2, 16, 16, 65), 1810, fwd="mfma3", njt=16, fused=True, nc_out=256, nc_hid=256, r_tiles64=2,
        r_rem64=1, nsplit=1, last_range=256),
    _wg("one_rel", (129, 33, 1, 4, 4, 1), 1111, fwd="simple", hl16=1, t_rem64=1, hh_rem8=1, fused=True, nc_out=64,
        nc_hid=256),
    _wg("lds_limit", (1024, 1024, 1, 4, 4, 2), 1112, fwd="mfma3", njt=0, fused=False),
    _wg("depth0_simple", (100, 0, 0, 16, 16, 20), 1113, fwd="simple", Hl=100, hl16=4, fused=True, nc_out=128, nc_hid=128),
    _wg("depth0_mfma", (64, 0, 0, 16, 16, 20), 1114, fwd="mfma3", njt=4, Hl=64, fused=True, nc_out=64, nc_hid=64),
    _wg("tile_tail", (64, 128, 2, 16, 17, 64), 1115, fwd="mfma3", njt=8, mtiles=17, last_wg_waves=1, bias_rem16=1,
        fused=True, nsplit=2, last_range=16, r_rem64=0),
    _wg("range_plus1", (32, 64, 2, 1, 257, 5), 1116, fwd="mfma3", njt=4, fused=True, nsplit=2, nsplit_bias=2, last_range=1,
        last_range_bias=1),
    _wg("c3_shape", (64, 128, 2, 128, 128, 20), 1317, fwd="mfma3", njt=8, fused=True, nsplit=64, nsplit_bias=1),
    _wg("chain_wide", (1000, 520, 2, 8, 8, 5), 1118, fwd="simple", hl16=8, fused=False),
]
WG_BY_NAME = {c.name: c for c in WG_SHAPES}
WG_FUSED = [c for c in WG_SHAPES if weightgen_bwd_supported(c.T, c.Hh, c.nh)]
WG_DROPOUT_NAMES = ("hl64_r33", "t_over_h", "depth7", "simple_wide")
WG_BATCHED_NAMES = ("hl48_r31", "simple_odd", "hl256_r15")
DROPOUT_P = 0.25


def realised(case) -> Dict:
    """The route the launchers take for `case` (a WGShape or a LayoutShape); asserts everything the entry promises."""
    layout = getattr(case, "layout", NATURAL)
    got = derive(*case.shape, layout=layout)
    assert layout_supported(layout, case.d_in, case.d_out), f"{case.name}: layout {layout} does not take d = {case.d_in}"
    assert max(case.T, case.Hh) <= WG_MAX_WIDTH and 0 <= case.nh <= WG_MAX_HIDDEN, f"{case.name}: the forward rejects this"
    for key, want in case.promise:
        assert key in got, f"{case.name}: promises {key}, which this route does not have"
        assert got[key] == want, f"{case.name}: promises {key} = {want!r}, the launcher gives {got[key]!r}"
    return got


@dataclass(frozen=True)
class LayoutShape:
    name: str
    layout: int
    d: int
    R: int
    Hh: int
    promise: Tuple[Tuple[str, object], ...]
    seed: int
    T: int = 32
    nh: int = 1

    @property
    def d_in(self):
        return self.d

    @property
    def d_out(self):
        return self.d

    @property
    def dims(self):
        return (self.T, self.Hh, self.nh, self.d, self.d)

    @property
    def shape(self):
        return (self.T, self.Hh, self.nh, self.d, self.d, self.R)


SPLIT2H_D = (32, 64, 96, 128)
FRAG16_D = (16, 48, 64, 128, 256)
SPLIT2H_REJECTED_D = (48, 160)
FRAG16_REJECTED_D = (24,)


# seeds are 2000 + position, but for: a unit 2^-20.9 from the kink; a log-scale gradient that cancels to 2e-4 of its terms
_LAYOUT_SEEDS = {"frag16_d64_r17_h64": 2126, "split2h_d128_r17_h40": 2115}


def _layout_shapes() -> List[LayoutShape]:
    out = []
    for layout, lname, ds in ((SPLIT2H, "split2h", SPLIT2H_D), (FRAG16, "frag16", FRAG16_D)):
        for d in ds:
            for R in (1, 17):
                for Hh in (64, 40):
                    if layout == SPLIT2H:
                        promise = dict(fwd="mfma3" if Hh == 64 else "simple", pack=True)
                    else:
                        promise = dict(fwd="mfma_frag16" if Hh == 64 else "simple_frag16", pack=False)
                    name = f"{lname}_d{d}_r{R}_h{Hh}"
                    out.append(LayoutShape(name, layout, d, R, Hh, tuple(sorted(promise.items())),
                                           _LAYOUT_SEEDS.get(name, 2000 + len(out))))
    return out


LAYOUT_SHAPES: List[LayoutShape] = _layout_shapes()


# ---------------------------------------------------------------------------------------------------------------------
# generator inputs
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class WGInputs:
    x: np.ndarray                         # [R, T] float32
    state: Dict[str, np.ndarray]          # the reference's state_dict names (float32)
    flat: List[np.ndarray]                # [head][layer][weight, bias], as ghf_weightgen_fwd takes them
    ls: np.ndarray                        # [3] float32
    g: Dict[str, np.ndarray]              # dL / d out per head (float32)


def wg_params(T, Hh, nh, d_in, d_out, seed) -> Tuple[Dict[str, np.ndarray], List[np.ndarray], np.ndarray]:
    """Parameters of one generator: torch-like hidden layers (synth.weight_generator_params), the last layer's weights x 30,
    its biases N(0, 0.3), the three log-scales -0.5 / 0.25 / -1.0: outputs and gradients well off the 0.01 initialisation."""
    state = synth.weight_generator_params("", T, d_in, d_out, Hh, nh, seed)
    flat = []
    for head in HEADS:
        last = f"generators.{head}.{2 * nh}"
        state[last + ".weight"] = (state[last + ".weight"] * np.float32(LAST_GAIN)).astype(np.float32)
        state[last + ".bias"] = synth.normal(seed, last + ".bias", state[last + ".bias"].shape, std=LAST_BIAS_STD)
        state[f"log_scales.{head}"] = np.full((1,), LOG_SCALES[head], dtype=np.float32)
        for l in range(nh + 1):
            flat += [state[f"generators.{head}.{2 * l}.weight"], state[f"generators.{head}.{2 * l}.bias"]]
    ls = np.array([LOG_SCALES[h] for h in HEADS], dtype=np.float32)
    return state, flat, ls


@functools.lru_cache(maxsize=None)
def wg_inputs(case) -> WGInputs:
    state, flat, ls = wg_params(case.T, case.Hh, case.nh, case.d_in, case.d_out, case.seed)
    x = synth.normal(case.seed, "text_emb", (case.R, case.T))
    g = {"W_msg": synth.normal(case.seed, "gW_msg", (case.R, case.d_in, case.d_out)),
         "W_self": synth.normal(case.seed, "gW_self", (case.R, case.d_in, case.d_out)),
         "bias": synth.normal(case.seed, "gbias", (case.R, case.d_out))}
    return WGInputs(x, state, flat, ls, g)


def wg_masks(case, p: float) -> Tuple[np.ndarray, float]:
    """(dropout masks [3, nh, R, Hh] scaled by 1 / (1 - p), log_keep = log(1 / (1 - p))); p = 1: all zero, log_keep 0."""
    shape = (3, case.nh, case.R, case.Hh)
    if p >= 1.0:
        return np.zeros(shape, dtype=np.float32), 0.0
    keep = synth.uniform01(case.seed, "dropout", int(np.prod(shape))).reshape(shape) >= p
    return (keep.astype(np.float32) / np.float32(1.0 - p)).astype(np.float32), -math.log(1.0 - p)


# ---------------------------------------------------------------------------------------------------------------------
# the generator in float64: per-head loops, exp(log_scale) last, a hand-written backward
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class WGRef:
    out: Dict[str, np.ndarray]            # per head, float64, [R, d_in, d_out] / [R, d_out]
    pre: List[List[np.ndarray]]           # [head][layer] hidden pre-activations [R, Hh]
    mag: List[List[np.ndarray]]           # ... the sums of their terms' magnitudes
    grads: Optional[Dict[str, np.ndarray]]  # "text_emb", the state_dict names, "log_scales.<head>"


def wg_ref64(x, flat, ls, nh, d_in, d_out, masks=None, g=None) -> WGRef:
    """out_k = (a_k W_last^T + b_last) exp(ls_k), a_k = the head's last hidden activation: hidden layer l is
    relu(a W_l^T + b_l) (times the mask).  With g: every gradient of sum_k sum(out_k g_k)."""
    x = np.asarray(x, dtype=np.float64)
    R, nl = x.shape[0], nh + 1
    P = [np.asarray(p, dtype=np.float64) for p in flat]
    out, pre, mag = {}, [], []
    grads = None if g is None else {"text_emb": np.zeros_like(x)}
    for k, head in enumerate(HEADS):
        W = [P[(k * nl + l) * 2] for l in range(nl)]
        b = [P[(k * nl + l) * 2 + 1] for l in range(nl)]
        acts, zs, ms = [x], [], []
        for l in range(nh):
            a = acts[-1]
            z = np.empty((R, W[l].shape[0]))
            for r in range(R):                                     # one relation at a time: a matrix-vector product
                z[r] = W[l] @ a[r] + b[l]
            zs.append(z)
            ms.append(np.abs(a) @ np.abs(W[l]).T + np.abs(b[l]))
            h = np.where(z > 0.0, z, 0.0)
            acts.append(h if masks is None else h * np.asarray(masks[k][l], dtype=np.float64))
        y = acts[-1] @ W[nh].T + b[nh]
        scale = math.exp(float(ls[k]))
        shape = (R, d_in, d_out) if k < 2 else (R, d_out)
        out[head] = (y * scale).reshape(shape)
        pre.append(zs)
        mag.append(ms)
        if g is None:
            continue
        gk = np.asarray(g[head], dtype=np.float64).reshape(R, -1)
        grads[f"log_scales.{head}"] = np.array([np.sum(gk * y) * scale])
        dy = gk * scale
        grads[f"generators.{head}.{2 * nh}.weight"] = dy.T @ acts[-1]
        grads[f"generators.{head}.{2 * nh}.bias"] = dy.sum(axis=0)
        da = dy @ W[nh]
        for l in range(nh - 1, -1, -1):
            dz = np.where(zs[l] > 0.0, da, 0.0)
            if masks is not None:
                dz = dz * np.asarray(masks[k][l], dtype=np.float64)
            grads[f"generators.{head}.{2 * l}.weight"] = dz.T @ acts[l]
            grads[f"generators.{head}.{2 * l}.bias"] = dz.sum(axis=0)
            da = dz @ W[l]
        grads["text_emb"] += da
    return WGRef(out, pre, mag, grads)


@functools.lru_cache(maxsize=None)
def wg_reference(case, p: Optional[float] = None) -> WGRef:
    """wg_ref64 of a table entry (with dropout masks of probability p), computed once and shared; do not modify."""
    inp = wg_inputs(case)
    masks = None if p is None else wg_masks(case, p)[0]
    return wg_ref64(inp.x, inp.flat, inp.ls, case.nh, case.d_in, case.d_out, masks=masks, g=inp.g)


def active_pattern(ref: WGRef) -> Optional[np.ndarray]:
    """[3, nh, R, Hh] bool: which hidden units are active (before any dropout mask); None without hidden layers."""
    if not ref.pre[0]:
        return None
    return np.stack([np.stack([z > 0.0 for z in head]) for head in ref.pre])


# ---------------------------------------------------------------------------------------------------------------------
# packed weight layouts (include/ghf.h: GHF_WLAYOUT_FRAG16, GHF_WLAYOUT_SPLIT2H)
# ---------------------------------------------------------------------------------------------------------------------

def _stacked(Wm, Ws, transpose):
    """[W_top[r]; W_bottom[r]] as [R, 2d, d] float32: None = zeros, transpose = each [d, d] matrix transposed."""
    ref = Wm if Wm is not None else Ws
    halves = [np.zeros_like(ref) if w is None else (np.transpose(w, (0, 2, 1)) if transpose else w) for w in (Wm, Ws)]
    return np.ascontiguousarray(np.concatenate(halves, axis=1), dtype=np.float32)


def frag16_of(Wm, Ws, transpose=False):
    """Wfrag[r][o/16][kk/16][lane = ((kk%16)/4)*16 + o%16][kk%4], kk indexes the rows of [W_msg; W_self]."""
    cat = _stacked(Wm, Ws, transpose)
    R, d = cat.shape[0], cat.shape[2]
    cat = cat.reshape(R, 2 * d // 16, 4, 4, d // 16, 16)                                  # r, j, q, s, nt, c16
    return np.ascontiguousarray(cat.transpose(0, 4, 1, 2, 5, 3)).reshape(-1)             # r, nt, j, q, c16, s


def frag16_back(buf, R, d):
    """The [R, 2d, d] matrix a FRAG16 buffer holds."""
    f = np.asarray(buf).reshape(R, d // 16, 2 * d // 16, 4, 16, 4)                        # r, nt, j, q, c16, s
    return np.ascontiguousarray(f.transpose(0, 2, 3, 5, 1, 4)).reshape(R, 2 * d, d)      # kk = 16j + 4q + s ; o = 16nt + c16


def split2h_np(x, axis_groups):
    """SPLIT2H pieces of x: per group (all axes but the first `axis_groups`) s = 13 - floor(log2(max |x|)) clamped to
    +-100; hi = fp16(x 2^s), lo = fp16(x 2^s - hi).  Returns (hi, lo as float16, 2^-s as float32 per group)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    mx = np.abs(x).reshape(x.shape[:axis_groups] + (-1,)).max(axis=-1)
    e = ((mx.view(np.uint32) >> 23) & 255).astype(np.int32) - 127                        # exponent field, as the device
    sh = np.clip(13 - e, -100, 100)
    up = np.ldexp(np.float32(1), sh).astype(np.float32).reshape(sh.shape + (1,) * (x.ndim - axis_groups))
    xs = x * up
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi, lo, np.ldexp(np.float32(1), -sh).astype(np.float32)


def split2h_of(Wm, Ws, transpose=False):
    """Wh[r][o/16][kk/32][piece][lane = ((kk%32)/8)*16 + o%16][kk%8] fp16 + float 2^-s [R], as an opaque float32 buffer."""
    cat = _stacked(Wm, Ws, transpose)
    R, d = cat.shape[0], cat.shape[2]
    hi, lo, down = split2h_np(cat, 1)                                                     # [R, 2d, d]
    pc = np.stack([hi, lo]).reshape(2, R, 2 * d // 32, 4, 8, d // 16, 16)                 # piece, r, ks, q, e, ct, c16
    frag = np.ascontiguousarray(pc.transpose(1, 5, 2, 0, 3, 6, 4)).reshape(-1)            # r, ct, ks, piece, q, c16, e
    return np.concatenate([frag.view(np.float32), down])


def split2h_back(buf, R, d):
    """(hi, lo [R, 2d, d] float16, scales [R] float32) of a SPLIT2H buffer."""
    buf = np.ascontiguousarray(buf, dtype=np.float32)
    n = R * 2 * d * d
    pc = buf[:n].view(np.float16).reshape(R, d // 16, 2 * d // 32, 2, 4, 16, 8)          # r, ct, ks, piece, q, c16, e
    pc = np.ascontiguousarray(pc.transpose(3, 0, 2, 4, 6, 1, 5)).reshape(2, R, 2 * d, d)  # piece, r, (ks, q, e), (ct, c16)
    return pc[0], pc[1], buf[n:n + R].copy()


# ---------------------------------------------------------------------------------------------------------------------
# text encoder
# ---------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class TextShape:
    name: str
    U: int
    Lmax: int
    C: int
    T: int
    V: int
    craft: str = "random"     # how ids / lens are made (text_inputs)
    raw: bool = False         # holds ids or lengths only a raw call can pass (the tokeniser never makes them)
    seed: int = 0

    @property
    def shape(self):
        return (self.U, self.Lmax, self.C, self.T, self.V)


TEXT_SHAPES: List[TextShape] = [
    TextShape("c1", 3, 5, 1, 48, 128, seed=3101),
    TextShape("c33", 6, 12, 33, 48, 128, seed=3102),
    TextShape("c256_t1", 4, 9, 256, 1, 128, seed=3103),
    TextShape("c257", 4, 9, 257, 48, 128, seed=3104),
    TextShape("c1024_t300", 2, 7, 1024, 300, 128, seed=3105),
    TextShape("u300", 300, 6, 24, 48, 128, seed=3106),
    TextShape("u1", 1, 4, 24, 48, 128, seed=3107),
    TextShape("lmax1", 5, 1, 24, 48, 128, seed=3108),
    TextShape("long300", 3, 300, 24, 48, 128, craft="long", seed=3109),
    TextShape("twins", 4, 8, 24, 48, 128, craft="twins", seed=3110),
    TextShape("empties", 4, 3, 24, 48, 128, craft="empty", seed=3111),
    TextShape("small_vocab", 6, 8, 24, 48, 5, seed=3112),
    TextShape("unused_char", 9, 10, 24, 48, 16, craft="unused", seed=3113),
    TextShape("raw_ids", 5, 6, 24, 48, 128, craft="raw_ids", raw=True, seed=3114),
    TextShape("raw_lens", 6, 5, 24, 48, 128, craft="raw_lens", raw=True, seed=3115),
]
UNUSED_CHAR = 11


@dataclass
class TextInputs:
    ids: np.ndarray       # [U, Lmax] int32, zero-padded past each length as the tokeniser pads
    lens: np.ndarray      # [U] int32
    E: np.ndarray         # [V, C]
    W: np.ndarray         # [T, C]
    b: np.ndarray         # [T]
    dte: np.ndarray       # [U, T]


@functools.lru_cache(maxsize=None)
def text_inputs(case: TextShape) -> TextInputs:
    U, Lmax, C, T, V = case.shape
    s = case.seed
    ids = synth.randint(s, "ids", U * Lmax, V).reshape(U, Lmax).astype(np.int32)
    lens = (1 + synth.randint(s, "lens", U, Lmax)).astype(np.int32)
    lens[0] = Lmax                                             # one string fills the matrix
    if case.craft == "long":
        ids[0], lens[0] = 65, Lmax                             # 300 equal characters
        lens[1] = 1
    elif case.craft == "twins":
        ids[2], lens[2] = ids[1], lens[1]
    elif case.craft == "empty":
        ids[:], lens[:] = 0, 0                                 # '' -> padded row of zeros, length 0 (read as [0])
    elif case.craft == "unused":
        ids[ids == UNUSED_CHAR] = UNUSED_CHAR + 1
    elif case.craft == "raw_ids":
        ids[0, 0], ids[1, 1], ids[2, 0], ids[2, 1] = -3, V + 5, V + 5, -3
        lens[1] = max(int(lens[1]), 2)
        lens[2] = max(int(lens[2]), 2)
    elif case.craft == "raw_lens":
        lens[1], lens[2], lens[3] = 0, -1, Lmax + 4
    if not case.raw:
        for u in range(U):
            ids[u, max(int(lens[u]), 0):] = 0
    bound = 1.0 / math.sqrt(C)
    return TextInputs(ids, lens, synth.normal(s, "char_emb", (V, C)), synth.uniform(s, "te.w", (T, C), bound),
                      synth.uniform(s, "te.b", (T,), bound), synth.normal(s, "dte", (U, T)))


def effective_ids(ids, lens, V) -> List[np.ndarray]:
    """The characters every string is read as: ids clamped to [0, V-1]; len <= 0 -> 1; len > Lmax -> Lmax."""
    ids = np.asarray(ids)
    out = []
    for u in range(ids.shape[0]):
        n = int(lens[u])
        n = 1 if n <= 0 else min(n, ids.shape[1])
        out.append(np.clip(ids[u, :n].astype(np.int64), 0, V - 1))
    return out


def text_ref64(ids, lens, E, W, b, dte=None):
    """te = tanh(mean_l E[id_l] W^T + b) per string, in float64; with dte: (te, dE, dW, db) for loss = sum(te dte)."""
    E, W, b = (np.asarray(a, dtype=np.float64) for a in (E, W, b))
    eff = effective_ids(ids, lens, E.shape[0])
    U, T = len(eff), W.shape[0]
    pooled = np.empty((U, E.shape[1]))
    for u, row in enumerate(eff):
        acc = np.zeros(E.shape[1])
        for c in row:                                          # one character at a time
            acc += E[c]
        pooled[u] = acc / len(row)
    te = np.tanh(pooled @ W.T + b)
    if dte is None:
        return te
    dpre = np.asarray(dte, dtype=np.float64) * (1.0 - te * te)
    dW, db = dpre.T @ pooled, dpre.sum(axis=0)
    dpooled = dpre @ W
    dE = np.zeros_like(E)
    for u, row in enumerate(eff):
        for c in row:
            dE[c] += dpooled[u] / len(row)
    return te, dE, dW, db


@functools.lru_cache(maxsize=None)
def text_reference(case: TextShape):
    """text_ref64 of a table entry with its gradients, computed once and shared; do not modify."""
    inp = text_inputs(case)
    return text_ref64(inp.ids, inp.lens, inp.E, inp.W, inp.b, inp.dte)


def used_chars(case: TextShape) -> np.ndarray:
    inp = text_inputs(case)
    used = np.zeros(case.V, dtype=bool)
    for row in effective_ids(inp.ids, inp.lens, case.V):
        used[row] = True
    return used


# ghf_weights_pack: (layout, d) x transpose x which halves are given, R = 3
PACK_R = 3
PACK_SHAPES = [(FRAG16, d) for d in (16, 64, 256)] + [(SPLIT2H, d) for d in (32, 96, 128)]
PACK_HALVES = ((True, True), (False, True), (True, False))     # (top given, bottom given)


def pack_inputs(d: int) -> Tuple[np.ndarray, np.ndarray]:
    return (synth.normal(4000 + d, "pack_top", (PACK_R, d, d), std=0.15),
            synth.normal(4000 + d, "pack_bottom", (PACK_R, d, d), std=0.4))
