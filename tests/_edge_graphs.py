"""Crafted edge-case graphs for the message kernels: the case catalogue, a float64 reference of the layer and a numpy
restatement of the plan's cut that checks every case really has the structure its name promises.

Not collected by pytest (test_edge_graphs_host.py and test_edge_graphs_gpu.py import it).  Every case is built from the
geometry handed in — (block_nodes, chunk_rows, split_chunks) of the kernel's plan and the rows-per-helper-wave of the bx
kernels — so a retuned kernel gets the cases of its new geometry, and `realised` fails when a case no longer is what it
claims (a block "at exactly split_chunks + 1 chunks" that has another count).

The graphs stay within 3 * block_nodes + 1 nodes, except the hub cases and the two graphs that line up blocks with 0..7
chunks in one launch (eight blocks).

The CSR catalogue is instantiated at every width of the relation-stationary layer (RS_WIDTHS).  For those widths the file
also restates the range guard's rule on the rows that layer cuts (cut_rows_margin: what the guard word must be after a
forward and after a backward) and the two-layer chain of test_wide_rows_gpu.py.

The same catalogue, less its hub case, runs the any-width route (message_generic_kernel) at the widths of ANY_FWD_WIDTHS:
test_any_width_host.py and test_any_width_gpu.py take their width tables and the kernels' thread geometry from here."""

from __future__ import annotations

from typing import List, NamedTuple, Tuple

import numpy as np
import torch

from graph_hypernetwork_forge_amd import synth

LN_EPS = 1e-5


class Case(NamedTuple):
    name: str
    N: int
    edge_index: np.ndarray      # [2, E] int64
    rel: np.ndarray             # [E] int64, never R - 1
    R: int
    expects: tuple              # conditions `realised` asserts, (tag, *args) each


# (geometry key, case name) -> seed of the layer inputs, where the default seed makes the case ill-conditioned (a LayerNorm
# row with next to no variance, a ReLU kink): test_edge_graphs_host.py checks that the seed named here is admissible
SEED = 7100
SEED_OVERRIDES: dict = {("bx128", "split_exactly_sc_chunks"): 7103, ("bx128", "split_sc_plus_1_chunks"): 7104,
                        ("csr512", "csr_hubs_around_hub_rows"): 7103, ("csr640", "csr_hubs_around_hub_rows"): 7105,
                        ("csr768", "csr_hubs_around_hub_rows"): 7102, ("csr896", "csr_hubs_around_hub_rows"): 7102,
                        ("csr1024", "csr_hubs_around_hub_rows"): 7101}
RS_WIDTHS = (128, 256, 384, 512, 640, 768, 896, 1024)       # every width ghf_message_rs_supported accepts

# ---- the any-width route (test_any_width_host.py / test_any_width_gpu.py) ---------------------------------------------
# message_generic_kernel and tail_kernel (csrc/message_generic.hip): GEN_TPB threads, thread t holds column t + GEN_TPB c for
# c < GEN_MAX_D / GEN_TPB, block_sum over GEN_TPB / 64 waves.  The widths: one live wave (1, 2, 3, 63), a second wave with one
# live lane (65), part-filled waves (100, 192, 255), a last column group with exactly one live thread (257, 513, 769), every
# column group with a dead last thread (1023).  Seeds of these widths' cases are recorded under the key f"any{d}".
GEN_TPB, GEN_MAX_D, WAVE = 256, 1024, 64
ANY_FWD_WIDTHS = (1, 2, 3, 63, 65, 100, 192, 255, 257, 513, 769, 1023)
ANY_BWD_WIDTHS = (3, 65, 100, 257, 513, 1023)             # (LayerNorm over one or two values has no well-conditioned gradient)
ANY_NO_HUBS = "csr_hubs_around_hub_rows"                  # cut around a threshold of the relation-stationary layer: not run here
SEED_OVERRIDES.update({("any3", "csr_n1_self_loop"): 7101})

# the fp32 input projection (csrc/input_proj.hip): input_proj_mfma_kernel<NT> at d = 16 NT, column tiles in groups of TG;
# W_in staged in LDS (WLDS) when cdiv(N, IP_ROWS_PER_BLOCK) >= IP_WLDS_MIN_BLOCKS and d (F + 4) 4 <= IP_WLDS_MAX_BYTES
IP_NT = tuple(range(1, 17))
IP_F = (16, 48, 80)
IP_N = (77, 8200)
IP_ROWS_PER_BLOCK, IP_WLDS_MIN_BLOCKS, IP_WLDS_MAX_BYTES = 128, 64, 72 * 1024
IP_SIMPLE = ((10, 72), (16, 200), (48, 320), (7, 1023))    # (F, d) of the vector-ALU fallback: F % 16, d % 16 or d > 256
MODEL_WIDTHS = (72, 96, 200)                               # the whole model: d % 16 != 0; MFMA projection at NT = 6; neither


def any_width_cases(seed: int = 7100) -> List["Case"]:
    """The CSR catalogue without the hub case, in the catalogue's order."""
    return [c for c in _csr_cases(seed) if c.name != ANY_NO_HUBS]


def dropout_mask(N: int, d: int, seed: int = 78) -> np.ndarray:
    """A layer's dropout mask at p = 0.25, scaled by 1 / (1 - p): [N, d] float32, the same on every machine."""
    return ((synth.uniform01(seed, "drop", N * d) < 0.75) / 0.75).astype(np.float32).reshape(N, d)


def tail_ref64(agg, h, gamma, beta, drop=None, eps: float = 1e-5) -> np.ndarray:
    """LayerNorm(ReLU(agg + h) * drop) in numpy float64 (biased variance)."""
    agg, h, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (agg, h, gamma, beta))
    x = np.maximum(agg + h, 0.0) * (1.0 if drop is None else np.asarray(drop, dtype=np.float64))
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * gamma + beta


def generic_geometry(d: int) -> dict:
    """How message_generic_kernel's 256 threads cover d columns: live waves (waves with a column in group 0), column groups
    used, live threads of the last group."""
    assert 1 <= d <= GEN_MAX_D
    groups = -(-d // GEN_TPB)
    return dict(live_waves=-(-min(d, GEN_TPB) // WAVE), groups=groups, last_group_threads=d - GEN_TPB * (groups - 1))


def ip_tile_group(NT: int) -> int:
    """TG of input_proj_mfma_kernel<NT>: column tiles whose MFMAs are interleaved."""
    return 4 if NT % 4 == 0 else (2 if NT % 2 == 0 else 1)


def ip_route(N: int, F: int, d: int) -> str:
    """The kernel launch_input_proj picks for 16-byte aligned operands and no h_split below N = 1024: "mfma_wlds", "mfma"
    (W_in's fragments from L2) or "simple" (the vector ALU)."""
    if F % 16 or d % 16 or d > 256:
        return "simple"
    wlds = d * (F + 4) * 4 <= IP_WLDS_MAX_BYTES and -(-N // IP_ROWS_PER_BLOCK) >= IP_WLDS_MIN_BLOCKS
    return "mfma_wlds" if wlds else "mfma"


def seed_for(geometry: str, name: str) -> int:
    return SEED_OVERRIDES.get((geometry, name), SEED)


def geometries():
    """[(key, d, block_nodes, chunk_rows, split_chunks, rows per helper wave)]: the plans of the tuned kernels and the CSR
    plan at every width that runs on it (the relation-stationary layer's eight widths; the generic kernel at 20).  Needs the
    library, no GPU."""
    from graph_hypernetwork_forge_amd import _native
    from graph_hypernetwork_forge_amd.plan import CSR_CONFIG
    bx128, bx64, pp128, pp64 = (_native.message_config(128), _native.message_config(64), _native.message_config(128, "pp"),
                                _native.exact_config(64))
    out = [("bx128", 128, bx128, bx128[0] // 4), ("bx64", 64, bx64, bx64[0] // 4), ("pp128", 128, pp128, 0), ("pp64", 64, pp64, 0),
           ("csr256", 256, CSR_CONFIG, 0), ("csr20", 20, CSR_CONFIG, 0)]
    out += [(f"csr{d}", d, CSR_CONFIG, 0) for d in RS_WIDTHS if d != 256]
    return [(k, d, c[0], c[2], c[3], npw) for k, d, c, npw in out]


# ---- building blocks ---------------------------------------------------------------------------------------------------

class _G:
    """Edges collected group by group; sources default to seeded-random nodes."""

    def __init__(self, name: str, N: int, R: int, seed: int) -> None:
        self.name, self.N, self.R, self.seed = name, N, R, seed
        self.s, self.d, self.r = [], [], []

    def add(self, dst, rel, src=None) -> None:
        dst = np.atleast_1d(np.asarray(dst, dtype=np.int64))
        n = dst.size
        rel = np.broadcast_to(np.asarray(rel, dtype=np.int64), (n,))
        if src is None:
            src = synth.randint(self.seed, f"{self.name}/src{len(self.s)}", n, self.N)
        src = np.broadcast_to(np.asarray(src, dtype=np.int64), (n,))
        assert dst.min() >= 0 and dst.max() < self.N and src.min() >= 0 and src.max() < self.N
        assert rel.min() >= 0 and rel.max() < self.R - 1, "relation R - 1 stays without edges"
        self.s.append(src), self.d.append(dst), self.r.append(rel)

    def case(self, *expects) -> Case:
        s, d, r = (np.concatenate(a) for a in (self.s, self.d, self.r))
        order = np.argsort(synth.raw_u64(self.seed, self.name + "/order", s.size), kind="stable")   # callers' lists are not sorted
        return Case(self.name, self.N, np.stack([s[order], d[order]]), r[order].copy(), self.R, tuple(expects))


def _ordinary(g: _G, block: int, bn: int, n: int = 30, rels: int = 1) -> None:
    """An ordinary block beside the odd one: n random in-edges."""
    lo, hi = block * bn, min((block + 1) * bn, g.N)
    dst = lo + synth.randint(g.seed, f"{g.name}/ord{block}", n, hi - lo)
    g.add(dst, synth.randint(g.seed, f"{g.name}/ordr{block}", n, rels))


def edge_cases(bn: int, cr: int, sc: int, npw: int, d: int, seed: int = SEED) -> List[Case]:
    """Named cases (name, N, edge_index, rel, R, expects) for a plan of `bn` destination rows per block, chunks of `cr` rows,
    blocks split above `sc` chunks and `npw` rows per helper wave (0: the kernel has none); bn == 1: the CSR catalogue.
    `d` is the hidden size the cases will run at (kept for the record: the graphs do not depend on it)."""
    return _csr_cases(seed) if bn == 1 else _block_cases(bn, cr, sc, npw, seed)


def _block_cases(bn: int, cr: int, sc: int, npw: int, seed: int) -> List[Case]:
    out: List[Case] = []

    # ---- sizes
    for label, N in (("bn_minus_1", bn - 1), ("bn", bn), ("bn_plus_1", bn + 1), ("2bn_plus_1", 2 * bn + 1)):
        g = _G(f"size_{label}_one_edge_per_block", N, 2, seed)
        nb = -(-N // bn)
        for b in range(nb):
            g.add([min(b * bn + 3, N - 1)], 0)
        out.append(g.case(("N", N), ("blocks", nb), *[("block_chunks", b, 1) for b in range(nb)]))
    g = _G("size_middle_block_without_in_edges", 3 * bn, 3, seed)
    _ordinary(g, 0, bn, rels=2)
    _ordinary(g, 2, bn, rels=2)
    out.append(g.case(("block_chunks", 1, 0), ("blocks", 3)))
    g = _G("size_only_last_node_has_in_edges", 2 * bn + 1, 3, seed)
    g.add(np.full(9, 2 * bn), [0, 0, 0, 0, 1, 1, 1, 1, 1])
    out.append(g.case(("only_dst", 2 * bn), ("block_chunks", 0, 0), ("block_chunks", 1, 0), ("block_chunks", 2, 2)))

    # ---- chunks per block: 0..7 in one graph, in that order and reversed (one relation with one edge = one chunk)
    for label, counts in (("0_to_7", list(range(8))), ("7_to_0", list(range(7, -1, -1)))):
        g = _G(f"chunks_per_block_{label}", 8 * bn, 8, seed)
        for b, k in enumerate(counts):
            for r in range(k):
                g.add([b * bn + (11 * r + b) % bn], r)
        out.append(g.case(*[("block_chunks", b, k) for b, k in enumerate(counts)]))

    # ---- chunk lengths: one (block, relation) group of each size
    sizes = sorted({n for n in (1, 15, 16, 17, 63, 64, 65, cr - 1, cr, cr + 1, 2 * cr, 2 * cr + 1) if n >= 1})
    g = _G("chunk_lengths", 3 * bn, len(sizes) + 1, seed)
    for i, n in enumerate(sizes):
        g.add((i % 3) * bn + (7 * i + np.arange(n)) % bn, i)          # distinct destinations where bn allows
    lens = sorted({m for n in sizes for m in ([cr] * (n // cr) + ([n % cr] if n % cr else []))})
    out.append(g.case(*[("group", n) for n in sizes], *[("chunk_len", m) for m in lens]))

    # ---- runs of equal destination inside one group
    g = _G("runs", 2 * bn, 12, seed)
    r = 0
    for L in (2, 15, 16, 17, 33):
        base = (r % 2) * bn
        g.add(base + np.concatenate([np.arange(5), np.full(L, 10), np.arange(20, 23)]), r)
        r += 1
    g.add(bn + np.concatenate([np.arange(15), np.full(2, 15), np.arange(16, 21)]), r)      # rows 15 and 16: tile 0's last, tile 1's first
    r += 1
    g.add(np.full(cr, 40), r)                                                              # the whole chunk is one destination
    r += 1
    g.add(bn + np.concatenate([np.arange(3), np.full(cr + 5, 50), np.arange(60, 62)]), r)   # a run over the chunk boundary
    r += 1
    g.add(np.concatenate([np.full(40, 70), np.arange(80, 84)]), r, np.concatenate([np.full(40, 9), np.arange(4)]))
    r += 1
    g.add(bn + np.concatenate([np.full(20, 90), np.arange(100, 103)]), r, np.concatenate([np.full(20, bn + 90), np.arange(3)]))
    out.append(g.case(("run", 2), ("run", 15), ("run", 16), ("run", 17), ("run", 33), ("run_at", 15, 2), ("chunk_one_dst", cr),
                      ("run_spans_chunks", cr + 5), ("dup", 40), ("self_loop", 20)))

    # ---- helper-wave boundaries (bx): local node v belongs to wave v // npw
    if npw > 0:
        g = _G("helper_wave_boundaries", 2 * bn, 5, seed)
        exp = [("wave_only", 3), ("locals", (0, npw - 1, npw, 2 * npw - 1, 2 * npw, bn - 1))]
        g.add(3 * npw + 2 * np.arange(10), 0)
        g.add(bn + np.array([0, npw - 1, npw, 2 * npw - 1, 2 * npw, bn - 1]), 1)
        if cr > 64 and npw >= 64:
            g.add(np.concatenate([np.arange(64), npw + np.arange(cr - 64)]), 2)
            exp.append(("wave_rows", 1, 64, cr - 1))
        if cr >= 68 and npw >= 62:
            g.add(bn + np.concatenate([np.arange(62), npw + np.arange(5), 2 * npw + np.arange(cr - 67)]), 3)
            exp.append(("wave_rows", 1, 62, 66))
        out.append(g.case(*exp))

    # ---- split blocks, each beside an ordinary block
    g = _G("split_exactly_sc_chunks", 2 * bn, 3, seed)
    g.add(np.full(sc * cr, 5), 0)
    _ordinary(g, 1, bn, rels=2)
    out.append(g.case(("block_chunks", 0, sc), ("items", 0, 1), ("indeg", sc * cr)))
    g = _G("split_sc_plus_1_chunks", 2 * bn, 3, seed)
    g.add(np.full((sc + 1) * cr, 5), 0)
    _ordinary(g, 1, bn, rels=2)
    out.append(g.case(("block_chunks", 0, sc + 1), ("items", 0, 2), ("indeg", (sc + 1) * cr)))
    g = _G("split_2sc_plus_1_chunks_three_relations", 2 * bn, 4, seed)
    per = [(2 * sc + 1 + 2 - i) // 3 for i in range(3)]
    for i, k in enumerate(per):
        g.add(bn + synth.randint(seed, f"split3/{i}", k * cr, bn), i)
    _ordinary(g, 0, bn, rels=2)
    out.append(g.case(("block_chunks", 1, 2 * sc + 1), ("items", 1, 3), ("items", 0, 1)))

    # ---- sources
    g = _G("sources_one_row_per_chunk", 2 * bn, 3, seed)
    g.add(np.arange(30), 0, 3)
    g.add(bn + 2 * np.arange(40), 1, 2 * bn - 1)
    _ordinary(g, 1, bn)
    out.append(g.case(("chunk_same_src", 30), ("chunk_same_src", 40)))
    g = _G("sources_all_last_node", 2 * bn, 3, seed)
    g.add(synth.randint(seed, "srclast/dst", 50, 2 * bn), synth.randint(seed, "srclast/rel", 50, 2), 2 * bn - 1)
    out.append(g.case(("all_src", 2 * bn - 1)))
    g = _G("sources_hub_with_sc_plus_1_chunks_of_out_edges", 2 * bn, 3, seed)
    g.add(np.arange((sc + 1) * cr) % (2 * bn), 0, 7)
    _ordinary(g, 0, bn, rels=2)
    out.append(g.case(("outdeg", 7, (sc + 1) * cr)))

    # ---- relations
    g = _G("relations_r2_all_in_relation_0", bn + 1, 2, seed)
    g.add(synth.randint(seed, "r2/dst", 40, bn + 1), 0)
    out.append(g.case(("R", 2), ("blocks", 2)))
    g = _G("relations_r64_one_edge_each", bn + 1, 64, seed)
    g.add((5 * np.arange(63)) % bn, np.arange(63))
    out.append(g.case(("R", 64), ("block_chunks", 0, 63), ("block_chunks", 1, 0)))

    # ---- the smallest graphs (last: the oddest launches of the catalogue)
    g = _G("size_n1_self_loop", 1, 2, seed)
    g.add([0], 0, [0])
    out.append(g.case(("N", 1), ("self_loop", 1), ("block_chunks", 0, 1)))
    g = _G("size_n2_one_edge", 2, 2, seed)
    g.add([1], 0, [0])
    out.append(g.case(("N", 2), ("edges", 1)))
    return out


def _csr_cases(seed: int) -> List[Case]:
    from graph_hypernetwork_forge_amd.plan import RS_HUB_ROWS, RS_RUN_MAX, RS_TILE
    out: List[Case] = []
    degs = (0, 1, 2, 63, 64, 65, 300)
    g = _G("csr_in_degrees", 40, 4, seed)
    for i, k in enumerate(degs):
        if k:
            g.add(np.full(k, 3 * i + 1), synth.randint(seed, f"deg/{k}", k, 3))
    out.append(g.case(*[("indeg", k) for k in degs]))
    counts = (1, RS_TILE - 1, RS_TILE, RS_TILE + 1, 2 * RS_TILE + 1)
    g = _G("csr_relation_sizes_around_the_tile", 150, len(counts) + 1, seed)
    for r, k in enumerate(counts):
        g.add(synth.randint(seed, f"relsz/{r}", k, 150), r)
    out.append(g.case(*[("rel_edges", k) for k in counts]))
    g = _G("csr_runs_around_run_max", 60, 4, seed)
    for i, k in enumerate((RS_RUN_MAX - 1, RS_RUN_MAX, RS_RUN_MAX + 1)):
        g.add(np.full(k, 10 * i + 2), i)
        g.add(np.full(3, 10 * i + 2), (i + 1) % 3)
    out.append(g.case(*[("dst_rel_run", k) for k in (RS_RUN_MAX - 1, RS_RUN_MAX, RS_RUN_MAX + 1)]))
    g = _G("csr_hubs_around_hub_rows", 500, 5, seed)
    for i, k in enumerate((RS_HUB_ROWS - 1, RS_HUB_ROWS, RS_HUB_ROWS + 1)):
        g.add(np.full(k, 100 * i + 17), synth.randint(seed, f"hub/{i}", k, 4))
    g.add(synth.randint(seed, "hub/rest", 200, 500), synth.randint(seed, "hub/restr", 200, 4))
    out.append(g.case(("indeg_at_least", RS_HUB_ROWS - 1), ("indeg_at_least", RS_HUB_ROWS), ("indeg_at_least", RS_HUB_ROWS + 1)))
    g = _G("csr_duplicates_and_self_loops", 30, 3, seed)
    g.add(np.full(40, 4), 0, 9)
    g.add(np.full(20, 11), 1, 11)
    g.add(synth.randint(seed, "dups/dst", 25, 30), synth.randint(seed, "dups/rel", 25, 2))
    out.append(g.case(("dup", 40), ("self_loop", 20)))
    g = _G("csr_n1_self_loop", 1, 2, seed)
    g.add([0], 0, [0])
    out.append(g.case(("N", 1), ("self_loop", 1)))
    g = _G("csr_n2_one_edge", 2, 2, seed)
    g.add([1], 0, [0])
    out.append(g.case(("N", 2), ("edges", 1)))
    return out


# ---- the layer in float64 ----------------------------------------------------------------------------------------------

def layer_inputs(case: Case, d: int, seed: int):
    """(h, W_msg, W_self, bias, gamma, beta) float32, at the scales of test_hip_parity._layer_inputs up to d = 256.  Beyond,
    the weights are scaled by sqrt(256 / d): at a fixed std the aggregate grows like sqrt(2 d) and its absolute error with
    it, and the float32 oracle itself leaves half of assert_close's bounds (test_edge_graphs_host.py); scaled, the
    aggregate keeps the magnitude it has at 256 and the same bounds hold at every width."""
    N, R = case.N, case.R
    h = synth.normal(seed, "h", (N, d))
    Wm = synth.normal(seed, "Wm", (R, d, d), std=0.15)
    Ws = synth.normal(seed, "Ws", (R, d, d), std=0.15)
    if d > 256:
        Wm, Ws = (W * np.float32(np.sqrt(256.0 / d)) for W in (Wm, Ws))
    b = synth.normal(seed, "b", (R, d), std=0.3)
    gamma = (1.0 + 0.2 * synth.normal(seed, "g", (d,))).astype(np.float32)
    beta = (0.2 * synth.normal(seed, "bt", (d,))).astype(np.float32)
    return h, Wm, Ws, b, gamma, beta


def layer_ref64(h, edge_index, rel, W_msg, W_self, bias, gamma, beta, eps: float = LN_EPS):
    """(out, h') in plain numpy float64:
    out_v = (1 / max(indeg_v, 1)) * sum_e (h_u W_msg[r] + b[r] + h_v W_self[r]),  h' = LayerNorm(ReLU(out + h)).
    The sources of a (destination, relation) pair are summed before they meet the weights — another order of operations
    than the oracle's per-edge products."""
    h, W_msg, W_self, bias, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (h, W_msg, W_self, bias, gamma, beta))
    src, dst = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    rel = np.asarray(rel, dtype=np.int64)
    N = h.shape[0]
    acc = np.zeros_like(h)
    for r in np.unique(rel):
        e = np.nonzero(rel == r)[0]
        rows, inv = np.unique(dst[e], return_inverse=True)
        X = np.zeros((rows.size, h.shape[1]))
        np.add.at(X, inv, h[src[e]])
        cnt = np.bincount(inv, minlength=rows.size).astype(np.float64)[:, None]
        acc[rows] += X @ W_msg[r] + cnt * (bias[r] + h[rows] @ W_self[r])
    out = acc / np.maximum(np.bincount(dst, minlength=N), 1).astype(np.float64)[:, None]
    x = np.maximum(out + h, 0.0)
    mu = x.mean(axis=1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    return out, (x - mu) / np.sqrt(var + eps) * gamma + beta


RANGE_ROWS = 1                                             # include/ghf.h: GHF_RANGE_ROWS
RS_TRAIN_WIDTHS = (256, 384, 512, 768, 1024)               # widths whose per-edge route test_edge_graphs_gpu.py differentiates


def cut_rows_margin(case: Case, h, agg, gamma, gout, eps: float = LN_EPS) -> dict:
    """How close the rows the relation-stationary layer cuts into fp16 pieces come to raising GHF_RANGE_ROWS (csrc/common.h:
    the bit is raised when tiny > 0 and tiny * 8 >= nonzero): the largest tiny * 8 / nonzero over
        "forward"   the rows of h and the sums of every (destination, relation) run's source rows (pass 0 of a run plan),
        "backward"  the rows the two gradient passes gather, G_v = dpre_v / max(indeg_v, 1) — dpre the gradient at the
                    aggregate, from `gout` at h' through LayerNorm and ReLU in float64 — and the run sums of G on the plan and
                    on the reversed plan, each where build_rs(runs=None) chooses a run plan (rows <= RS_RUNS_MAX_SHARE * E).
    Runs are cut into rows of RS_RUN_MAX edges in the stable order of the case's edge list (the plan's own order inside a
    run may differ: that moves which sources share a row of a run longer than RS_RUN_MAX, not what kind of rows they are).
    The backward of a graph with hubs is NOT of ordinary range by itself: on the reversed plan a run that mixes a hub's row
    of G (divided by thousands) with a leaf's has the hub's entries 2^-12 down wherever the ReLU masks the leaf's — the
    guard's rule is met or missed by a few entries, and `predicted_range_word` says which."""
    from _rows_cases import guard_counts
    from graph_hypernetwork_forge_amd.plan import RS_RUN_MAX, RS_RUNS_MAX_SHARE
    h64, agg, gamma, g = (np.asarray(a, dtype=np.float64) for a in (h, agg, gamma, gout))
    src, dst, rel = case.edge_index[0], case.edge_index[1], case.rel
    pre = agg + h64
    x = np.maximum(pre, 0.0)
    mu = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(axis=1, keepdims=True) + eps)
    xhat, dxh = (x - mu) * rstd, g * gamma
    dx = rstd * (dxh - dxh.mean(axis=1, keepdims=True) - xhat * (dxh * xhat).mean(axis=1, keepdims=True))
    Gm = (dx * (pre > 0) / np.maximum(np.bincount(dst, minlength=case.N), 1)[:, None]).astype(np.float32)

    def worst(rows):
        out = 0.0
        for row in rows:
            tiny, nz = guard_counts(row)
            out = max(out, tiny * 8 / nz if nz else 0.0)
        return out

    def run_rows(to, frm):
        """(the source lists of the rows of two or more edges, rows in all) of the run plan keyed by (`to`, relation)."""
        key = to * case.R + rel
        order = np.argsort(key, kind="stable")
        ks, ss = key[order], frm[order]
        heads = np.nonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))[0].tolist() + [ks.size]
        rows = [ss[a:min(a + RS_RUN_MAX, q)] for p, q in zip(heads[:-1], heads[1:]) for a in range(p, q, RS_RUN_MAX)]
        return [r for r in rows if r.size > 1], len(rows)

    def sums(X, rows):
        return (X[r].sum(axis=0, dtype=np.float32) for r in rows)

    h32 = np.asarray(h, dtype=np.float32)
    fwd_rows, n_fwd = run_rows(dst, src)
    rev_rows, n_rev = run_rows(src, dst)
    E = rel.size
    bwd = [worst(Gm)]
    bwd += [worst(sums(Gm, fwd_rows))] if n_fwd <= RS_RUNS_MAX_SHARE * E else []
    bwd += [worst(sums(Gm, rev_rows))] if n_rev <= RS_RUNS_MAX_SHARE * E else []
    return {"forward": max(worst(h32), worst(sums(h32, fwd_rows))), "backward": max(bwd)}


def predicted_range_word(margin: float) -> int:
    """The guard word a pass leaves whose rows reach `margin` of the rule (cut_rows_margin): it fires from 1 on.  Within 0.03
    of 1 the prediction is not made: the kernels' fp32 rows differ from the restatement's in their last bits, which can move
    a handful of entries standing at the "tiny" threshold — 3 % of a row's nonzero entries (ten and more from d = 384) is
    far more than that.  test_edge_graphs_host.py keeps every differentiated case outside the band."""
    assert abs(margin - 1.0) > 0.03, f"margin {margin:.3f}: too close to the guard's rule to call"
    return RANGE_ROWS if margin >= 1.0 else 0


def two_layer_inputs(case: Case, d: int, seed: int):
    """(layer 1: h, W_msg, W_self, bias, gamma, beta; layer 2: W_msg, W_self, bias, gamma, beta) for two layers on one graph:
    layer 2's parameters are layer_inputs' of another seed."""
    return layer_inputs(case, d, seed), layer_inputs(case, d, seed + 1000)[1:]


def two_layer_ref64(case: Case, ins1, ins2) -> np.ndarray:
    """h'' of two layers (layer_ref64 twice) in float64."""
    _, h1 = layer_ref64(ins1[0], case.edge_index, case.rel, *ins1[1:])
    return layer_ref64(h1, case.edge_index, case.rel, *ins2)[1]


def layer_ref64_torch(h, edge_index, rel, W_msg, W_self, bias, gamma, beta, eps: float = LN_EPS):
    """layer_ref64 on float64 torch tensors (for autograd); returns (out, h')."""
    src, dst = edge_index[0], edge_index[1]
    N, d = h.shape
    acc = torch.zeros(N, d, dtype=torch.float64)
    for r in torch.unique(rel).tolist():
        e = torch.nonzero(rel == r).flatten()
        X = torch.zeros(N, d, dtype=torch.float64).index_add(0, dst[e], h[src[e]])
        cnt = torch.bincount(dst[e], minlength=N).to(torch.float64).unsqueeze(1)
        rows = torch.nonzero(cnt.flatten() > 0).flatten()
        acc = acc.index_add(0, rows, X[rows] @ W_msg[r] + cnt[rows] * (bias[r] + h[rows] @ W_self[r]))
    out = acc / torch.bincount(dst, minlength=N).clamp(min=1).to(torch.float64).unsqueeze(1)
    x = torch.relu(out + h)
    mu = x.mean(dim=1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=1, keepdim=True)
    return out, (x - mu) / torch.sqrt(var + eps) * gamma + beta


# ---- the plan's cut, restated ------------------------------------------------------------------------------------------

def realised(case: Case, bn: int, cr: int, sc: int, npw: int) -> dict:
    """What the plan makes of `case`, computed without it, and the proof that the case is what its name says.

    Block plans (bn > 1): edges sorted by (dst // bn, relation, dst % bn); every (block, relation) group cut from its start
    into chunks of <= cr rows; a block with more than sc chunks cut into ceil(chunks / sc) work items.  Returns the chunk
    counts per block and their offsets (blk_chunk_off), the item offsets (item_off), the chunk lengths, the runs of equal
    destination (group, first row in the group, length, row inside its 16-row tile) and, per chunk, the row range of every
    helper wave.  CSR plans (bn == 1): in-degrees, edges per relation and the (destination, relation) run lengths."""
    src, dst = case.edge_index[0], case.edge_index[1]
    rel, N, R = case.rel, case.N, case.R
    assert rel.size == dst.size >= 1 and rel.max() < R - 1, "relation R - 1 has no edges"
    trip = np.stack([src, dst, rel], axis=1)
    _, dup_counts = np.unique(trip, axis=0, return_counts=True)
    loops = trip[src == dst]
    loop_counts = np.unique(loops, axis=0, return_counts=True)[1] if loops.size else np.zeros(0, dtype=np.int64)
    indeg, outdeg = np.bincount(dst, minlength=N), np.bincount(src, minlength=N)
    res = dict(indeg=indeg, rel_edges=np.bincount(rel, minlength=R))
    if bn == 1:
        _, res["dst_rel_runs"] = np.unique(dst * R + rel, return_counts=True)
    else:
        blk, loc = dst // bn, dst % bn
        order = np.lexsort((loc, rel, blk))
        blk, loc, srel, ssrc = blk[order], loc[order], rel[order], src[order]
        nb = -(-N // bn)
        gid, g0, gn = np.unique(blk * R + srel, return_index=True, return_counts=True)
        chunks = []                                            # (block, relation, first sorted edge, rows, group)
        for k, (gk, a, n) in enumerate(zip(gid.tolist(), g0.tolist(), gn.tolist())):
            chunks += [(gk // R, gk % R, a + j, min(cr, n - j), k) for j in range(0, n, cr)]
        c_blk = np.array([c[0] for c in chunks], dtype=np.int64)
        per_block = np.bincount(c_blk, minlength=nb)
        items = np.where(per_block > sc, -(-per_block // sc), 1)
        res.update(chunks_per_block=per_block, blk_chunk_off=np.concatenate([[0], np.cumsum(per_block)]),
                   items_per_block=items, item_off=np.concatenate([[0], np.cumsum(items)]),
                   chunk_lens=np.array([c[3] for c in chunks]), group_sizes=gn, chunks=chunks)
        runs = []                                              # (group, first row in the group, length, row in its tile)
        for k, (a, n) in enumerate(zip(g0.tolist(), gn.tolist())):
            l = loc[a:a + n]
            heads = np.nonzero(np.concatenate([[True], l[1:] != l[:-1]]))[0]
            for p, q in zip(heads.tolist(), np.append(heads[1:], n).tolist()):
                runs.append((k, p, q - p, p % 16))
        res["runs"] = runs
        res["sorted"] = (blk, srel, loc, ssrc)
        if npw > 0:
            waves = []                                         # per chunk: {wave: (first row, last row)}
            for (_, _, e0, rows, _) in chunks:
                w = loc[e0:e0 + rows] // npw
                waves.append({int(x): (int(np.nonzero(w == x)[0][0]), int(np.nonzero(w == x)[0][-1])) for x in np.unique(w)})
            res["waves"] = waves
    for exp in case.expects:
        tag, a = exp[0], exp[1:]
        ok = _CHECKS[tag](res, case, bn, cr, sc, npw, dup_counts, loop_counts, outdeg, *a)
        assert ok, f"{case.name}: condition {exp} is not realised at bn={bn} cr={cr} sc={sc} npw={npw}"
    return res


def _chunk_rows(res, i):
    _, _, e0, rows, _ = res["chunks"][i]
    return slice(e0, e0 + rows)


_CHECKS = {
    "N": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: c.N == n,
    "R": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: c.R == n and res["rel_edges"][n - 1] == 0,
    "edges": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: c.rel.size == n,
    "blocks": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: -(-c.N // bn) == n,
    "self_loop": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: n in loops,
    "dup": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: n in dup,
    "indeg": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: n in res["indeg"],
    "indeg_at_least": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: n in res["indeg"],
    "outdeg": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, v, n: outdeg[v] >= n and (c.edge_index[0] == v).sum() >= n,
    "only_dst": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, v: (c.edge_index[1] == v).all(),
    "all_src": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, v: (c.edge_index[0] == v).all(),
    "rel_edges": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: n in res["rel_edges"],
    "dst_rel_run": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: n in res["dst_rel_runs"],
    "block_chunks": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, b, k: res["chunks_per_block"][b] == k,
    "items": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, b, k: res["items_per_block"][b] == k,
    "group": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: n in res["group_sizes"],
    "chunk_len": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: n in res["chunk_lens"],
    "run": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: any(r[2] == n for r in res["runs"]),
    "run_at": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, row, n: any(r[3] == row and r[2] == n for r in res["runs"]),
    "run_spans_chunks": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: any(
        r[2] == n and r[1] // cr != (r[1] + n - 1) // cr for r in res["runs"]),
    "chunk_one_dst": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: any(
        ch[3] == n and len(set(res["sorted"][2][_chunk_rows(res, i)].tolist())) == 1 for i, ch in enumerate(res["chunks"])),
    "chunk_same_src": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, n: any(
        ch[3] == n and len(set(res["sorted"][3][_chunk_rows(res, i)].tolist())) == 1 for i, ch in enumerate(res["chunks"])),
    "locals": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, want: any(
        tuple(res["sorted"][2][_chunk_rows(res, i)].tolist()) == tuple(want) for i in range(len(res["chunks"]))),
    "wave_only": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, w: any(set(ws) == {w} for ws in res["waves"]),
    "wave_rows": lambda res, c, bn, cr, sc, npw, dup, loops, outdeg, w, lo, hi: any(ws.get(w) == (lo, hi) for ws in res["waves"]),
}
