"""What the crafted-graph catalogue cannot show of the relation-stationary layer (csrc/message_rs.hip) at its eight widths:

  ghf_weights_pack_rs, called through the C ABI, writes byte for byte what its contract says (tests/_rs_pack_ref.py: the numpy
      restatement, proven in test_wide_rows_host.py) — every width, a relation whose largest entry stands in W_self, a relation
      without W_msg (the backward's shape) — and raises GHF_RANGE_WEIGHTS for exactly the tiles at the guard's threshold.
  The split rows pass 2 writes for the next layer (h_split_out) are the bytes ghf_split_rows cuts from its fp32 output, and a
      second layer fed with them gives the bits of one that cuts the rows itself: the plumbing HyperGNN.forward uses at wide
      rows, without a weight generator (a whole model at hidden 512 has 256 x d^2 parameters per generator head)."""

import functools

import numpy as np
import pytest
import torch

import _edge_graphs as G
import _rs_pack_ref as P
from _util import assert_close
from graph_hypernetwork_forge_amd import _native
from graph_hypernetwork_forge_amd.plan import build_plan, build_rs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S2H = _native.WLAYOUT_SPLIT2H


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pack_on_device(Wm, Ws):
    """(bytes uint8 [ghf_weights_rs_bytes], shifts int32 [R], guard word) of ghf_weights_pack_rs on natural [R, d, d] arrays."""
    lib = _native.load()
    R, d, _ = Wm.shape
    Wm_d, Ws_d = dev(Wm), dev(Ws)
    nbytes = lib.ghf_weights_rs_bytes(R, d)
    assert nbytes == R * 8 * d * d + 4 * R
    buf = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)         # (64 bytes behind the buffer: must stay)
    shift = torch.full((R,), -12345, dtype=torch.int32, device=DEV)
    flag = _native.range_flag(DEV)
    flag.zero_()
    _native._check(lib.ghf_weights_pack_rs(Wm_d.data_ptr(), Ws_d.data_ptr(), R, d, buf.data_ptr(), shift.data_ptr(), _native._stream()),
                   "ghf_weights_pack_rs")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[nbytes:] == 0xA5).all(), "bytes behind the buffer were written"
    return out[:nbytes], shift.cpu().numpy(), int(flag.item())


def _where(idx, R, d):
    body = R * 8 * d * d
    if idx >= body:
        return f"scale of relation {(idx - body) // 4}"
    e = idx // 2
    r, half, piece, n, k = np.unravel_index(e, (R, 2, 2, d, d))
    return f"relation {r} {'W_self' if half else 'W_msg'} piece {'lo' if piece else 'hi'} n={n} k={k}"


@pytest.mark.parametrize("d", G.RS_WIDTHS)
def test_weights_pack_rs_bytes(d):
    assert _native.rs_supported(d)
    Wm, Ws = P.ordinary_weights(d)
    got, shift, word = pack_on_device(Wm, Ws)
    want = P.pack_rs(Wm, Ws)
    assert shift.tolist() == P.shifts(Wm, Ws).tolist(), "per-relation shifts"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, the first at {_where(int(bad[0]), 3, d)}"
    assert word == 0 == P.guard_word(Wm, Ws), f"range guard word {word} on ordinary weights"


@pytest.mark.parametrize("d", (128, 384, 1024))
@pytest.mark.parametrize("case", P.GUARD_CASES)
def test_weights_pack_rs_guard(d, case):
    Wm, Ws, _, expected = P.guard_weights(d, case)
    got, shift, word = pack_on_device(Wm, Ws)
    assert word == expected == P.guard_word(Wm, Ws), f"{case}: guard word {word}, expected {expected}"
    assert np.array_equal(got, P.pack_rs(Wm, Ws)) and shift.tolist() == P.shifts(Wm, Ws).tolist()


# ---- two layers: pass 2's split rows feed the next pass 1 -------------------------------------------------------------------

CHAIN_CASES = ("csr_runs_around_run_max", "csr_in_degrees")


@functools.lru_cache(maxsize=None)
def _chain(d, name):
    """(case, layer-1 inputs, layer-2 parameters, float64 h'' of the two layers), shared by both kinds of plan; read-only."""
    key = f"csr{d}"
    geo = {g[0]: g for g in G.geometries()}[key]
    (case,) = [c for c in G.edge_cases(*geo[2:], d) if c.name == name]
    ins1, ins2 = G.two_layer_inputs(case, d, G.seed_for(key, name))
    ref = G.two_layer_ref64(case, ins1, ins2)
    ref.flags.writeable = False
    return case, ins1, ins2, ref


@pytest.mark.parametrize("runs", (False, True), ids=("edges", "runs"))
@pytest.mark.parametrize("name", CHAIN_CASES)
@pytest.mark.parametrize("d", (384, 512))
def test_split_rows_chain_between_two_layers(d, name, runs, monkeypatch):
    monkeypatch.delenv("GHF_KERNEL", raising=False)
    case, ins1, ins2, ref = _chain(d, name)
    N = case.N
    flag = _native.range_flag(DEV)
    flag.zero_()
    plan = build_plan(dev(case.edge_index), dev(case.rel), [""] * case.R, N, d, DEV)
    assert plan.block_nodes == 1
    rs = build_rs(plan, runs=runs)
    assert (rs.run_start is not None) == runs
    h, Wm1, Ws1, b1, g1, bt1 = (dev(a) for a in ins1)
    Wm2, Ws2, b2, g2, bt2 = (dev(a) for a in ins2)
    Y = torch.full((max(rs.rows, 1), d), float("nan"), device=DEV)
    hs0 = _native.split_rows(h, S2H)
    _native.edge_transform_fwd(h, rs, Wm1, Ws1, b1, Y, h_split=hs0, exact=False)
    out1 = torch.full((N, d), float("nan"), device=DEV)
    hs1 = torch.full_like(_native.alloc_split(N, d, S2H, DEV), 7)
    _native.segment_tail_fwd(Y, rs, h, g1, bt1, G.LN_EPS, out1, h_split_out=hs1, exact=False)
    assert torch.equal(hs1, _native.split_rows(out1, S2H)), "pass 2's split rows are not ghf_split_rows of its output"

    def second(h_split):
        Y.fill_(float("nan"))
        _native.edge_transform_fwd(out1, rs, Wm2, Ws2, b2, Y, h_split=h_split, exact=False)
        out = torch.full((N, d), float("nan"), device=DEV)
        return _native.segment_tail_fwd(Y, rs, out1, g2, bt2, G.LN_EPS, out, exact=False)

    out2 = second(hs1)
    assert torch.equal(out2, second(None)), "layer 2 on the handed-over rows differs from layer 2 cutting them itself"
    got = out2.cpu().numpy()
    rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print(f"FIG chain d={d} {name} runs={int(runs)} rel_l2={rel:.3e} max_abs={np.abs(got - ref).max():.3e}")
    assert_close(got, ref, f"two layers, d={d} {name} runs={runs}")
    assert int(flag.item()) == 0, f"range guard word {int(flag.item())} on inputs of ordinary dynamic range"
