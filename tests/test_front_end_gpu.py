"""The forward's front end at the shapes where its kernels change path: the input projection on two fp16 pieces
(csrc/input_proj.hip: input_proj_h_kernel, a wave walking tiles of 32 rows with clamped row indices past N) and the batched
weight generators (csrc/weightgen.hip: wg_hidden_rb_kernel, several relations per workgroup; wg_out_mfma3_kernel;
wg_pack2h_kernel).

Values are compared with float64 restatements under the bounds the suite already uses (tests/_util.py, tests/_hyper_cases.py);
layouts, the range guard and every "same kernel chain" claim are exact: bit patterns against the stand-alone cutting pass,
against the one-relation-per-workgroup hidden kernel (ghf_weightgen_acts) and against the per-head output kernels the batched
launcher falls back to when one head's last-layer weights are not 16-byte aligned.
"""

import functools

import numpy as np
import pytest
import torch

import _hyper_cases as H
from _util import assert_close
from graph_hypernetwork_forge_amd import HyperGNN, _native, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAT, SPLIT2H = _native.WLAYOUT_NATURAL, _native.WLAYOUT_SPLIT2H


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# input projection, two-piece path
# ---------------------------------------------------------------------------------------------------------------------

# The launcher's geometry (launch_input_proj): a wave owns tiles of 32 rows, a workgroup four waves, the grid is capped at 512
# workgroups, and a wave walks tiles (block * 4 + wave), + grid * 4, ...
ROWS_PER_TILE, WAVES, MAX_GRID = 32, 4, 512
IP_N = [1024,          # the smallest N that takes this kernel: every wave has at most one tile
        65536 + 1,     # 513 blocks on 512 workgroups: one wave runs a second tile — one live row, every other row clamped
        131109]        # two to three tiles per wave, the last tile partly filled, N % 16 != 0
IP_FD = [(F, d) for F in (32, 64, 96, 128) for d in (64, 128)]            # every instance of the kernel


def test_the_row_counts_are_what_the_geometry_promises():
    def tiles_of_waves(N):
        ntiles = -(-N // ROWS_PER_TILE)
        grid = min(-(-N // (ROWS_PER_TILE * WAVES)), MAX_GRID)
        return ntiles, [len(range(w, ntiles, grid * WAVES)) for w in range(grid * WAVES)]
    assert max(tiles_of_waves(1024)[1]) == 1
    ntiles, per = tiles_of_waves(65537)
    assert sorted(set(per)) == [1, 2] and per.count(2) == 1 and per[0] == 2 and 65537 - (ntiles - 1) * ROWS_PER_TILE == 1
    ntiles, per = tiles_of_waves(131109)
    assert sorted(set(per)) == [2, 3] and 131109 % 16 != 0 and 0 < 131109 - (ntiles - 1) * ROWS_PER_TILE < ROWS_PER_TILE


@functools.lru_cache(maxsize=None)
def _ip_inputs(N, F, d):
    """(x, W, b on the device, relu(x W^T + b) in float64 — the oracle's line, hypergnn_oracle.py:219); shared, not modified."""
    x = synth.normal(31, "x", (N, F))
    W = synth.normal(31, "W", (d, F), std=0.2)
    b = synth.normal(31, "b", (d,), std=0.5)
    ref = np.maximum(x.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64), 0.0)
    return _t(x), _t(W), _t(b), ref


@pytest.mark.parametrize("N", IP_N)
@pytest.mark.parametrize("F,d", IP_FD, ids=[f"F{F}-d{d}" for F, d in IP_FD])
def test_input_projection_on_two_pieces(N, F, d):
    x, W, b, ref = _ip_inputs(N, F, d)
    flag = _native.range_flag(DEV)
    flag.zero_()
    hs = _native.alloc_split(N, d, SPLIT2H, DEV)
    h0 = _native.input_proj_fwd(x, W, b, h_split=hs, split_layout=SPLIT2H)
    assert_close(h0.cpu().numpy(), ref, f"input projection N={N} F={F} d={d}")
    assert torch.equal(hs, _native.split_rows(h0, SPLIT2H)), "the rows' pieces and scales are not the cutting pass's"
    assert int(flag.item()) == 0, "benign inputs raised the range guard"
    assert not torch.equal(_native.input_proj_fwd(x, W, b), h0), "the exact kernel ran: this test would be vacuous"
    # one row with too much dynamic range: the last row — at N = 65537 the only live row of the only second tile, whose other
    # rows are clamped onto it; at 131109 a row of the partly filled last tile
    x2 = x.clone()
    x2[N - 1, 0] = 3.0e9
    h2 = _native.input_proj_fwd(x2, W, b, h_split=hs, split_layout=SPLIT2H)
    assert int(flag.item()) & _native.RANGE_ROWS, "the planted row did not raise the rows bit"
    assert torch.equal(h2[:N - 1], h0[:N - 1]), "the planted row changed other rows"
    flag.zero_()


# ---------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------

WG_RB = 4                                       # relations per workgroup of wg_hidden_rb_kernel (csrc/weightgen.hip)
GEN_R = sorted({1, 5, 8 * WG_RB - 1, 8 * WG_RB, 8 * WG_RB + 1, 33})
T, HH, NH = 64, 128, 2                          # the model's generator: hidden width max(64, 2 T), two hidden layers


@functools.lru_cache(maxsize=None)
def _case(d, R):
    return H._wg(f"front_d{d}_r{R}", (T, HH, NH, d, d, R), 5100 + d + R)


@functools.lru_cache(maxsize=None)
def _generators(d, R, L):
    """L generators of one shape with distinct parameters: ([flat parameter list], [three log-scale tensors]) on the device and
    their float64 outputs; shared, not modified."""
    case = _case(d, R)
    x = H.wg_inputs(case).x
    flats, lss, refs = [], [], []
    for g in range(L):
        _, flat, ls = H.wg_params(T, HH, NH, d, d, case.seed + 7 * g)
        flats.append([_t(p) for p in flat])
        lss.append([_t(ls[k:k + 1]) for k in range(3)])
        refs.append(H.wg_ref64(x, flat, ls, NH, d, d))
    return _t(x), flats, lss, refs


def _off_by_one_float(t: torch.Tensor) -> torch.Tensor:
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _per_head(x, flat, ls, d, layout):
    """One generator through the per-head output kernels: with one head's last-layer weights off 16-byte alignment the launcher
    leaves the merged kernel and that head takes the vector ALU, the other two wg_out_mfma_kernel — the merged kernel's chain.
    Two calls, each misaligning a head whose result is taken from the other: (W_msg or packed, W_self or None, bias)."""
    last = [(k * (NH + 1) + NH) * 2 for k in range(3)]
    moved = list(flat)
    moved[last[2]] = _off_by_one_float(flat[last[2]])
    mats = _native.weightgen_fwd(x, moved, ls, T, HH, NH, d, d, layout)
    moved = list(flat)
    moved[last[0]] = _off_by_one_float(flat[last[0]])
    bias = _native.weightgen_fwd(x, moved, ls, T, HH, NH, d, d, NAT)[2]
    return mats[0], mats[1], bias


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("R", GEN_R)
@pytest.mark.parametrize("d", [64, 128])
def test_batched_generators(d, R, L):
    x, flats, lss, refs = _generators(d, R, L)
    nat = _native.weightgen_fwd_batched(x, flats, lss, T, HH, NH, d, d, NAT)
    packed = _native.weightgen_fwd_batched(x, flats, lss, T, HH, NH, d, d, SPLIT2H)
    assert len(nat) == len(packed) == L
    for g in range(L):
        for k, got in zip(H.HEADS, nat[g]):
            ratio = H.fwd_ratio(got.cpu().numpy(), refs[g].out[k], f"d={d} R={R} generator {g}/{L} {k}")
            print(f"FRONT-RATIO d={d} R={R} g={g}/{L} {k} {ratio:.4f}")
            assert ratio <= 1.0, f"generator {g} {k}: {ratio:.3f} of the bound"
        Wp, none, bp = packed[g]
        assert none is None and _same_bits(bp, nat[g][2])
        want = _t(H.split2h_of(nat[g][0].cpu().numpy(), nat[g][1].cpu().numpy()))
        assert _same_bits(Wp, want), f"generator {g}: not the packed form of the natural outputs"
        # the same generator alone, head by head, through the kernels the merged launch replaces
        for layout, mine in ((NAT, nat[g]), (SPLIT2H, packed[g])):
            single = _per_head(x, flats[g], lss[g], d, layout)
            for a, c in zip(mine, single):
                assert (a is None and c is None) or _same_bits(a, c), f"generator {g} of {L}, layout {layout}: not the per-head bits"
    if L > 1:
        assert not _same_bits(nat[0][0], nat[1][0])


@pytest.mark.parametrize("R", [8 * WG_RB + 1, 5])
def test_saved_activations_are_the_one_relation_kernel_s(R):
    """The training path's operands: the activations the forward leaves (several relations per workgroup) against
    ghf_weightgen_acts (one relation per workgroup), bit for bit, and the outputs against float64."""
    d = 64
    x, flats, lss, refs = _generators(d, R, 1)
    Wm, Ws, b, acts = _native.weightgen_fwd(x, flats[0], lss[0], T, HH, NH, d, d, NAT, want_acts=True)
    assert tuple(acts.shape) == (3, NH, R, HH)
    assert _same_bits(acts, _native.weightgen_acts(x, flats[0], T, HH, NH))
    plain = _native.weightgen_fwd(x, flats[0], lss[0], T, HH, NH, d, d, NAT)
    for k, got, same in zip(H.HEADS, (Wm, Ws, b), plain):
        assert H.fwd_ratio(got.cpu().numpy(), refs[0].out[k], f"acts R={R} {k}") <= 1.0
        assert _same_bits(got, same), "asking for the activations changed the outputs"


def test_dropout_masks_line_up_with_the_relations_of_a_workgroup():
    d, R = 64, 8 * WG_RB + 1
    case = _case(d, R)
    x, flats, lss, _ = _generators(d, R, 1)
    masks, _ = H.wg_masks(case, H.DROPOUT_P)
    inp = H.wg_inputs(case)
    _, flat, ls = H.wg_params(T, HH, NH, d, d, case.seed)
    ref = H.wg_ref64(inp.x, flat, ls, NH, d, d, masks=masks)
    m = _t(masks)
    Wm, Ws, b, acts = _native.weightgen_fwd(x, flats[0], lss[0], T, HH, NH, d, d, NAT, hidden_drop=m, want_acts=True)
    assert _same_bits(acts, _native.weightgen_acts(x, flats[0], T, HH, NH, hidden_drop=m))
    assert bool((acts[m == 0] == 0).all()) and bool((acts[m != 0] != 0).any())
    for k, got in zip(H.HEADS, (Wm, Ws, b)):
        assert H.fwd_ratio(got.cpu().numpy(), ref.out[k], f"dropout {k}") <= 1.0


def test_model_generate_batched_is_the_raw_call():
    torch.manual_seed(3)
    model = HyperGNN(text_dim=T, node_feat_dim=32, hidden_dim=64, num_layers=3).to(DEV).eval().requires_grad_(False)
    te = _t(synth.normal(41, "te", (8 * WG_RB + 1, T)))
    got = model.generate_batched(te, SPLIT2H)
    gens = list(model.weight_generators)
    raw = _native.weightgen_fwd_batched(te, [g._head_params() for g in gens], [g._log_scale_vector() for g in gens],
                                        T, gens[0].hidden_dim, gens[0].num_hidden, 64, 64, SPLIT2H)
    assert len(got) == len(raw) == 3
    for a, c in zip(got, raw):
        assert _same_bits(a[0], c[0]) and a[1] is None and _same_bits(a[2], c[2])
