"""The hypernetwork suite's case tables and float64 restatements (tests/_hyper_cases.py), checked on the CPU.

For every entry: the route it promises is the route the launcher's rules give; the hand-written float64 forward and backward
equal the oracle and its autograd; a plain float32 implementation (the oracle in float32) stays within HALF the bounds the
GPU tests hold the kernels to, so those bounds are reachable; and the hidden units sit far enough from the ReLU kink that
a correct float32 kernel must reproduce the float64 sign pattern.
"""

import numpy as np
import pytest
import torch

import _hyper_cases as H
from oracle import hypergnn_oracle as O

ALL_WG = H.WG_SHAPES + H.LAYOUT_SHAPES
KINK_MARGIN = 2.0 ** -18          # |pre-activation| / sum |terms|: fp32's rounding of a 1024-term sum stays well inside


def _ids(cases):
    return [c.name for c in cases]


def _rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _oracle(case, dtype, masks=None, grad=False):
    """(outputs, gradients) of the oracle in `dtype`: autograd through oracle.weight_generator for loss = sum out . g."""
    inp = H.wg_inputs(case)
    params = {k: torch.from_numpy(v).to(dtype).requires_grad_(grad) for k, v in inp.state.items()}
    x = torch.from_numpy(inp.x).to(dtype).requires_grad_(grad)
    drop = None if masks is None else torch.from_numpy(masks).to(dtype)
    with torch.enable_grad() if grad else torch.no_grad():
        out = O.weight_generator(params, "", x, case.d_in, case.d_out, dtype=dtype, drop=drop)
        grads = None
        if grad:
            sum((out[k] * torch.from_numpy(inp.g[k]).to(dtype)).sum() for k in out).backward()
            grads = {k: p.grad.numpy() for k, p in params.items()}
            grads["text_emb"] = x.grad.numpy()
    return {k: v.detach().numpy() for k, v in out.items()}, grads


def _oracle_active32(case):
    """The float32 oracle's hidden sign pattern [3, nh, R, Hh] (its expression for a hidden layer, layer by layer)."""
    inp = H.wg_inputs(case)
    heads = []
    for head in H.HEADS:
        z, layers = torch.from_numpy(inp.x), []
        for l in range(case.nh):
            w, b = (torch.from_numpy(inp.state[f"generators.{head}.{2 * l}.{n}"]) for n in ("weight", "bias"))
            z = torch.relu(z @ w.t() + b)
            layers.append((z > 0).numpy())
        heads.append(np.stack(layers))
    return np.stack(heads)


@pytest.mark.parametrize("case", ALL_WG, ids=_ids(ALL_WG))
def test_every_entry_reaches_the_route_it_promises(case):
    got = H.realised(case)
    assert case.promise, f"{case.name} promises nothing"
    assert got["fused"] == (case.name not in ("lds_limit", "chain_wide"))


def test_the_tables_hold_what_the_suite_is_meant_to_cover():
    names = {c.name for c in H.WG_SHAPES}
    assert len(names) == len(H.WG_SHAPES) == 18
    routes = {(H.realised(c)["fwd"], H.realised(c)["njt"]) for c in H.WG_SHAPES}
    assert routes == {("mfma3", 2), ("mfma3", 4), ("mfma3", 8), ("mfma3", 16), ("mfma3", 0), ("simple", None)}
    assert set(H.WG_DROPOUT_NAMES) | set(H.WG_BATCHED_NAMES) <= names
    assert {(c.layout, c.d) for c in H.LAYOUT_SHAPES} == ({(H.SPLIT2H, d) for d in H.SPLIT2H_D} | {(H.FRAG16, d) for d in H.FRAG16_D})
    assert {H.realised(c)["fwd"] for c in H.LAYOUT_SHAPES} == {"mfma3", "simple", "mfma_frag16", "simple_frag16"}
    assert len(H.LAYOUT_SHAPES) == 36 and {c.R for c in H.LAYOUT_SHAPES} == {1, 17}
    for d in H.SPLIT2H_REJECTED_D:
        assert not H.layout_supported(H.SPLIT2H, d, d)
    for d in H.FRAG16_REJECTED_D:
        assert not H.layout_supported(H.FRAG16, d, d)
    assert not H.layout_supported(H.FRAG16, 16, 32) and not H.weightgen_bwd_supported(257, 16, 1)
    assert H.weightgen_bwd_supported(256, 256, 7) and not H.weightgen_bwd_supported(16, 16, 8)
    assert H.weightgen_bwd_supported(256, 9999, 0) and [H.cover(w) for w in (1, 32, 33, 64, 65, 200, 256)] == [32, 32, 64, 64, 128, 256, 256]
    ts = H.TEXT_SHAPES
    assert {1, 33, 256, 257, 1024} <= {c.C for c in ts} and {1, 48, 300} <= {c.T for c in ts} and {1, 300} <= {c.U for c in ts}
    assert any(c.Lmax == 1 for c in ts) and len({c.name for c in ts}) == len(ts)


@pytest.mark.parametrize("case", ALL_WG, ids=_ids(ALL_WG))
def test_wg_ref64_equals_the_float64_oracle_and_its_autograd(case):
    ref = H.wg_reference(case)
    out, grads = _oracle(case, torch.float64, grad=True)
    for k in H.HEADS:
        assert _rel_err(ref.out[k], out[k]) <= 1e-12, k
    assert set(grads) == set(ref.grads)
    for k in grads:
        assert _rel_err(ref.grads[k].reshape(grads[k].shape), grads[k]) <= 1e-12, k


@pytest.mark.parametrize("name", H.WG_DROPOUT_NAMES + ("hl64_r33/p1",))
def test_wg_ref64_with_masks_equals_the_oracle(name):
    case, p = H.WG_BY_NAME[name.split("/")[0]], 1.0 if name.endswith("/p1") else H.DROPOUT_P
    masks, log_keep = H.wg_masks(case, p)
    assert masks.shape == (3, case.nh, case.R, case.Hh)
    if p < 1.0:
        kept = float((masks > 0).mean())
        assert abs(kept - (1 - p)) < 0.05 and np.all((masks == 0) | (masks == np.float32(1 / (1 - p))))
        assert log_keep == pytest.approx(np.log(masks.max()), rel=1e-6)
    else:
        assert not masks.any() and log_keep == 0.0
    ref = H.wg_reference(case, p)
    out, grads = _oracle(case, torch.float64, masks=masks, grad=True)
    for k in H.HEADS:
        assert _rel_err(ref.out[k], out[k]) <= 1e-12, k
    for k in grads:
        if np.abs(grads[k]).max() == 0.0:
            assert not ref.grads[k].any(), k
        else:
            assert _rel_err(ref.grads[k].reshape(grads[k].shape), grads[k]) <= 1e-12, k
    if p >= 1.0:                                  # everything behind a dropped layer has no gradient; the last biases do
        assert not ref.grads["text_emb"].any() and not ref.grads["generators.W_msg.0.weight"].any()
        assert ref.grads["generators.bias.4.bias"].any()


@pytest.mark.parametrize("case", ALL_WG, ids=_ids(ALL_WG))
def test_a_float32_implementation_stays_within_half_the_bounds(case):
    ref = H.wg_reference(case)
    out, grads = _oracle(case, torch.float32, grad=True)
    worst_f = max(H.fwd_ratio(out[k], ref.out[k], k) for k in H.HEADS)
    worst_g = max(H.grad_ratio(grads[k], ref.grads[k].reshape(grads[k].shape), k) for k in grads)
    print(f"HYPER-HOST {case.name}: fp32 oracle forward {worst_f:.3f} gradients {worst_g:.3f} of the bounds")
    assert worst_f <= 0.5 and worst_g <= 0.5, (worst_f, worst_g)


@pytest.mark.parametrize("case", ALL_WG, ids=_ids(ALL_WG))
def test_hidden_units_are_mixed_and_off_the_kink(case):
    ref = H.wg_reference(case)
    if case.nh == 0:
        assert H.active_pattern(ref) is None
        return
    margin = min(float((np.abs(z) / m).min()) for zs, ms in zip(ref.pre, ref.mag) for z, m in zip(zs, ms))
    print(f"HYPER-HOST {case.name}: smallest kink margin {margin:.3e} = 2^{np.log2(margin):.1f}")
    assert margin > KINK_MARGIN
    active = H.active_pattern(ref)
    frac = active.reshape(3, case.nh, -1).mean(axis=2)
    assert (frac >= 0.10).all() and (frac <= 0.90).all(), frac
    assert np.array_equal(_oracle_active32(case), active)


@pytest.mark.parametrize("case", H.TEXT_SHAPES, ids=_ids(H.TEXT_SHAPES))
def test_text_ref64_equals_the_float64_oracle_and_its_autograd(case):
    inp = H.text_inputs(case)
    assert inp.ids.shape == (case.U, case.Lmax) and inp.E.shape == (case.V, case.C) and inp.W.shape == (case.T, case.C)
    te, dE, dW, db = H.text_reference(case)
    # the oracle takes strings: the characters each row is read as (clamped ids, clamped lengths; V <= 128 keeps ord = id)
    assert case.V <= O.ASCII_VOCAB
    texts = ["".join(chr(int(c)) for c in row) for row in H.effective_ids(inp.ids, inp.lens, case.V)]
    assert all(O.tokenize(t) == list(row) for t, row in zip(texts, H.effective_ids(inp.ids, inp.lens, case.V)))
    params = {"text_encoder.char_emb.weight": torch.from_numpy(inp.E).double().requires_grad_(True),
              "text_encoder.proj.0.weight": torch.from_numpy(inp.W).double().requires_grad_(True),
              "text_encoder.proj.0.bias": torch.from_numpy(inp.b).double().requires_grad_(True)}
    out = O.text_encode(params, texts, dtype=torch.float64)
    (out * torch.from_numpy(inp.dte).double()).sum().backward()
    assert _rel_err(te, out.detach().numpy()) <= 1e-12
    for got, key in ((dE, "char_emb.weight"), (dW, "proj.0.weight"), (db, "proj.0.bias")):
        assert _rel_err(got, params["text_encoder." + key].grad.numpy()) <= 1e-12, key
    used = H.used_chars(case)
    assert not dE[~used].any() and (np.abs(dE[used]).max(axis=1) > 0).all()
    # a float32 implementation within half the bounds
    p32 = {k: v.detach().float().requires_grad_(True) for k, v in params.items()}
    out32 = O.text_encode(p32, texts)
    (out32 * torch.from_numpy(inp.dte)).sum().backward()
    assert H.text_fwd_ratio(out32.detach().numpy(), te) <= 0.5
    for ref, key in ((dE, "char_emb.weight"), (dW, "proj.0.weight"), (db, "proj.0.bias")):
        assert H.grad_ratio(p32["text_encoder." + key].grad.numpy(), ref, key) <= 0.5, key


def test_text_cases_hold_their_crafted_rows():
    by = {c.name: c for c in H.TEXT_SHAPES}
    long = H.text_inputs(by["long300"])
    assert long.lens[0] == 300 and (long.ids[0] == long.ids[0, 0]).all()
    tw = H.text_inputs(by["twins"])
    assert tw.lens[1] == tw.lens[2] and np.array_equal(tw.ids[1], tw.ids[2])
    te = H.text_reference(by["twins"])[0]
    assert np.array_equal(te[1], te[2])
    em = H.text_inputs(by["empties"])
    assert not em.lens.any() and not em.ids.any()
    assert H.used_chars(by["empties"]).sum() == 1 and H.used_chars(by["small_vocab"]).all()
    un = H.used_chars(by["unused_char"])
    assert not un[H.UNUSED_CHAR] and un.sum() >= by["unused_char"].V - 3
    ri, V = H.text_inputs(by["raw_ids"]), by["raw_ids"].V
    assert {-3, V + 5} <= set(ri.ids.reshape(-1).tolist())
    eff = H.effective_ids(ri.ids, ri.lens, V)
    assert eff[0][0] == 0 and eff[1][1] == V - 1 and list(eff[2][:2]) == [V - 1, 0]
    rl, Lmax = H.text_inputs(by["raw_lens"]), by["raw_lens"].Lmax
    assert list(rl.lens[1:4]) == [0, -1, Lmax + 4]
    assert [len(r) for r in H.effective_ids(rl.ids, rl.lens, 128)[1:4]] == [1, 1, Lmax]


@pytest.mark.parametrize("d", H.FRAG16_D)
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("halves", H.PACK_HALVES)
def test_frag16_helper_inverts_exactly(d, transpose, halves):
    top, bottom = H.pack_inputs(d)
    a, b = (top if halves[0] else None), (bottom if halves[1] else None)
    buf = H.frag16_of(a, b, transpose=transpose)
    assert buf.dtype == np.float32 and buf.shape == (H.PACK_R * 2 * d * d,)
    back = H.frag16_back(buf, H.PACK_R, d)
    for half, w in ((back[:, :d], a), (back[:, d:], b)):
        want = np.zeros_like(top) if w is None else (w.transpose(0, 2, 1) if transpose else w)
        assert np.array_equal(half, want)
    # the documented index: Wfrag[r][o/16][kk/16][((kk%16)/4)*16 + o%16][kk%4]
    r, kk, o = H.PACK_R - 1, d + 5, d - 3
    at = ((((r * (d // 16) + o // 16) * (d // 8) + kk // 16) * 64 + ((kk % 16) // 4) * 16 + o % 16) * 4) + kk % 4
    assert buf[at] == back[r, kk, o]


@pytest.mark.parametrize("d", H.SPLIT2H_D)
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("halves", H.PACK_HALVES)
def test_split2h_helper_inverts_to_its_documented_error(d, transpose, halves):
    top, bottom = H.pack_inputs(d)
    a, b = (top if halves[0] else None), (bottom if halves[1] else None)
    buf = H.split2h_of(a, b, transpose=transpose)
    assert buf.shape == (H.PACK_R * 2 * d * d + H.PACK_R,)
    hi, lo, down = H.split2h_back(buf, H.PACK_R, d)
    cat = np.concatenate([np.zeros_like(top) if w is None else (w.transpose(0, 2, 1) if transpose else w) for w in (a, b)], axis=1)
    mx = np.abs(cat).max(axis=(1, 2))
    assert np.array_equal(down, 2.0 ** (np.floor(np.log2(mx)) - 13))       # lifts the largest magnitude into [2^13, 2^14)
    back = (hi.astype(np.float64) + lo.astype(np.float64)) * down.astype(np.float64)[:, None, None]
    big = np.abs(cat) >= mx[:, None, None] * 2.0 ** -10
    assert np.all(np.abs(back - cat)[big] <= np.abs(cat[big]) * 2.0 ** -21)
    assert np.all(np.abs(back - cat) <= mx[:, None, None] * 2.0 ** -36 + np.abs(cat) * 2.0 ** -21)
    # the documented index: Wh[r][o/16][kk/32][piece][((kk%32)/8)*16 + o%16][kk%8]
    r, kk, o = 1, d + 9, d - 2
    h16 = buf[:H.PACK_R * 2 * d * d].view(np.float16)
    at = (((((r * (d // 16) + o // 16) * (d // 16) + kk // 32) * 2 + 1) * 64 + ((kk % 32) // 8) * 16 + o % 16) * 8) + kk % 8
    assert h16[at] == lo[r, kk, o] and h16[at - 512] == hi[r, kk, o]
