"""The hypernetwork kernels at crafted shapes, forward and backward, against float64 restatements (tests/_hyper_cases.py).

csrc/weightgen.hip (every route of launch_weightgen_batched, every packed layout), csrc/weightgen_bwd.hip (the fused
backward and the per-operation chain it replaces, with and without dropout masks), csrc/text_encoder.hip (forward and its
three backward kernels) and ghf_weights_pack.  The shapes come from the launchers' tile geometry; test_hypernet_host.py
shows on the CPU that each reaches the route it names and that a plain float32 implementation stays within half of every
bound used here.  Layout and reproducibility claims are exact (bit patterns compared).

Every comparison prints its error as a fraction of its bound ("HYPER-RATIO ..."; run with -s to see them).
"""

import functools

import numpy as np
import pytest
import torch

import _hyper_cases as H
from graph_hypernetwork_forge_amd import WeightGenerator, _native
from graph_hypernetwork_forge_amd import autograd as A
from graph_hypernetwork_forge_amd.models.hypergnn import TextEncoder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAT, FRAG16, SPLIT2H = _native.WLAYOUT_NATURAL, _native.WLAYOUT_FRAG16, _native.WLAYOUT_SPLIT2H
MFMA_WG = [c for c in H.WG_SHAPES if H.derive(*c.shape)["fwd"] == "mfma3"]
SIMPLE_WG = [c for c in H.WG_SHAPES if H.derive(*c.shape)["fwd"] == "simple"]


def _ids(cases):
    return [c.name for c in cases]


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(*shape) -> torch.Tensor:
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _report(kind, case, what, ratio):
    print(f"HYPER-RATIO {kind} {case} {what} {ratio:.4f}")
    return ratio


def _check_fwd(case, what, got, ref):
    assert _report("fwd", case, what, H.fwd_ratio(got.detach().cpu().numpy(), ref, f"{case}/{what}")) <= 1.0, f"{case}/{what}"


def _check_grad(case, what, got, ref):
    got = got.detach().cpu().numpy()
    assert _report("grad", case, what, H.grad_ratio(got, ref.reshape(got.shape), f"{case}/d {what}")) <= 1.0, f"{case}/d {what}"


def test_the_constants_restated_for_the_tables_are_the_library_s():
    assert (NAT, FRAG16, SPLIT2H) == (H.NATURAL, H.FRAG16, H.SPLIT2H) and _native.WG_BATCH_MAX == H.WG_MAX_L
    for c in H.WG_SHAPES + H.LAYOUT_SHAPES:
        assert _native.weightgen_bwd_supported(c.T, c.Hh, c.nh) == H.weightgen_bwd_supported(c.T, c.Hh, c.nh), c.name
    assert not _native.weightgen_bwd_supported(257, 16, 1) and not _native.weightgen_bwd_supported(16, 257, 1)


# ---------------------------------------------------------------------------------------------------------------------
# generator forward
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dev(case):
    """(text_emb, flat parameter list, three log-scale tensors) of a table entry on the device."""
    inp = H.wg_inputs(case)
    return _t(inp.x), [_t(p) for p in inp.flat], [_t(inp.ls[k:k + 1]) for k in range(3)]


def _generate(case, layout=NAT, flat=None, want_acts=False):
    """_native.weightgen_fwd into NaN-prefilled buffers."""
    x, flat0, ls = _dev(case)
    R, d_in, d_out = case.R, case.d_in, case.d_out
    if layout == NAT:
        out = (_nan(R, d_in, d_out), _nan(R, d_in, d_out), _nan(R, d_out))
    else:
        out = (_nan(_native.load().ghf_weights_bytes(R, d_in, d_out, layout) // 4), None, _nan(R, d_out))
    res = _native.weightgen_fwd(x, flat0 if flat is None else flat, ls, *case.dims, layout, out=out, want_acts=want_acts)
    assert res[0] is out[0] and res[1] is out[1] and res[2] is out[2]
    return res


@pytest.mark.parametrize("case", H.WG_SHAPES, ids=_ids(H.WG_SHAPES))
def test_generator_forward_natural(case):
    H.realised(case)
    ref = H.wg_reference(case)
    Wm, Ws, b, acts = _generate(case, want_acts=True)
    for k, got in zip(H.HEADS, (Wm, Ws, b)):
        assert torch.isfinite(got).all(), f"{case.name}/{k}: not every element was written"
        _check_fwd(case.name, k, got, ref.out[k])
    active = H.active_pattern(ref)
    if active is None:
        assert acts is None
    else:
        assert tuple(acts.shape) == (3, case.nh, case.R, case.Hh) and torch.isfinite(acts).all()
        assert np.array_equal(acts.cpu().numpy() > 0, active), "hidden sign pattern differs from the float64 one"
    again = _generate(case, want_acts=True)
    for a, c in zip((Wm, Ws, b, acts), again):
        assert (a is None and c is None) or _same_bits(a, c)


def _module(case) -> WeightGenerator:
    gen = WeightGenerator(case.T, case.d_in, case.d_out, hidden_dim=case.Hh, num_hidden=case.nh)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in H.wg_inputs(case).state.items()})
    return gen.to(DEV)


@pytest.mark.parametrize("case", H.WG_SHAPES, ids=_ids(H.WG_SHAPES))
def test_generator_forward_through_the_module(case):
    ref = H.wg_reference(case)
    gen = _module(case).eval()
    x = _dev(case)[0]
    with torch.no_grad():
        out = gen(x)
        row = gen(x[case.R - 1])                                         # a 1-D embedding: one relation
    assert list(out) == list(H.HEADS) == list(row)
    for k in H.HEADS:
        _check_fwd(case.name, "module " + k, out[k], ref.out[k])
        assert row[k].shape == out[k].shape[1:]
        _check_fwd(case.name, "module row " + k, row[k], ref.out[k][case.R - 1])


@pytest.mark.parametrize("case", H.LAYOUT_SHAPES, ids=_ids(H.LAYOUT_SHAPES))
def test_generator_layouts_are_the_packed_natural_outputs(case):
    route = H.realised(case)
    ref = H.wg_reference(case)
    Wm, Ws, b = _generate(case)
    for k, got in zip(H.HEADS, (Wm, Ws, b)):
        _check_fwd(case.name, k, got, ref.out[k])
    Wp, none, bp = _generate(case, layout=case.layout)
    assert none is None and _same_bits(bp, b)
    helper = H.split2h_of if route["pack"] else H.frag16_of
    want = _t(helper(Wm.cpu().numpy(), Ws.cpu().numpy()))
    if case.layout == FRAG16:
        assert torch.isfinite(Wp).all()
    assert _same_bits(Wp, want), f"{case.name}: not the packed form of the natural outputs"


def _generators(case, L):
    """L generators of the entry's shape with distinct parameters."""
    gens = [H.wg_params(case.T, case.Hh, case.nh, case.d_in, case.d_out, case.seed + 7 * g)[1:] for g in range(L)]
    return [[_t(p) for p in flat] for flat, _ in gens], [[_t(ls[k:k + 1]) + 0.01 * g for k in range(3)] for g, (_, ls) in enumerate(gens)]


@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("name", H.WG_BATCHED_NAMES)
def test_batched_generators_give_the_single_calls_bits(name, L):
    case = H.WG_BY_NAME[name]
    x = _dev(case)[0]
    flats, lss = _generators(case, L)
    layouts = [l for l in (NAT, FRAG16, SPLIT2H) if H.layout_supported(l, case.d_in, case.d_out)]
    assert NAT in layouts
    for layout in layouts:
        batched = _native.weightgen_fwd_batched(x, flats, lss, *case.dims, layout)
        assert len(batched) == L
        for g in range(L):
            single = _native.weightgen_fwd(x, flats[g], lss[g], *case.dims, layout)
            for a, c in zip(batched[g], single):
                assert (a is None and c is None) or _same_bits(a, c), f"{name}: generator {g} of {L}, layout {layout}"
        if L > 1:
            assert not _same_bits(batched[0][2], batched[1][2]) and not _same_bits(batched[0][0], batched[L - 1][0])
    if layouts == [NAT]:                      # the packed layouts do not take this d: they are rejected, batched too
        for layout in (FRAG16, SPLIT2H):
            with pytest.raises(ValueError):
                _native.weightgen_fwd_batched(x, flats, lss, *case.dims, layout)


def _off_by_one_float(t: torch.Tensor) -> torch.Tensor:
    """A contiguous copy of t whose storage starts one float into its allocation (4-byte, not 16-byte aligned)."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("case", H.WG_SHAPES, ids=_ids(H.WG_SHAPES))
def test_misaligned_last_layer_weights_take_the_vector_alu_kernel(case):
    ref = H.wg_reference(case)
    flat = list(_dev(case)[1])
    nl = case.nh + 1
    last = [(k * nl + case.nh) * 2 for k in range(3)]
    assert all(flat[i].data_ptr() % 16 == 0 for i in last)
    aligned = _generate(case)
    moved = list(flat)
    for i in last:
        moved[i] = _off_by_one_float(flat[i])
    got = _generate(case, flat=moved)
    for k, g in zip(H.HEADS, got):
        assert torch.isfinite(g).all()
        _check_fwd(case.name, "misaligned " + k, g, ref.out[k])
    if H.derive(*case.shape)["fwd"] == "mfma3":
        # another order of the same sum: some bit differs, or the fallback was not taken
        assert H.derive(*case.shape, aligned=False)["fwd"] == "simple"
        assert not all(_same_bits(a, g) for a, g in zip(aligned, got)), "the misaligned call ran the MFMA kernel"
        # one head misaligned: the other two run the per-head MFMA kernel, the same chain as the merged launch
        moved = list(flat)
        moved[last[0]] = _off_by_one_float(flat[last[0]])
        one = _generate(case, flat=moved)
        _check_fwd(case.name, "one head misaligned W_msg", one[0], ref.out["W_msg"])
        assert _same_bits(one[0], got[0]) and _same_bits(one[1], aligned[1]) and _same_bits(one[2], aligned[2])
    else:
        assert all(_same_bits(a, g) for a, g in zip(aligned, got))         # the vector-ALU kernel either way


def _raw_params(T, Hh, nh, d_in, d_out):
    flat = []
    for n_out in (d_in * d_out, d_in * d_out, d_out):
        width = T
        for _ in range(nh):
            flat += [torch.zeros(Hh, width, device=DEV), torch.zeros(Hh, device=DEV)]
            width = Hh
        flat += [torch.zeros(n_out, width, device=DEV), torch.zeros(n_out, device=DEV)]
    return flat


@pytest.mark.parametrize("what,T,Hh,nh,d,layout", [
    ("T = 1025", 1025, 8, 1, 4, NAT), ("Hh = 1025", 8, 1025, 1, 4, NAT), ("num_hidden = 8", 8, 8, 8, 4, NAT),
    ("SPLIT2H at d = 48", 8, 16, 1, 48, SPLIT2H), ("SPLIT2H at d = 160", 8, 16, 1, 160, SPLIT2H),
    ("FRAG16 at d = 24", 8, 16, 1, 24, FRAG16)])
def test_generator_rejects_what_it_cannot_run(what, T, Hh, nh, d, layout):
    R = 2
    x = torch.zeros(R, T, device=DEV)
    ls = [torch.zeros(1, device=DEV) for _ in range(3)]
    big = _nan(R * 2 * d * d + R)
    out = (_nan(R, d, d), _nan(R, d, d), _nan(R, d)) if layout == NAT else (big, None, _nan(R, d))
    with pytest.raises(ValueError):
        _native.weightgen_fwd(x, _raw_params(T, Hh, nh, d, d), ls, T, Hh, nh, d, d, layout, out=out)
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in out if o is not None), f"{what}: rejected, yet something was written"


def test_batched_call_rejects_nine_generators():
    case = H.WG_BY_NAME["simple_odd"]
    flats, lss = _generators(case, 8)
    with pytest.raises(ValueError):
        _native.weightgen_fwd_batched(_dev(case)[0], flats + flats[:1], lss + lss[:1], *case.dims, NAT)
    torch.cuda.synchronize()
    assert len(_native.weightgen_fwd_batched(_dev(case)[0], flats, lss, *case.dims, NAT)) == 8


# ---------------------------------------------------------------------------------------------------------------------
# generator backward
# ---------------------------------------------------------------------------------------------------------------------

def _backward(case, masks=None, log_keep=None):
    """One training step's gradients through WeightGenerator (with masks: through WeightGeneratorFn, as generate_with_grad
    hands them over): ({name: gradient}, outputs)."""
    inp = H.wg_inputs(case)
    gen = _module(case)
    x = _dev(case)[0].clone().requires_grad_(True)
    if masks is None:
        out = gen(x)
    else:
        dims = case.dims + (masks, log_keep)
        outs = A.WeightGeneratorFn.apply(dims, x, *(gen.log_scales[h] for h in H.HEADS), *gen._head_parameters())
        out = dict(zip(H.HEADS, outs))
    sum((out[k] * _t(inp.g[k])).sum() for k in H.HEADS).backward()
    grads = {"text_emb": x.grad}
    for k, p in gen.named_parameters():
        assert p.grad is not None, f"no gradient on {k}"
        grads[k] = p.grad
    return grads, out


def _count_fused_calls(monkeypatch, fused):
    monkeypatch.setattr(A, "_WG_FUSED_BWD", 2 if fused else 0)
    calls = []
    real = _native.weightgen_bwd
    monkeypatch.setattr(_native, "weightgen_bwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
@pytest.mark.parametrize("case", H.WG_SHAPES, ids=_ids(H.WG_SHAPES))
def test_generator_backward(case, fused, monkeypatch):
    calls = _count_fused_calls(monkeypatch, fused)
    ref = H.wg_reference(case)
    grads, out = _backward(case)
    assert len(calls) == (1 if fused and H.realised(case)["fused"] else 0)
    for k in H.HEADS:
        _check_fwd(case.name, "training forward " + k, out[k], ref.out[k])
    assert set(grads) == set(ref.grads)
    for k in grads:
        _check_grad(case.name, k, grads[k], ref.grads[k])
    again, _ = _backward(case)
    for k in grads:
        assert _same_bits(grads[k], again[k]), f"{case.name}: d {k} differs between two passes"


DROPOUT_CASES = [(n, H.DROPOUT_P) for n in H.WG_DROPOUT_NAMES] + [("hl64_r33", 1.0)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
@pytest.mark.parametrize("name,p", DROPOUT_CASES, ids=[f"{n}-p{p}" for n, p in DROPOUT_CASES])
def test_generator_backward_with_dropout_masks(name, p, fused, monkeypatch):
    case = H.WG_BY_NAME[name]
    calls = _count_fused_calls(monkeypatch, fused)
    masks, log_keep = H.wg_masks(case, p)
    ref = H.wg_reference(case, p)
    grads, out = _backward(case, _t(masks), torch.full((1,), log_keep, dtype=torch.float32, device=DEV))
    assert len(calls) == (1 if fused else 0)
    for k in H.HEADS:
        _check_fwd(case.name, f"p={p} training forward {k}", out[k], ref.out[k])
    for k in grads:
        if p >= 1.0 and not ref.grads[k].any():
            # every unit dropped: nothing reaches the hidden layers, the last layer's weights or the embedding
            assert k == "text_emb" or k.endswith(".weight") or not k.endswith(f".{2 * case.nh}.bias")
            assert not grads[k].any().item(), f"d {k} must be exactly zero"
        else:
            _check_grad(case.name, f"p={p} {k}", grads[k], ref.grads[k])
    if p >= 1.0:
        assert not ref.grads["text_emb"].any() and all(ref.grads[f"generators.{h}.{2 * case.nh}.bias"].any() for h in H.HEADS)
    again, _ = _backward(case, _t(masks), torch.full((1,), log_keep, dtype=torch.float32, device=DEV))
    for k in grads:
        assert _same_bits(grads[k], again[k])


@pytest.mark.parametrize("case", H.WG_FUSED, ids=_ids(H.WG_FUSED))
def test_fused_backward_without_dx_gives_the_same_parameter_gradients(case):
    inp = H.wg_inputs(case)
    x, flat, ls = _dev(case)
    Wm, Ws, b, acts = _generate(case, want_acts=True)
    R = case.R
    outs = [Wm.view(R, -1), Ws.view(R, -1), b]
    g = [_t(inp.g[k]).view(R, -1) for k in H.HEADS]
    ls3 = torch.cat(ls)
    dp, dls, dx = _native.weightgen_bwd(x, flat, acts, outs, g, ls3, *case.dims, want_dx=True)
    dp0, dls0, dx0 = _native.weightgen_bwd(x, flat, acts, outs, g, ls3, *case.dims, want_dx=False)
    assert dx0 is None and dx is not None and len(dp) == len(dp0) == len(flat)
    assert _same_bits(dls, dls0) and all(_same_bits(a, c) for a, c in zip(dp, dp0))
    _check_grad(case.name, "raw text_emb", dx, H.wg_reference(case).grads["text_emb"])


@pytest.mark.parametrize("name", ["lds_limit", "chain_wide"])
def test_fused_backward_rejects_wider_generators(name):
    case = H.WG_BY_NAME[name]
    assert not _native.weightgen_bwd_supported(case.T, case.Hh, case.nh)
    x, flat, ls = _dev(case)
    R = case.R
    z = lambda *s: torch.zeros(*s, device=DEV)                            # noqa: E731
    with pytest.raises(ValueError):
        _native.weightgen_bwd(x, flat, z(3, case.nh, R, case.Hh), [z(R, 16), z(R, 16), z(R, 4)], [z(R, 16), z(R, 16), z(R, 4)],
                              torch.cat(ls), *case.dims)


# ---------------------------------------------------------------------------------------------------------------------
# text encoder
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _text_dev(case):
    inp = H.text_inputs(case)
    return tuple(_t(a) for a in (inp.ids, inp.lens, inp.E, inp.W, inp.b, inp.dte))


@pytest.mark.parametrize("case", H.TEXT_SHAPES, ids=_ids(H.TEXT_SHAPES))
def test_text_encoder_forward(case):
    ids, lens, E, W, b, _ = _text_dev(case)
    te = _native.text_encode_fwd(ids, lens, E, W, b)
    assert tuple(te.shape) == (case.U, case.T)
    ratio = H.text_fwd_ratio(te.cpu().numpy(), H.text_reference(case)[0], case.name)
    assert _report("text-fwd", case.name, "te", ratio) <= 1.0
    assert _same_bits(te, _native.text_encode_fwd(ids, lens, E, W, b))
    if case.craft == "twins":
        assert _same_bits(te[1], te[2])
    if case.craft == "empty":
        assert all(_same_bits(te[0], te[u]) for u in range(1, case.U))


@pytest.mark.parametrize("case", H.TEXT_SHAPES, ids=_ids(H.TEXT_SHAPES))
def test_text_encoder_backward(case):
    ids, lens, E, W, b, dte = _text_dev(case)
    _, dE_ref, dW_ref, db_ref = H.text_reference(case)
    te = _native.text_encode_fwd(ids, lens, E, W, b)
    dE, dW, db = _native.text_encode_bwd(ids, lens, E, W, te, dte)
    for what, got, ref in (("char_emb", dE, dE_ref), ("proj.weight", dW, dW_ref), ("proj.bias", db, db_ref)):
        assert _report("text-grad", case.name, what, H.grad_ratio(got.cpu().numpy(), ref, f"{case.name}/d {what}")) <= 1.0, what
    unused = _t(~H.used_chars(case))
    assert (dE[unused] == 0).all(), "a character no string uses has a gradient"
    if case.craft == "unused":
        assert unused[H.UNUSED_CHAR] and (dE[H.UNUSED_CHAR] == 0).all()
    again = _native.text_encode_bwd(ids, lens, E, W, te, dte)
    assert all(_same_bits(a, c) for a, c in zip((dE, dW, db), again))


def test_text_encoder_rejects_a_wider_character_embedding():
    z = lambda *s: torch.zeros(*s, device=DEV)                            # noqa: E731
    ids, lens = torch.zeros(2, 3, dtype=torch.int32, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        _native.text_encode_fwd(ids, lens, z(8, 1025), z(4, 1025), z(4))
    assert torch.isfinite(_native.text_encode_fwd(ids, lens, z(8, 1024), z(4, 1024), z(4))).all()


def test_text_encoder_module_gradients_are_the_raw_call_s():
    torch.manual_seed(11)
    enc = TextEncoder(text_dim=48, char_emb_dim=24).to(DEV)
    texts = ["knows", "", "café → 東京", "a", "x" * 300, "knows"]
    dte = _t(H.synth.normal(77, "module dte", (len(texts), 48)))
    out = enc(texts, DEV)
    assert out.requires_grad
    (out * dte).sum().backward()
    E, lin = enc.char_emb.weight, enc.proj[0]
    assert all(p.grad is not None for p in (E, lin.weight, lin.bias))
    ids, lens = enc._token_matrix(texts, DEV)
    raw = _native.text_encode_bwd(ids, lens, E.detach(), lin.weight.detach(), out.detach(), dte)
    assert all(_same_bits(p.grad, r) for p, r in zip((E, lin.weight, lin.bias), raw))
    te, dE, dW, db = H.text_ref64(ids.cpu().numpy(), lens.cpu().numpy(), E.detach().cpu().numpy(), lin.weight.detach().cpu().numpy(),
                                  lin.bias.detach().cpu().numpy(), dte.cpu().numpy())
    assert _report("text-fwd", "module", "te", H.text_fwd_ratio(out.detach().cpu().numpy(), te)) <= 1.0
    for what, p, ref in (("char_emb", E, dE), ("proj.weight", lin.weight, dW), ("proj.bias", lin.bias, db)):
        assert _report("text-grad", "module", what, H.grad_ratio(p.grad.cpu().numpy(), ref)) <= 1.0
    assert _same_bits(out[0], out[5]) and (E.grad[1] == 0).all() and E.grad[0].any() and E.grad[127].any()


# ---------------------------------------------------------------------------------------------------------------------
# ghf_weights_pack
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("halves", H.PACK_HALVES, ids=["both", "no-top", "no-bottom"])
@pytest.mark.parametrize("transpose", [False, True], ids=["plain", "transposed"])
@pytest.mark.parametrize("layout,d", H.PACK_SHAPES, ids=[f"{'frag16' if l == H.FRAG16 else 'split2h'}-d{d}" for l, d in H.PACK_SHAPES])
def test_weights_pack_is_the_documented_layout(layout, d, transpose, halves):
    R = H.PACK_R
    top_np, bottom_np = H.pack_inputs(d)
    top, bottom = (_t(top_np) if halves[0] else None), (_t(bottom_np) if halves[1] else None)
    lib = _native.load()
    out = _nan(lib.ghf_weights_bytes(R, d, d, layout) // 4)                # the C call itself: the buffer is the test's own
    _native._check(lib.ghf_weights_pack(_native._ptr(top), _native._ptr(bottom), 1 if transpose else 0, R, d, layout,
                                        out.data_ptr(), _native._stream()), "ghf_weights_pack")
    helper = H.frag16_of if layout == FRAG16 else H.split2h_of
    want = _t(helper(top_np if halves[0] else None, bottom_np if halves[1] else None, transpose=transpose))
    if layout == FRAG16:
        assert torch.isfinite(out).all()
    assert _same_bits(out, want)
    assert _same_bits(_native.weights_pack(top, bottom, transpose, R, d, layout), want)
