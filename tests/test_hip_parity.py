"""Parity of the HIP path (through the C ABI) with the reference's golden vectors and the oracle.

All tests here need an MI355X.  Tolerance: allclose(rtol=1e-4, atol=1e-5) plus relative
L2 <= 1e-5 (tests/_util.py), the bar BASELINE.json states for this fp32 path.
"""

import dataclasses
import os

import numpy as np
import pytest
import torch

import cases
from _hyper_cases import frag16_of as _to_frag16, split2h_np as _split2h_np, split2h_of as _to_split2h
from _util import assert_close
from graph_hypernetwork_forge_amd import HyperGNN, WeightGenerator, ToyKnowledgeGraph, _native, synth
from graph_hypernetwork_forge_amd.plan import build_plan, relation_ids
from oracle import hypergnn_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def make_model(cfg: cases.ModelCfg, params=None) -> HyperGNN:
    m = HyperGNN(cfg.text_dim, cfg.node_feat_dim, cfg.hidden_dim, cfg.num_layers, char_emb_dim=cfg.char_emb_dim)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in (params or cfg.params()).items()})
    return m.to(DEV).eval()


def run_case(case: cases.GraphCase) -> np.ndarray:
    model = make_model(cases.MODELS[case.model])
    with torch.no_grad():
        out = model(torch.from_numpy(case.node_features).to(DEV), torch.from_numpy(case.edge_index).to(DEV),
                    case.edge_texts)
    return out.cpu().numpy()


def test_native_library_is_loaded():
    lib = _native.load()
    assert lib.ghf_abi_version() == _native.ABI_VERSION
    assert os.path.basename(_native.lib_path()) == "libghf_hip.so"
    assert _native.message_config(128) == (384, _native.WLAYOUT_SPLIT2H, 76, 128)
    assert _native.message_config(64) == (192, _native.WLAYOUT_SPLIT2H, 64, 128)
    assert _native.message_config(20) == (1, _native.WLAYOUT_NATURAL, 0, 0)
    try:
        os.environ["GHF_KERNEL"] = "pp"
        assert _native.message_config(128) == (216, _native.WLAYOUT_FRAG16, 48, 128)
    finally:
        del os.environ["GHF_KERNEL"]


# ---- golden vectors from the reference -----------------------------------------------------

@pytest.mark.parametrize("name", [n for n in cases.GRAPH_CASE_NAMES if n != "g5_c2"])
def test_forward_matches_reference_golden(golden_dir, name):
    (case,) = cases.graph_cases(only=[name])
    g = np.load(os.path.join(golden_dir, f"{name}.npz"))
    assert str(g["params_sha256"]) == cases.params_digest(cases.MODELS[case.model].params())
    assert_close(run_case(case), g["out"], name)


def test_forward_c2_shape_sampled_rows(golden_dir):
    """(200 k edges: below plan.D64_PIECES_MIN_EDGES, so this fixture runs the exact kernel message_pp<64>; BASELINE config 2's own
    size — 1 M edges, message_bx<64> — is test_forward_c2_full_size_default_kernel.)"""
    (case,) = cases.graph_cases(only=["g5_c2"])
    g = np.load(os.path.join(golden_dir, "g5_c2.npz"))
    from graph_hypernetwork_forge_amd import plan as plan_mod
    assert case.edge_index.shape[1] < plan_mod.D64_PIECES_MIN_EDGES
    assert plan_mod.plan_config(64, case.edge_index.shape[1], case.node_features.shape[0])[1] != _native.WLAYOUT_SPLIT2H
    out = run_case(case)
    assert out.shape == tuple(g["out_shape"])
    assert_close(out[g["rows"]], g["out_rows"], "g5_c2 rows")
    assert abs(np.linalg.norm(out.astype(np.float64)) - float(g["out_l2"])) <= 1e-5 * float(g["out_l2"])


_C2_FULL = {}


def _c2_full():
    """BASELINE config 2 at its own size (100 k nodes, 1 M edges, 32 relations, hidden 64, two layers; SURVEY.md §8d's synthetic
    KG, seed 1002) and the oracle's forward on it (reference hypergnn.py:236-298; a few seconds on the host)."""
    if not _C2_FULL:
        cfg = cases.MODELS["c2"]
        params = cfg.params()
        kg = synth.make_kg(100_000, 1_000_000, 32, cfg.node_feat_dim, 1002, "uniform")
        texts = kg.edge_texts()
        ref = O.forward(params, kg.node_features, kg.edge_index, texts, variant="factorised").numpy()
        _C2_FULL.update(cfg=cfg, params=params, x=kg.node_features, ei=kg.edge_index, texts=texts, ref=ref)
    return _C2_FULL


def test_forward_c2_full_size_default_kernel(monkeypatch):
    """The whole model at BASELINE config 2's size through the DEFAULT plan — message_bx<64> on blocks of 192 nodes, two workgroups
    per CU (the kernel BENCH's C2 line times) — against the oracle on EVERY row."""
    monkeypatch.delenv("GHF_KERNEL", raising=False)
    c = _c2_full()
    model = make_model(c["cfg"], c["params"])
    x, ei = torch.from_numpy(c["x"]).to(DEV), torch.from_numpy(c["ei"]).to(DEV)
    plan = model.plan_for(ei, c["texts"], x.size(0), DEV)
    assert plan.block_nodes == 192 and plan.wlayout == _native.WLAYOUT_SPLIT2H and plan.chunk_rows == 64
    with torch.no_grad():
        out = model(x, ei, c["texts"])
        again = model(x, ei, c["texts"])
    assert model.last_range_flags == 0 and torch.equal(out, again)
    assert_close(out.cpu().numpy(), c["ref"], "config 2 at full size, every row")


@pytest.mark.parametrize("flag", ["ZERO_SRC", "ZERO_DST"])
def test_hidden_64_gradient_pass_instances_match_the_oracle_at_half_a_million_edges(flag):
    """message_bx_kernel<64, 1> / <64, 2> — the backward's two passes, at the same two workgroups per CU as the forward's
    instance — on a 0.6 M-edge layer, raw sums of sampled rows against float64 (the half the flag names is zero, as ghf.h
    requires; reference hypergnn.py:201-230 with that half's weights zero)."""
    N, E, R, d = 60_000, 600_000, 24, 64
    ei, rel, h, Wm, Ws, b, gamma, beta = _layer_inputs(N, E, R, d, seed=9090, kind="uniform")
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    os.environ["GHF_KERNEL"] = "bx"
    try:
        plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    finally:
        del os.environ["GHF_KERNEL"]
    assert plan.block_nodes == 192 and plan.wlayout == _native.WLAYOUT_SPLIT2H
    top, bottom = (None, Ws) if flag == "ZERO_SRC" else (Wm, None)
    Wz = _native.weights_pack(None if top is None else t(top), None if bottom is None else t(bottom), True, R, d, plan.wlayout)
    h_d = t(h)
    hs = _native.split_rows(h_d, plan.wlayout)
    out = torch.empty_like(h_d)
    _native.message_layer_fwd(h_d, plan, Wz, None, t(b), plan.wlayout, None, None, 0.0, out, h_split=hs,
                              flags=_native.GHF_FLAG_RAW_SUM | getattr(_native, "GHF_FLAG_" + flag))
    rows = np.unique(synth.randint(6, "rows", 400, N))
    keep = np.isin(ei[1], rows)
    e_src, e_dst, e_rel = ei[0][keep], ei[1][keep], rel[keep]
    h64 = h.astype(np.float64)
    want = np.zeros((N, d))
    # (packed transposed, as the backward packs them: the passes multiply by W^T)
    Wm64 = np.zeros_like(Wm, dtype=np.float64) if top is None else Wm.astype(np.float64).transpose(0, 2, 1)
    Ws64 = np.zeros_like(Ws, dtype=np.float64) if bottom is None else Ws.astype(np.float64).transpose(0, 2, 1)
    for r in range(R):
        m = e_rel == r
        np.add.at(want, e_dst[m], h64[e_src[m]] @ Wm64[r] + h64[e_dst[m]] @ Ws64[r] + b[r].astype(np.float64))
    assert_close(out.cpu().numpy()[rows], want[rows].astype(np.float32), f"{flag} raw sums, sampled rows")


@pytest.mark.parametrize("N,F,d", [(1000, 128, 128), (77, 48, 64), (50, 20, 128)])
def test_input_projection_and_its_fused_split(N, F, d):
    """relu(x W^T + b) against torch, and the SPLIT2H rows the projection emits == ghf_split_rows of its output."""
    x = torch.from_numpy(synth.normal(5, "x", (N, F))).to(DEV)
    W = torch.from_numpy(synth.normal(5, "W", (d, F), std=0.2)).to(DEV)
    b = torch.from_numpy(synth.normal(5, "b", (d,), std=0.5)).to(DEV)
    hs = _native.alloc_split(N, d, _native.WLAYOUT_SPLIT2H, DEV)
    h0 = _native.input_proj_fwd(x, W, b, h_split=hs, split_layout=_native.WLAYOUT_SPLIT2H)
    ref = torch.relu(x.cpu() @ W.cpu().t() + b.cpu())
    assert_close(h0.cpu().numpy(), ref.numpy(), "input projection")
    assert torch.equal(hs, _native.split_rows(h0, _native.WLAYOUT_SPLIT2H))
    assert torch.equal(_native.input_proj_fwd(x, W, b), h0)


@pytest.mark.parametrize("N,F,d", [(20000, 128, 128), (5000, 64, 64), (3001, 32, 128), (70000, 96, 64)])
def test_input_projection_on_two_fp16_pieces(N, F, d, monkeypatch):
    """Callers on the two-piece path (they ask for the SPLIT2H rows) get the projection on fp16 pieces too (round 3): within the
    fp32 tolerance of relu(x W^T + b) (reference hypergnn.py:261), its pieces = ghf_split_rows of its output bit for bit, rows
    with a wide dynamic range raise the guard, and callers without split rows keep the fp32 MFMAs."""
    x = synth.normal(6, "x", (N, F))
    x[::7] *= 37.0                                                   # rows of different magnitudes: one power of two per row
    x[5] = 0.0
    x = torch.from_numpy(x).to(DEV)
    W = torch.from_numpy(synth.normal(6, "W", (d, F), std=0.2)).to(DEV)
    b = torch.from_numpy(synth.normal(6, "b", (d,), std=0.5)).to(DEV)
    flag = _native.range_flag(DEV)
    flag.zero_()
    hs = _native.alloc_split(N, d, _native.WLAYOUT_SPLIT2H, DEV)
    h0 = _native.input_proj_fwd(x, W, b, h_split=hs, split_layout=_native.WLAYOUT_SPLIT2H)
    xd, Wd, bd = x.cpu().double(), W.cpu().double(), b.cpu().double()
    ref = torch.relu(xd @ Wd.t() + bd)
    # the bound of include/ghf.h: 4 * 2^-22 * sum_k |x_k w_k| per output (rows scaled by 37 have sums of ~600: an element that
    # cancels to 0.07 carries the sum's rounding, in fp32 arithmetic as here) — and the usual relative L2
    bound = 4.0 * 2.0 ** -22 * (xd.abs() @ Wd.abs().t() + bd.abs()) + 1e-7
    err = (h0.cpu().double() - ref).abs()
    assert bool((err <= bound).all()), f"input projection on two fp16 pieces: worst error / bound {float((err / bound).max()):.3f}"
    assert float(torch.linalg.norm(h0.cpu().double() - ref) / torch.linalg.norm(ref)) < 1e-6
    assert torch.equal(hs, _native.split_rows(h0, _native.WLAYOUT_SPLIT2H))
    assert int(flag.item()) == 0
    exact = _native.input_proj_fwd(x, W, b)
    assert bool(((exact.cpu().double() - ref).abs() <= bound).all()), "fp32 projection"
    assert not torch.equal(exact, h0), "the two paths are different kernels (this test would be vacuous otherwise)"
    # a row whose small entries lie 2^30 below its largest: flagged
    x2 = x.clone()
    x2[11, 0] = 3.0e9
    flag.zero_()
    _native.input_proj_fwd(x2, W, b, h_split=hs, split_layout=_native.WLAYOUT_SPLIT2H)
    assert int(flag.item()) & _native.RANGE_ROWS
    flag.zero_()


def test_score_triple_and_fused_edge_scores():
    """reference :304-318 and its call form score_triple(embs[src], embs[dst]) (demo.py:90-94)."""
    model = HyperGNN(text_dim=16, node_feat_dim=8, hidden_dim=128, num_layers=1).to(DEV).eval().requires_grad_(False)
    N, E, d = 5000, 40000, 128
    embs = torch.from_numpy(synth.normal(9, "embs", (N, d))).to(DEV)
    src = torch.from_numpy(synth.randint(9, "s", E, N)).to(DEV)
    dst = torch.from_numpy(synth.randint(9, "d", E, N)).to(DEV)
    ref = O.score_triple(embs.cpu()[src.cpu()], embs.cpu()[dst.cpu()])
    assert_close(model.score_edges(embs, src, dst).cpu().numpy(), ref.numpy(), "score_edges", atol=1e-4)
    assert_close(model.score_triple(embs[src], embs[dst]).cpu().numpy(), ref.numpy(), "score_triple [B, d]", atol=1e-4)
    one = model.score_triple(embs[3], embs[7])
    assert one.dim() == 0 and abs(one.item() - float(O.score_triple(embs[3].cpu(), embs[7].cpu()))) < 1e-4
    # recorded: score_edges with its own backward (autograd.ScoreEdgesFn: the pairs grouped by node, one gather pass) against
    # float64 autograd of the oracle's score in the reference's call form; self pairs and repeated pairs included; twice the same bits
    w = torch.from_numpy(synth.normal(9, "w", (E,))).to(DEV)
    src2, dst2 = src % (N - 50), dst % (N - 50)                        # (the last 50 nodes are in no pair)
    src2[:100] = dst2[:100]                                            # i -> i
    src2[100:200], dst2[100:200] = src2[200:300], dst2[200:300]        # the same pair again
    grads = []
    for _ in range(2):
        eg = embs.clone().requires_grad_(True)
        s = model.score_edges(eg, src2, dst2)
        (s * w).sum().backward()
        grads.append(eg.grad)
    e64 = embs.cpu().double().requires_grad_(True)
    s64 = O.score_triple(e64[src2.cpu()], e64[dst2.cpu()])
    (s64 * w.cpu().double()).sum().backward()
    assert_close(s.detach().cpu().numpy(), s64.detach().float().numpy(), "score_edges (recorded)", atol=1e-4)
    assert_close(grads[0].cpu().numpy(), e64.grad.float().numpy(), "d score_edges / d embs", atol=1e-4)
    assert torch.equal(grads[0], grads[1])
    assert float(grads[0][N - 50:].abs().max()) == 0.0 and float(grads[0][:N - 50].abs().max()) > 0.0   # nodes in no pair: zeros
    # odd widths take the scalar path; an out-of-range index gives NaN, not a fault
    e20 = torch.from_numpy(synth.normal(9, "e20", (64, 20))).to(DEV)
    assert_close(_native.score_pairs_fwd(e20, e20).cpu().numpy(), (e20.cpu() ** 2).sum(-1).numpy(), "d = 20", atol=1e-5)
    bad = _native.score_pairs_fwd(embs, embs, torch.tensor([0, N], device=DEV), torch.tensor([1, 2], device=DEV))
    assert torch.isfinite(bad[0]) and torch.isnan(bad[1])
    with pytest.raises(ValueError):
        model.score_triple(embs[:3], embs[:4])


def test_text_encoder_matches_oracle():
    """ghf_text_encode_fwd: all strings in one launch == the reference's per-string loop (empty string, characters
    beyond ASCII clamped to 127, long and one-character strings)."""
    from graph_hypernetwork_forge_amd.models.hypergnn import TextEncoder
    torch.manual_seed(3)
    enc = TextEncoder(text_dim=48, char_emb_dim=24).to(DEV).eval().requires_grad_(False)
    params = {"text_encoder." + k: v.detach().cpu() for k, v in enc.state_dict().items()}
    texts = ["knows", "", "café → 東京", "a", "is parent of", "x" * 300]
    got = enc(texts, DEV)
    ref = O.text_encode(params, texts)
    assert got.shape == (6, 48)
    assert_close(got.cpu().numpy(), ref.numpy(), "text encoder", atol=1e-6)


@pytest.mark.parametrize("name", ["g1_demo", "g1_demo_ls0", "g2_toy", "g3_mid32"])
def test_generated_weights_match_reference(golden_dir, name):
    """K1 in NATURAL layout against the reference's per-layer (W_msg, W_self, bias)."""
    (case,) = cases.graph_cases(only=[name])
    cfg = cases.MODELS[case.model]
    g = np.load(os.path.join(golden_dir, f"{name}.npz"))
    model = make_model(cfg)
    unique, _ = relation_ids(case.edge_texts)
    with torch.no_grad():
        te = model.text_encoder(unique, DEV)
        assert_close(te.cpu().numpy(), g["text_embs"], f"{name}/text_embs")
        for l, gen in enumerate(model.weight_generators):
            w = gen(te)
            for k in ("W_msg", "W_self", "bias"):
                assert_close(w[k].cpu().numpy(), g[f"{k}{l}"], f"{name}/{k}{l}", atol=1e-7)


@pytest.mark.parametrize("c", cases.WG_CASES, ids=lambda c: c.name)
def test_weight_generator_module(golden_dir, c):
    g = np.load(os.path.join(golden_dir, "wg_cases.npz"))
    gen = WeightGenerator(c.text_dim, c.d_in, c.d_out, hidden_dim=c.hidden_dim, num_hidden=c.num_hidden,
                          dropout=c.dropout)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in c.params().items()})
    gen = gen.to(DEV).eval()
    with torch.no_grad():
        out = gen(torch.from_numpy(c.text_emb()).to(DEV))
    assert list(out.keys()) == ["W_msg", "W_self", "bias"]
    for k in ("W_msg", "W_self", "bias"):
        got = out[k].cpu().numpy()
        if c.batch is None:
            assert got.shape == ((c.d_in, c.d_out) if k != "bias" else (c.d_out,))
        if c.keep is not None:
            got = got[list(c.keep)]
        assert_close(got, g[f"{c.name}/{k}"], f"{c.name}/{k}", atol=1e-7)


@pytest.mark.parametrize("num_layers", [3, 9])
@pytest.mark.parametrize("layout", ["natural", "split2h", "frag16"])
def test_batched_generators_equal_the_single_calls(layout, num_layers):
    """ghf_weightgen_fwd_batched (round 3: all layers' generators in one launch sequence) gives, bit for bit, what one
    ghf_weightgen_fwd call per layer gives (reference: one WeightGenerator per layer, hypergnn.py:131-143, :278) — in the
    natural layout (merged output kernel), in SPLIT2H (merged + batched packing) and in FRAG16 (per-head kernels in a loop).
    Nine layers: more generators than one call takes (_native.WG_BATCH_MAX), so generate_batched goes in groups."""
    cfg = dataclasses.replace(cases.MODELS["c3"], num_layers=num_layers)
    assert (num_layers > _native.WG_BATCH_MAX) == (num_layers == 9)
    model = make_model(cfg)
    kg = synth.make_kg(50, 400, 23, cfg.node_feat_dim, seed=5)
    unique, _ = relation_ids(kg.edge_texts())
    wl = {"natural": _native.WLAYOUT_NATURAL, "split2h": _native.WLAYOUT_SPLIT2H, "frag16": _native.WLAYOUT_FRAG16}[layout]
    with torch.no_grad():
        te = model.text_encoder(unique, DEV)
        batched = model.generate_batched(te, wl)
        single = [gen.generate(te, wl) for gen in model.weight_generators]
    torch.cuda.synchronize()
    assert len(batched) == len(single) == num_layers
    for l in range(cfg.num_layers):
        for a, b in zip(batched[l], single[l]):
            assert (a is None) == (b is None)
            if a is not None:
                assert torch.equal(a, b), f"layer {l} {layout}"
    # different layers are different generators: the batched call must not have mixed them up
    assert not torch.equal(batched[0][2], batched[1][2])
    assert not torch.equal(batched[0][2], batched[-1][2])


def test_nine_layer_forward_groups_its_generators(monkeypatch):
    """A model deeper than one batched generator call takes (nine layers: groups of 8 + 1), whole forward, on a small
    block-kernel graph at d = 128 (BASELINE config 3's model with only the depth changed): (a) bit for bit the forward whose
    generate_batched is one ghf_weightgen_fwd call per layer, and (b) the oracle's forward (reference hypergnn.py:236-298)
    within the tolerance the goldens of up to three layers are held to (tests/_util.py)."""
    cfg = dataclasses.replace(cases.MODELS["c3"], num_layers=9)
    params = cfg.params()
    model = make_model(cfg, params)
    kg = synth.make_kg(1500, 6000, 16, cfg.node_feat_dim, seed=909)
    x, ei, texts = torch.from_numpy(kg.node_features).to(DEV), torch.from_numpy(kg.edge_index).to(DEV), kg.edge_texts()
    assert model.plan_for(ei, texts, x.size(0), DEV).block_nodes > 1
    with torch.no_grad():
        out = model(x, ei, texts)
        monkeypatch.setattr(HyperGNN, "generate_batched",
                            lambda self, te, layout: [gen.generate(te, layout) for gen in self.weight_generators])
        looped = model(x, ei, texts)
    assert model.last_range_flags == 0
    assert torch.equal(out, looped)
    ref = O.forward(params, kg.node_features, kg.edge_index, texts, variant="factorised")
    assert_close(out.cpu().numpy(), ref.numpy(), "nine layers")


def test_frag16_layout_is_a_permutation_of_natural():
    c = [x for x in cases.WG_CASES if x.name == "wg_c3_shape"][0]
    gen = WeightGenerator(c.text_dim, c.d_in, c.d_out, hidden_dim=c.hidden_dim)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in c.params().items()})
    gen = gen.to(DEV).eval()
    x = torch.from_numpy(c.text_emb()).to(DEV)
    with torch.no_grad():
        Wm, Ws, b = gen.generate(x, _native.WLAYOUT_NATURAL)
        Wf, none, b2 = gen.generate(x, _native.WLAYOUT_FRAG16)
    assert none is None and torch.equal(b, b2)
    R, d = x.size(0), c.d_in
    # Wfrag[r][o/16][kk/16][lane=((kk%16)/4)*16 + o%16][kk%4], kk indexes rows of [W_msg; W_self]
    cat = torch.cat([Wm, Ws], dim=1)                                   # [R, 2d, d]
    f = Wf.view(R, d // 16, 2 * d // 16, 4, 16, 4)                     # r, nt, j, q, c16, s
    back = f.permute(0, 2, 3, 5, 1, 4).reshape(R, 2 * d, d)            # kk = 16j + 4q + s ; o = 16nt + c16
    assert torch.equal(back, cat)


def _rows_split2h(h):
    """What ghf_split_rows(SPLIT2H) writes: [N][2][d] fp16 then float 2^-s [N], as int16."""
    hi, lo, down = _split2h_np(h, 1)
    return np.concatenate([np.stack([hi, lo], axis=1).reshape(-1).view(np.int16), down.view(np.int16)])


def test_split2h_layout_is_the_two_piece_cut_of_natural():
    c = [x for x in cases.WG_CASES if x.name == "wg_c3_shape"][0]
    gen = WeightGenerator(c.text_dim, c.d_in, c.d_out, hidden_dim=c.hidden_dim)
    gen.load_state_dict({k: torch.from_numpy(v) for k, v in c.params().items()})
    gen = gen.to(DEV).eval()
    x = torch.from_numpy(c.text_emb()).to(DEV)
    with torch.no_grad():
        Wm, Ws, b = gen.generate(x, _native.WLAYOUT_NATURAL)
        Wh, none, b2 = gen.generate(x, _native.WLAYOUT_SPLIT2H)
    assert none is None and torch.equal(b, b2)
    Wm, Ws = Wm.cpu().numpy(), Ws.cpu().numpy()
    assert np.array_equal(Wh.cpu().numpy().view(np.uint16), _to_split2h(Wm, Ws).view(np.uint16))
    # the pieces carry 22 significand bits of every weight within 2^-16 of its matrix' largest
    cat = np.concatenate([Wm, Ws], axis=1)
    hi, lo, down = _split2h_np(cat, 1)
    back = (hi.astype(np.float64) + lo.astype(np.float64)) * down.astype(np.float64)[:, None, None]
    big = np.abs(cat) >= np.abs(cat).max(axis=(1, 2), keepdims=True) * 2.0 ** -10
    assert np.all(np.abs(back - cat)[big] <= np.abs(cat[big]) * 2.0 ** -21)
    assert np.all(np.abs(back - cat) <= np.abs(cat).max(axis=(1, 2), keepdims=True) * 2.0 ** -36 + np.abs(cat) * 2.0 ** -21)


def test_split_rows_and_the_fused_tail_agree(kernel):
    """ghf_split_rows matches its numpy restatement, and a layer's h_split_out equals split_rows of its h_out."""
    if kernel == "pp":
        pytest.skip("the fp32 MFMA kernel gathers h itself")
    d, N, E, R = 128, 3000, 30000, 16
    ei, rel, h, Wm, Ws, b, gamma, beta = _layer_inputs(N, E, R, d, seed=77, kind="uniform")
    h[5] = 0.0                                                                            # an all-zero row
    h[6] *= 1e-30
    h[7] *= 1e20
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    wl = plan.wlayout
    assert wl == _native.WLAYOUT_SPLIT2H
    h_d = t(h)
    hs = _native.split_rows(h_d, wl)
    want = _rows_split2h(h)
    assert np.array_equal(hs.cpu().numpy().reshape(-1), want.reshape(-1))
    part = torch.zeros_like(hs)
    _native.split_rows(h_d, wl, out=part, row0=100, rows=50)
    per_row = 2 * d
    a, z = hs.reshape(-1)[: N * per_row].reshape(N, per_row), part.reshape(-1)[: N * per_row].reshape(N, per_row)
    assert torch.equal(z[100:150], a[100:150]) and not z[:100].any() and not z[150:].any()
    W = _pack_weights(plan, Wm, Ws)[0]
    out, out_split = torch.empty_like(h_d), torch.zeros_like(hs)
    _native.message_layer_fwd(h_d, plan, W, None, t(b), wl, t(gamma), t(beta), 1e-5, out, h_split=hs, h_split_out=out_split)
    assert torch.equal(out_split, _native.split_rows(out, wl))


def _pack_weights(plan, Wm, Ws):
    """(W, W_self) device tensors in the layout the plan's kernel reads."""
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    if plan.wlayout == _native.WLAYOUT_SPLIT2H:
        return t(_to_split2h(Wm, Ws)), None
    if plan.wlayout == _native.WLAYOUT_FRAG16:
        return t(_to_frag16(Wm, Ws)), None
    return t(Wm), t(Ws)


def _skip_unless_kernel_exists(kernel, d):
    """d = 128 and 64: bx and pp; other sizes have one kernel (run once, under "bx")."""
    if kernel not in {128: ("bx", "pp"), 64: ("bx", "pp")}.get(d, ("bx",)):
        pytest.skip(f"no {kernel} kernel for d = {d}")


@pytest.fixture(params=["bx", "pp"])
def kernel(request, monkeypatch):
    """The d = 128 / 64 message kernels: two fp16 pieces with the block sums in registers (bx, the default) and the exact
    v_mfma_f32_16x16x4_f32 kernel the range guard falls back to (pp)."""
    monkeypatch.setenv("GHF_KERNEL", request.param)
    return request.param


# ---- K0 plan properties -----------------------------------------------------------------------

@pytest.mark.parametrize("bn,cr,sc", [(1, 0, 0), (216, 48, 128), (432, 96, 4)])
def test_plan_is_a_sorted_permutation_of_the_edges(bn, cr, sc):
    N, E, R = 5000, 60000, 13
    ei, rel = synth.make_graph_arrays(N, E, R, seed=77, kind="powerlaw")
    pl = _native.plan_build(torch.from_numpy(ei).to(DEV), torch.from_numpy(rel).to(DEV), N, R, bn, cr, sc)
    sk, ss, off, indeg, ctab, boff, status = (pl[k] for k in ("sorted_key", "sorted_src", "seg_off", "indeg", "chunk_tab",
                                                              "blk_chunk_off", "status"))
    assert int(status[0].item()) == 0
    key = sk.cpu().numpy().view(np.uint32).astype(np.int64)
    assert (np.diff(key) >= 0).all()
    blk, rem = key // (R * bn), key % (R * bn)
    r, loc = rem // bn, rem % bn
    dst = blk * bn + loc
    raw = ss.cpu().numpy().view(np.uint32).astype(np.int64)
    src = raw & _native.SRC_MASK if bn > 1 else raw
    got = np.stack([src, dst, r])
    want = np.stack([ei[0], ei[1], rel])
    order = lambda a: a[:, np.lexsort(a[::-1])]                          # noqa: E731
    assert np.array_equal(order(got), order(want))
    assert np.array_equal(indeg.cpu().numpy(), np.bincount(ei[1], minlength=N))
    off = off.cpu().numpy()
    seg = dst if bn == 1 else blk * R + r
    nseg = N if bn == 1 else -(-N // bn) * R
    assert off.shape == (nseg + 1,) and off[0] == 0 and off[-1] == E
    assert np.array_equal(np.diff(off), np.bincount(seg, minlength=nseg))
    if bn == 1:
        assert ctab is None and boff is None
        return
    # run heads: first row of the edge's run of equal keys inside its 16-row tile (tiles start at the group start)
    head = raw >> 28
    t = (np.arange(E) - off[seg]) % 16
    want_head = np.empty(E, dtype=np.int64)
    for e in range(E):
        j = t[e]
        while j > 0 and key[e - (t[e] - j) - 1] == key[e]:
            j -= 1
        want_head[e] = j
    assert np.array_equal(head, want_head)
    # chunk table: the groups of a block, cut into chunks of <= cr rows, in order
    boff = boff.cpu().numpy()
    nb = -(-N // bn)
    assert boff.shape == (nb + 1,) and boff[0] == 0 and (np.diff(boff) >= 0).all()
    tab = ctab.cpu().numpy()[: 2 * boff[-1]].reshape(-1, 2)
    e0, rel_c, rows, cross = tab[:, 0], tab[:, 1] >> 8, tab[:, 1] & 127, (tab[:, 1] >> 7) & 1
    assert rows.min() >= 1 and rows.max() <= cr and rows.sum() == E
    assert np.array_equal(e0, np.concatenate([[0], np.cumsum(rows)[:-1]]))          # chunks tile the sorted edges
    for c in range(len(tab)):
        sl = slice(e0[c], e0[c] + rows[c])
        assert (r[sl] == rel_c[c]).all() and len(set(blk[sl])) == 1
        assert boff[blk[e0[c]]] <= c < boff[blk[e0[c]] + 1]
        want_cross = any(key[e0[c] + b - 1] == key[e0[c] + b] for b in range(16, rows[c], 16))
        assert cross[c] == int(want_cross)
        assert (e0[c] - off[seg[e0[c]]]) % cr == 0
    # work items: a block's chunks in order, cut evenly into ceil(chunks / sc) items when there are more than sc — the whole
    # rule only while the blocks fit one round of workgroups (with more blocks than compute units the last round's blocks
    # are cut further: tests/test_plan_gpu.py::test_last_round_split)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert nb <= cus, f"{nb} blocks on {cus} compute units: the item rule asserted below holds only for plans of one round"
    ioff = pl["blk_item_off"].cpu().numpy()
    n_items, n_slots = int(status[1].item()), int(status[2].item())
    items = pl["item_tab"].cpu().numpy()[: 4 * n_items].reshape(-1, 4)
    assert ioff.shape == (nb + 1,) and ioff[0] == 0 and ioff[-1] == n_items
    slots = []
    for b in range(nb):
        mine = items[ioff[b]:ioff[b + 1]]
        nchunks = boff[b + 1] - boff[b]
        assert len(mine) == (-(-nchunks // sc) if nchunks > sc else 1)
        assert (mine[:, 0] == b).all() and mine[0, 1] == boff[b] and mine[-1, 2] == boff[b + 1]
        assert (mine[1:, 1] == mine[:-1, 2]).all() and (mine[:, 2] >= mine[:, 1]).all()
        if len(mine) > 1:
            assert (mine[:, 2] - mine[:, 1]).max() <= sc
            slots += mine[:, 3].tolist()
        else:
            assert mine[0, 3] == -1
    assert slots == list(range(n_slots))
    assert n_slots > 0 or sc != 4                                       # a small threshold splits this graph for sure


def test_plan_flags_out_of_range_ids():
    ei = torch.tensor([[0, 1, 9], [1, 2, 0]], device=DEV)
    with pytest.raises(IndexError):
        build_plan(ei, torch.tensor([0, 0, 0], device=DEV), ["a"], 5, 16, DEV)
    with pytest.raises(IndexError):
        build_plan(torch.tensor([[0, 1], [1, 2]], device=DEV), torch.tensor([0, 3], device=DEV), ["a", "b"], 5, 16, DEV)


# ---- one message layer against the oracle, seeded inputs --------------------------------------

def _layer_inputs(N, E, R, d, seed, kind):
    ei, rel = synth.make_graph_arrays(N, E, R, seed, kind)
    h = synth.normal(seed, "h", (N, d))
    Wm = synth.normal(seed, "Wm", (R, d, d), std=0.15)
    Ws = synth.normal(seed, "Ws", (R, d, d), std=0.15)
    b = synth.normal(seed, "b", (R, d), std=0.3)
    gamma = (1.0 + 0.2 * synth.normal(seed, "g", (d,))).astype(np.float32)
    beta = (0.2 * synth.normal(seed, "bt", (d,))).astype(np.float32)
    return ei, rel, h, Wm, Ws, b, gamma, beta


@pytest.mark.parametrize("d,N,E,R,kind", [
    (128, 3000, 30000, 64, "uniform"), (128, 2000, 40000, 5, "powerlaw"), (128, 500, 300, 64, "uniform"),
    (64, 6000, 50000, 32, "uniform"), (64, 3000, 45000, 3, "powerlaw"),
    (20, 400, 3000, 7, "uniform"), (16, 300, 2000, 4, "powerlaw"), (256, 300, 2400, 9, "uniform"),
])
@pytest.mark.parametrize("no_tail", [False, True])
def test_message_layer_matches_oracle(d, N, E, R, kind, no_tail, kernel):
    _skip_unless_kernel_exists(kernel, d)
    ei, rel, h, Wm, Ws, b, gamma, beta = _layer_inputs(N, E, R, d, seed=1000 + d + R, kind=kind)
    plan = build_plan(torch.from_numpy(ei).to(DEV), torch.from_numpy(rel).to(DEV), [""] * R, N, d, DEV)
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    W, W2 = _pack_weights(plan, Wm, Ws)
    h_d = t(h)
    out = torch.full_like(h_d, float("nan"))
    _native.message_layer_fwd(h_d, plan, W, W2, t(b), plan.wlayout, None if no_tail else t(gamma),
                              None if no_tail else t(beta), 1e-5, out, flags=_native.GHF_FLAG_NO_TAIL if no_tail else 0)
    th = torch.from_numpy
    ref = O.message_passing_factorised(th(h), th(ei), th(rel), th(Wm), th(Ws), th(b))
    if not no_tail:
        ref = O.layer_tail(ref, th(h), th(gamma), th(beta))
    assert_close(out.cpu().numpy(), ref.numpy(), f"layer d={d} {kind} no_tail={no_tail}")
    if no_tail:                                # K3 alone on the NO_TAIL output reproduces the fused tail
        out2 = torch.empty_like(h_d)
        _native.tail_fwd(out, h_d, t(gamma), t(beta), 1e-5, out2)
        assert_close(out2.cpu().numpy(), O.layer_tail(ref, th(h), th(gamma), th(beta)).numpy(), "tail_fwd")


@pytest.mark.parametrize("d", [128, 64])
def test_split_hub_blocks_match_oracle(d, kernel):
    """Power-law in-degrees: blocks with more chunks than split_chunks are cut into work items whose partial sums a
    second kernel combines in item order (ghf.h: item_tab) — same result, still bitwise reproducible."""
    _skip_unless_kernel_exists(kernel, d)
    N, E, R = 6000, 150000, 8
    ei, rel, h, Wm, Ws, b, gamma, beta = _layer_inputs(N, E, R, d, seed=4242, kind="powerlaw")
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    nb = -(-N // plan.block_nodes)
    n_items = int(plan.item_off_host[-1])
    assert plan.n_slots > 0 and n_items > nb, "this graph must have split blocks"
    assert np.any(np.diff(plan.item_off_host) == 1), "and unsplit ones"
    W, h_d = _pack_weights(plan, Wm, Ws)[0], t(h)
    th = torch.from_numpy
    agg = O.message_passing_factorised(th(h), th(ei), th(rel), th(Wm), th(Ws), th(b))
    for no_tail in (False, True):
        out = torch.full_like(h_d, float("nan"))
        g, bt = (None, None) if no_tail else (t(gamma), t(beta))
        flags = _native.GHF_FLAG_NO_TAIL if no_tail else 0
        _native.message_layer_fwd(h_d, plan, W, None, t(b), plan.wlayout, g, bt, 1e-5, out, flags=flags)
        ref = agg if no_tail else O.layer_tail(agg, th(h), th(gamma), th(beta))
        assert_close(out.cpu().numpy(), ref.numpy(), f"split blocks d={d} no_tail={no_tail}")
        again = torch.empty_like(h_d)
        _native.message_layer_fwd(h_d, plan, W, None, t(b), plan.wlayout, g, bt, 1e-5, again, flags=flags)
        assert torch.equal(out, again)
        bn = plan.block_nodes
        part = torch.full_like(h_d, 7.0)
        _native.message_layer_fwd(h_d, plan, W, None, t(b), plan.wlayout, g, bt, 1e-5, part, row0=bn, rows=3 * bn, flags=flags)
        assert torch.equal(part[bn:4 * bn], out[bn:4 * bn])
        assert (part[:bn] == 7.0).all() and (part[4 * bn:] == 7.0).all()


@pytest.mark.parametrize("N,E,R,kind", [(3000, 30000, 64, "uniform"), (6000, 150000, 8, "powerlaw")])
def test_side_output_and_zero_half_flags(N, E, R, kind):
    """What the training path adds to the d = 128 launch (ghf.h): agg_out — the aggregate before the tail, written beside h'
    and the split rows by the same launch (split hub blocks included) — is bit for bit the GHF_FLAG_NO_TAIL output and
    leaves h' unchanged; GHF_FLAG_ZERO_SRC / ZERO_DST on weights whose half really is zero change nothing but the time."""
    d = 128
    ei, rel, h, Wm, Ws, b, gamma, beta = _layer_inputs(N, E, R, d, seed=515 + R, kind=kind)
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    assert _native.side_output_supported(plan, d)
    W, h_d = _pack_weights(plan, Wm, Ws)[0], t(h)
    hs = _native.split_rows(h_d, plan.wlayout)
    plain, plain_split = torch.empty_like(h_d), torch.empty_like(hs)
    _native.message_layer_fwd(h_d, plan, W, None, t(b), plan.wlayout, t(gamma), t(beta), 1e-5, plain, h_split=hs, h_split_out=plain_split)
    no_tail = torch.empty_like(h_d)
    _native.message_layer_fwd(h_d, plan, W, None, t(b), plan.wlayout, None, None, 0.0, no_tail, h_split=hs, flags=_native.GHF_FLAG_NO_TAIL)
    out, agg, split = torch.empty_like(h_d), torch.full_like(h_d, float("nan")), torch.empty_like(hs)
    _native.message_layer_fwd(h_d, plan, W, None, t(b), plan.wlayout, t(gamma), t(beta), 1e-5, out, h_split=hs, h_split_out=split, agg_out=agg)
    assert torch.equal(out, plain) and torch.equal(split.view(torch.uint8), plain_split.view(torch.uint8))
    assert torch.equal(agg, no_tail)
    th = torch.from_numpy
    assert_close(agg.cpu().numpy(), O.message_passing_factorised(th(h), th(ei), th(rel), th(Wm), th(Ws), th(b)).numpy(), "agg_out")
    with pytest.raises(ValueError, match="agg_out"):
        _native.message_layer_fwd(h_d, plan, W, None, t(b), plan.wlayout, None, None, 0.0, out, h_split=hs, agg_out=agg, flags=_native.GHF_FLAG_NO_TAIL)
    # the two gradient passes: one half of the weights is zero
    zb = torch.zeros(R, d, device=DEV)
    for top, bottom, flag in ((None, Ws, _native.GHF_FLAG_ZERO_SRC), (Wm, None, _native.GHF_FLAG_ZERO_DST)):
        Wz = _native.weights_pack(None if top is None else t(top), None if bottom is None else t(bottom), True, R, d, plan.wlayout)
        for bias in (zb, t(b)):
            base, fast = torch.empty_like(h_d), torch.full_like(h_d, float("nan"))
            _native.message_layer_fwd(h_d, plan, Wz, None, bias, plan.wlayout, None, None, 0.0, base, h_split=hs, flags=_native.GHF_FLAG_RAW_SUM)
            _native.message_layer_fwd(h_d, plan, Wz, None, bias, plan.wlayout, None, None, 0.0, fast, h_split=hs, flags=_native.GHF_FLAG_RAW_SUM | flag)
            assert torch.equal(fast, base), f"flag {flag}: max diff {float((fast - base).abs().max()):.3e}"
    # ... and the flags MEAN "that half must not be read" (ghf.h): ONE pack with both halves nonzero serves both passes, as the
    # backward hands it over (autograd.layer_backward); each pass equals the pass on the pack whose other half is zero
    both = _native.weights_pack(t(Wm), t(Ws), True, R, d, plan.wlayout)
    for top, bottom, flag in ((None, Ws, _native.GHF_FLAG_ZERO_SRC), (Wm, None, _native.GHF_FLAG_ZERO_DST)):
        Wz = _native.weights_pack(None if top is None else t(top), None if bottom is None else t(bottom), True, R, d, plan.wlayout)
        want, got = torch.empty_like(h_d), torch.full_like(h_d, float("nan"))
        _native.message_layer_fwd(h_d, plan, Wz, None, zb, plan.wlayout, None, None, 0.0, want, h_split=hs, flags=_native.GHF_FLAG_RAW_SUM)
        _native.message_layer_fwd(h_d, plan, both, None, zb, plan.wlayout, None, None, 0.0, got, h_split=hs, flags=_native.GHF_FLAG_RAW_SUM | flag)
        # (one power of two per relation is shared by both halves of a pack: the two results agree to the pieces' precision, not bitwise)
        assert_close(got.cpu().numpy(), want.cpu().numpy(), f"flag {flag} on a pack with both halves")
    # kernels that cannot leave a half out refuse the flags instead of computing with it
    os.environ["GHF_KERNEL"] = "pp"
    try:
        plan_pp = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    finally:
        del os.environ["GHF_KERNEL"]
    Wpp = _pack_weights(plan_pp, Wm, Ws)[0]
    with pytest.raises(_native.GhfError, match="ZERO"):
        _native.message_layer_fwd(h_d, plan_pp, Wpp, None, zb, plan_pp.wlayout, None, None, 0.0, out, flags=_native.GHF_FLAG_RAW_SUM | _native.GHF_FLAG_ZERO_SRC)
    with pytest.raises(ValueError, match="nothing to compute"):
        _native.message_layer_fwd(h_d, plan, W, None, zb, plan.wlayout, None, None, 0.0, out, h_split=hs,
                                  flags=_native.GHF_FLAG_RAW_SUM | _native.GHF_FLAG_ZERO_SRC | _native.GHF_FLAG_ZERO_DST)
    # GHF_FLAG_ADD_H: the pass plus other rows, one fp32 add in the tail (how the backward sums its three terms)
    other = torch.randn(N, d, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    for flag in (_native.GHF_FLAG_NO_TAIL, _native.GHF_FLAG_RAW_SUM):
        base, added = torch.empty_like(h_d), torch.full_like(h_d, float("nan"))
        _native.message_layer_fwd(h_d, plan, W, None, t(b), plan.wlayout, None, None, 0.0, base, h_split=hs, flags=flag)
        _native.message_layer_fwd(other, plan, W, None, t(b), plan.wlayout, None, None, 0.0, added, h_split=hs, flags=flag | _native.GHF_FLAG_ADD_H)
        if flag == _native.GHF_FLAG_RAW_SUM:                    # no division: exactly one add
            assert torch.equal(added, base + other)
        else:                                                   # sum / indeg + h contracts into one fma: within an ulp of the two-step form
            torch.testing.assert_close(added, base + other, rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError, match="ADD_H"):
        _native.message_layer_fwd(other, plan, W, None, t(b), plan.wlayout, t(gamma), t(beta), 1e-5, out, h_split=hs, flags=_native.GHF_FLAG_ADD_H)


@pytest.mark.parametrize("d,N", [(20, 301), (32, 77), (64, 1000), (128, 1), (128, 9001), (256, 2050), (384, 130), (512, 300), (1024, 70)])
@pytest.mark.parametrize("dropping", [False, True])
def test_tail_bwd_outputs(d, N, dropping):
    """ghf_tail_bwd against float64 autograd of the tail (reference hypergnn.py:288-296): dpre, G = dpre / c, the LayerNorm's
    dgamma / dbeta summed inside the launch, and G in the two-piece form — the pieces and scales ghf_split_rows cuts from G."""
    g = torch.Generator().manual_seed(100 * d + N)
    agg, h, go = (torch.randn(N, d, generator=g) for _ in range(3))
    gamma = torch.rand(d, generator=g) + 0.5
    indeg = torch.randint(0, 6, (N,), generator=g, dtype=torch.int32)
    drop = ((torch.rand(N, d, generator=g) < 0.75).float() / 0.75) if dropping else None
    pre = (agg.double() + h.double()).requires_grad_(True)
    gam = gamma.double().requires_grad_(True)
    bet = torch.zeros(d, dtype=torch.float64, requires_grad=True)
    x = torch.relu(pre) * (drop.double() if dropping else 1.0)
    torch.nn.functional.layer_norm(x, (d,), gam, bet, 1e-5).backward(go.double())
    dev = lambda a: a.to(DEV)                                                              # noqa: E731
    splittable = d in (64, 128) or d % 128 == 0
    dpre, G, Gs, dgamma, dbeta = _native.tail_bwd(dev(go), dev(agg), dev(h), dev(gamma), 1e-5, dev(indeg), drop=None if drop is None else dev(drop),
                                                  split_layout=_native.WLAYOUT_SPLIT2H if splittable else None)
    assert_close(dpre.cpu().numpy(), pre.grad.float().numpy(), "dpre")
    torch.testing.assert_close(G, dpre / dev(indeg).clamp(min=1).float().unsqueeze(1), rtol=3e-7, atol=0.0)    # (the kernel multiplies by 1/c)
    scale = float(N) ** 0.5                                                                 # the column sums grow like sqrt(N)
    assert_close(dgamma.cpu().numpy() / scale, gam.grad.float().numpy() / scale, "dgamma")
    assert_close(dbeta.cpu().numpy() / scale, bet.grad.float().numpy() / scale, "dbeta")
    if splittable:
        ref = _native.split_rows(G, _native.WLAYOUT_SPLIT2H)                # equal as numbers (a dropped entry's zero keeps its sign here)
        assert torch.equal(Gs[:2 * N * d].view(torch.float16), ref[:2 * N * d].view(torch.float16))
        assert torch.equal(Gs[2 * N * d:], ref[2 * N * d:])                                # the rows' scales
    else:
        assert Gs is None


@pytest.mark.parametrize("d,N,E,R,kind", [(20, 300, 2500, 5, "powerlaw"), (128, 1200, 9000, 6, "uniform"),
                                          (128, 500, 6000, 3, "powerlaw"), (64, 1500, 14000, 6, "uniform"),
                                          (64, 700, 9000, 3, "powerlaw")])
def test_message_layer_backward_matches_autograd_of_the_oracle(d, N, E, R, kind, monkeypatch):
    """Gradients of one layer with respect to h, W_msg, W_self, bias, gamma, beta: HIP backward (autograd.py) against
    torch.autograd through the oracle's restatement of the reference ops.  (d = 64 on the two-piece kernel, which graphs of
    this size do not take by default.)"""
    from graph_hypernetwork_forge_amd.autograd import MessageLayerFn, build_train_plan
    if d == 64:
        monkeypatch.setenv("GHF_KERNEL", "bx")
    ei, rel, h, Wm, Ws, b, gamma, beta = _layer_inputs(N, E, R, d, seed=300 + d + R, kind=kind)
    th = torch.from_numpy
    dev = lambda a: th(a).to(DEV).requires_grad_(True)                                      # noqa: E731
    plan = build_plan(th(ei).to(DEV), th(rel).to(DEV), [""] * R, N, d, DEV)
    tp = build_train_plan(th(ei).to(DEV), th(rel).to(DEV), plan, d, DEV)
    args = [dev(a) for a in (h, Wm, Ws, b, gamma, beta)]
    out = MessageLayerFn.apply(*args, 1e-5, tp)
    gout = th(synth.normal(77, "gout", (N, d)))
    out.backward(gout.to(DEV))
    # oracle: same function in torch on the CPU, differentiated by autograd
    ref_in = [th(a).clone().requires_grad_(True) for a in (h, Wm, Ws, b, gamma, beta)]
    agg = O.message_passing_factorised(ref_in[0], th(ei), th(rel), ref_in[1], ref_in[2], ref_in[3])
    ref = O.layer_tail(agg, ref_in[0], ref_in[4], ref_in[5])
    assert_close(out.detach().cpu().numpy(), ref.detach().numpy(), "training forward")
    ref.backward(gout)
    for name, got, want in zip(("h", "W_msg", "W_self", "bias", "gamma", "beta"), args, ref_in):
        gw, gg = want.grad.numpy(), got.grad.cpu().numpy()
        scale = float(np.abs(gw).max())
        assert np.allclose(gg, gw, rtol=2e-4, atol=2e-5 * max(scale, 1.0)), \
            f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
        rel_l2 = np.linalg.norm((gg - gw).astype(np.float64)) / max(np.linalg.norm(gw.astype(np.float64)), 1e-30)
        assert rel_l2 < 2e-5, f"d{name}: relative L2 {rel_l2:.3e}"


@pytest.mark.parametrize("d,N,E,R", [(128, 700, 30000, 5), (64, 300, 9000, 3), (128, 50, 40, 4), (256, 400, 12000, 4),
                                     (384, 150, 3000, 3)])
def test_edge_outer_matches_the_plain_contraction(d, N, E, R):
    """ghf_edge_outer (all three per-relation gradients in one pass over sliced relation groups) against the same sums in
    float64, including relations without edges, slices shorter than a tile and a hub destination."""
    from graph_hypernetwork_forge_amd import autograd as A
    rng = np.random.default_rng(d + E)
    ei = rng.integers(0, N, size=(2, E))
    ei[1, : E // 4] = 7                                             # a hub
    rel = rng.integers(0, R - 1, size=E)                            # the last relation stays empty
    h = synth.normal(11, "eo_h", (N, d))
    G = synth.normal(12, "eo_g", (N, d))
    t = lambda a: torch.from_numpy(a).to(DEV)                       # noqa: E731
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    old = A.SLICE_EDGES
    try:
        A.SLICE_EDGES = 1024                                        # several slices per relation at this size
        tp = A.build_train_plan(t(ei), t(rel), plan, d, DEV)
    finally:
        A.SLICE_EDGES = old
    assert tp.slice_tab is not None and tp.slice_tab.size(0) >= min(R - 1, E // 1024)
    dW, db = _native.edge_outer(t(h), t(G), tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, R)
    again = _native.edge_outer(t(h), t(G), tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, R)
    assert torch.equal(dW, again[0]) and torch.equal(db, again[1])   # fixed summation order
    # the launch order (band by band, build_train_plan) and any other permutation of the slices: the same bits, on the 16-bit
    # pipe and on the exact fp32 chain
    S = tp.slice_tab.size(0)
    assert tp.slice_order is not None and sorted(tp.slice_order.cpu().tolist()) == list(range(S))
    for order in (tp.slice_order, torch.from_numpy(rng.permutation(S).astype(np.int32)).to(DEV)):
        for exact in (False, True):
            base = (dW, db) if not exact else _native.edge_outer(t(h), t(G), tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, R, exact=True)
            perm = _native.edge_outer(t(h), t(G), tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, R, exact=exact, order=order)
            assert torch.equal(base[0], perm[0]) and torch.equal(base[1], perm[1])
    if d % 128 == 0:
        # ghf_edge_outer_scaled: the one scale per tensor read off the row scales of the split forms — the same bits
        # (rows scaled apart by 2^10 and a row of zeros: the tensor's scale is its largest row's; apart by 2^20 — one outlier row
        # sets the scale for all the others — the scaled call's range guard sends it to the exact chain, see below)
        for lift, same in ((10, True), (20, False)):
            h2 = h.copy()
            h2[3] *= 2.0 ** lift
            h2[5] = 0.0
            hs, gs = _native.split_rows(t(h2), _native.WLAYOUT_SPLIT2H), _native.split_rows(t(G), _native.WLAYOUT_SPLIT2H)
            plain = _native.edge_outer(t(h2), t(G), tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, R)
            scaled = _native.edge_outer(t(h2), t(G), tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, R,
                                        h_scales=_native.split_row_scales(hs, N, d), G_scales=_native.split_row_scales(gs, N, d))
            if not same:
                plain = _native.edge_outer(t(h2), t(G), tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, R, exact=True)
            assert torch.equal(plain[0], scaled[0]) and torch.equal(plain[1], scaled[1]), f"lift 2^{lift}"
        # the range guard of the one-scale pieces (ghf.h): fifteen rows in sixteen of G 2^-20 below the rest (a few rows set the
        # scale) — the call runs on the exact fp32 chain, decided on the device; a quarter of the rows that far down (what a
        # training step's G looks like) does not trip it
        hs1 = _native.split_rows(t(h), _native.WLAYOUT_SPLIT2H)
        for keep_every, trips in ((16, True), (0, False)):
            G3 = G.copy()
            if keep_every:
                small = np.arange(N) % keep_every != 0
            else:
                small = np.arange(N) % 4 == 0
            G3[small] *= 2.0 ** -20
            gs3 = _native.split_rows(t(G3), _native.WLAYOUT_SPLIT2H)
            kw = dict(h_scales=_native.split_row_scales(hs1, N, d), G_scales=_native.split_row_scales(gs3, N, d))
            got = _native.edge_outer(t(h), t(G3), tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, R, **kw)
            exact_chain = _native.edge_outer(t(h), t(G3), tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, R, exact=True)
            pieces = _native.edge_outer(t(h), t(G3), tp.src_by_rel, tp.dst_by_rel, tp.slice_tab, tp.slice_off, R)
            want = exact_chain if trips else pieces
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"guard {'did not trip' if trips else 'tripped'}"
            assert not torch.equal(exact_chain[0], pieces[0]) or N < 100      # (the two chains do differ in their last bits)
    h64, G64 = h.astype(np.float64), G.astype(np.float64)
    for r in range(R):
        m = rel == r
        X = np.concatenate([h64[ei[0, m]], h64[ei[1, m]]], axis=1)
        want, want_b = X.T @ G64[ei[1, m]], G64[ei[1, m]].sum(axis=0)
        scale = max(float(np.abs(want).max()), 1.0)
        assert np.abs(dW[r].cpu().numpy() - want).max() < 2e-5 * scale, f"relation {r}"
        assert np.abs(db[r].cpu().numpy() - want_b).max() < 2e-5 * max(float(np.abs(want_b).max()), 1.0)


@pytest.mark.parametrize("N,d", [(1, 8), (700, 128), (300000, 20), (1500, 4100), (270000, 128), (513, 7)])
def test_backward_helpers_match_numpy(N, d):
    """ghf_colsum (masked, accumulating, several tree levels, widths that are not a multiple of 4 or wider than one
    column tile), ghf_dot, ghf_add3, ghf_rowscale, ghf_scale_exp, ghf_relu_mask, ghf_transpose_batched, matmul_tn."""
    X, M = synth.normal(41, "cs_x", (N, d)), synth.normal(42, "cs_m", (N, d))
    t = lambda a: torch.from_numpy(a).to(DEV)                       # noqa: E731
    tol = lambda want: 3e-6 * max(1.0, float(np.abs(want).max())) * np.sqrt(N)   # noqa: E731
    want = X.astype(np.float64).sum(axis=0)
    got = _native.colsum(t(X))
    assert np.abs(got.cpu().numpy() - want).max() < tol(want)
    assert torch.equal(got, _native.colsum(t(X)))
    wantm = (X.astype(np.float64) * (M > 0)).sum(axis=0)
    acc = torch.ones(d, device=DEV)
    _native.colsum(t(X), mask=t(M), out=acc)
    assert np.abs(acc.cpu().numpy() - 1.0 - wantm).max() < tol(wantm)
    wd = float((X.astype(np.float64) * M).sum())
    assert abs(float(_native.dot(t(X), t(M))) - wd) < 1e-5 * max(1.0, abs(wd)) + 1e-6 * np.sqrt(N * d)
    assert torch.equal(_native.add3(t(X), t(M), t(X)), (t(X) + t(M)) + t(X)) and torch.equal(_native.add3(t(X), t(M)), t(X) + t(M))
    g = synth.normal(43, "cs_g", (N,))
    assert torch.equal(_native.rowscale(t(X), t(g)), t(X) * t(g)[:, None])
    ls = torch.tensor([-0.7], device=DEV)
    assert torch.allclose(_native.scale_exp(t(X), ls), t(X) * ls.exp(), rtol=1e-6, atol=0)
    assert torch.equal(_native.relu_mask(t(X), t(M)), torch.where(t(M) > 0, t(X), torch.zeros_like(t(X))))
    if N * d < 4_000_000:
        assert torch.equal(_native.transpose_batched(t(X)[None]), t(X).t().contiguous()[None])
        Bm = synth.normal(44, "cs_b", (N, 24))
        wmm = X.astype(np.float64).T @ Bm.astype(np.float64)
        gmm = _native.matmul_tn(t(X), t(Bm)).cpu().numpy()
        assert np.abs(gmm - wmm).max() < tol(wmm)


def _grad_check(name, got, want, rtol=2e-4, l2=5e-5):
    gw, gg = want.astype(np.float64), got.astype(np.float64)
    assert gg.shape == gw.shape, f"d{name}: shape {gg.shape} vs {gw.shape}"
    scale = float(np.abs(gw).max())
    assert np.allclose(gg, gw, rtol=rtol, atol=1e-4 * max(scale, 1e-30)), \
        f"d{name}: max abs err {np.abs(gg - gw).max():.3e} at scale {scale:.3e}"
    rel_l2 = np.linalg.norm(gg - gw) / max(np.linalg.norm(gw), 1e-30)
    assert rel_l2 < l2, f"d{name}: relative L2 {rel_l2:.3e}"


@pytest.mark.parametrize("T,Hh,nh,d_in,d_out,R", [(32, 64, 2, 16, 16, 7), (64, 128, 2, 128, 128, 5), (16, 40, 1, 8, 24, 3),
                                                  (16, 32, 0, 8, 8, 4), (32, 64, 3, 20, 20, 1), (64, 128, 2, 20, 20, 187),
                                                  (32, 64, 2, 16, 16, 600), (64, 256, 2, 64, 64, 70), (300, 48, 1, 8, 8, 3)])
@pytest.mark.parametrize("fused", [True, False])
def test_weight_generator_backward_matches_autograd_of_the_oracle(T, Hh, nh, d_in, d_out, R, fused, monkeypatch):
    """Reference tests/test_weight_generator.py:86-106 (gradient reaches the embedding, the scales train) made exact: every
    gradient of WeightGenerator.forward against torch.autograd through the oracle, in float64 — through ghf_weightgen_bwd (all
    heads and layers in three launches; widths up to 256) and through the per-operation chain it replaces."""
    from graph_hypernetwork_forge_amd import autograd as A
    monkeypatch.setattr(A, "_WG_FUSED_BWD", 2 if fused else 0)
    calls = []
    real = _native.weightgen_bwd
    monkeypatch.setattr(_native, "weightgen_bwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.manual_seed(T + Hh + nh)
    gen = WeightGenerator(T, d_in, d_out, hidden_dim=Hh, num_hidden=nh).to(DEV)
    with torch.no_grad():
        for h in ("W_msg", "W_self", "bias"):
            gen.generators[h][-1].weight.mul_(30.0)                    # beyond the 0.01 initialisation
            gen.generators[h][-1].bias.normal_(0.0, 0.3)
            gen.log_scales[h].fill_({"W_msg": -0.5, "W_self": 0.25, "bias": -1.0}[h])
    x = torch.from_numpy(synth.normal(5, "wgx", (R, T))).to(DEV).requires_grad_(True)
    out = gen(x)
    gouts = {k: torch.from_numpy(synth.normal(6, "g" + k, tuple(v.shape))) for k, v in out.items()}
    sum((out[k] * gouts[k].to(DEV)).sum() for k in out).backward()
    assert len(calls) == (1 if fused and max(T, Hh if nh else 0) <= 256 else 0)
    ref_p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in gen.state_dict(keep_vars=True).items()}
    xr = x.detach().cpu().double().requires_grad_(True)
    ref = O.weight_generator(ref_p, "", xr, d_in, d_out, dtype=torch.float64)
    for k in out:
        assert_close(out[k].detach().cpu().numpy(), ref[k].detach().float().numpy(), f"training forward {k}")
    sum((ref[k] * gouts[k].double()).sum() for k in ref).backward()
    _grad_check("text_emb", x.grad.cpu().numpy(), xr.grad.numpy())
    for k, p in gen.named_parameters():
        assert p.grad is not None, f"no gradient on {k}"
        _grad_check(k, p.grad.cpu().numpy(), ref_p[k].grad.numpy())
    single = gen(x.detach()[0].clone().requires_grad_(True))            # 1-D embedding (reference :132-134)
    assert single["W_msg"].shape == (d_in, d_out) and single["W_msg"].requires_grad


def _model_grads(name, node_features, edge_index, edge_texts, gout, x_grad=False):
    """(HIP model with .grad filled, oracle float64 parameters with .grad filled, outputs) for loss = sum(out * gout)."""
    cfg = cases.MODELS[name]
    params = cfg.params()
    model = make_model(cfg, params).train()
    x = torch.from_numpy(node_features).to(DEV).requires_grad_(x_grad)
    out = model(x, torch.from_numpy(edge_index).to(DEV), edge_texts)
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    ref_p = {k: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True) for k, v in params.items()}
    xr = torch.from_numpy(node_features).double().requires_grad_(x_grad)
    ref = O.forward(ref_p, xr, edge_index, edge_texts, variant="factorised", dtype=torch.float64)
    (ref * torch.from_numpy(gout).double()).sum().backward()
    return model, ref_p, out, ref, x, xr


@pytest.mark.parametrize("name,N,E,R,kind", [("small", 0, 0, 0, "toy"), ("mid32", 300, 2500, 6, "powerlaw"),
                                             ("c2", 700, 6000, 9, "uniform"), ("c3", 900, 8000, 7, "powerlaw")])
def test_model_backward_matches_autograd_of_the_oracle(name, N, E, R, kind):
    """Every parameter gradient of HyperGNN.forward (text encoder, input projection, generators, log-scales, LayerNorms)
    against torch.autograd through the float64 oracle — the reference trains by plain autograd (demo.py:79-101)."""
    cfg = cases.MODELS[name]
    if kind == "toy":
        kg = ToyKnowledgeGraph(feat_dim=cfg.node_feat_dim)
        nf, ei, texts = kg.node_features.numpy(), kg.edge_index.numpy(), kg.edge_texts
    else:
        g = synth.make_kg(N, E, R, cfg.node_feat_dim, seed=900 + N, kind=kind)
        nf, ei, texts = g.node_features, g.edge_index, g.edge_texts()
    gout = synth.normal(31, "gout", (nf.shape[0], cfg.hidden_dim))
    model, ref_p, out, ref, x, xr = _model_grads(name, nf, ei, texts, gout, x_grad=(name != "c3"))
    assert_close(out.detach().cpu().numpy(), ref.detach().float().numpy(), "training forward")
    for k, p in model.named_parameters():
        assert p.grad is not None, f"no gradient on {k}"
        _grad_check(k, p.grad.cpu().numpy(), ref_p[k].grad.numpy())
    if x.requires_grad:
        _grad_check("node_features", x.grad.cpu().numpy(), xr.grad.numpy())
    model.eval()
    with torch.no_grad():                                               # the inference kernels agree with the recorded forward
        assert_close(model(x.detach(), torch.from_numpy(ei).to(DEV), texts).cpu().numpy(), out.detach().cpu().numpy(), "eval")


@pytest.mark.parametrize("d", [128, 256])
def test_training_forward_falls_back_to_the_exact_kernels_when_the_range_guard_fires(d):
    """rows the two-fp16-piece kernels cannot hold used to raise in training mode; the reference's plain
    fp32 autograd (tests/test_hypergnn.py:183-226) computes them.  The recorded forward now reruns on the exact plan: output =
    the oracle, every parameter gradient = float64 autograd through the oracle."""
    cfg, params, x_np, ei_np, texts = _adversarial_graph(d)
    gout = synth.normal(33, "gout", (x_np.shape[0], d))
    model = make_model(cfg, params).train()
    x = torch.from_numpy(x_np).to(DEV)
    out = model(x, torch.from_numpy(ei_np).to(DEV), texts)
    assert model.last_range_flags & _native.RANGE_ROWS
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    ref_p = {k: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True) for k, v in params.items()}
    ref = O.forward(ref_p, torch.from_numpy(x_np).double(), ei_np, texts, variant="factorised", dtype=torch.float64)
    (ref * torch.from_numpy(gout).double()).sum().backward()
    assert_close(out.detach().cpu().numpy(), ref.detach().float().numpy(), f"training forward after the fallback d={d}")
    for k, p in model.named_parameters():
        if float(ref_p[k].grad.abs().max()) == 0.0:                     # (the adversarial model zeroes a block of generator weights)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
            continue
        _grad_check(k, p.grad.cpu().numpy(), ref_p[k].grad.numpy())


def test_feature_gradient_beyond_one_launch_of_rows():
    """d loss / d node_features was capped at 1,048,560 rows (a grid dimension of the contraction);
    now slabs of rows.  1.2 M rows: sampled rows of the gradient of h0 = relu(x W^T + b) against float64 (reference
    hypergnn.py:261 under plain autograd)."""
    from graph_hypernetwork_forge_amd.autograd import InputProjFn
    N, F, d = 1_200_000, 16, 32
    g = torch.Generator(device="cpu").manual_seed(8)
    x = torch.randn(N, F, generator=g).to(DEV).requires_grad_(True)
    W = (0.3 * torch.randn(d, F, generator=g)).to(DEV).requires_grad_(True)
    b = (0.1 * torch.randn(d, generator=g)).to(DEV).requires_grad_(True)
    gout = torch.randn(N, d, generator=g).to(DEV)
    h0 = InputProjFn.apply(x, W, b)
    (h0 * gout).sum().backward()
    rows = torch.cat([torch.arange(0, 64), torch.arange(1_048_500, 1_048_700), torch.arange(N - 64, N)]).to(DEV)
    xr = x.detach()[rows].double().cpu().requires_grad_(True)
    Wr, br = W.detach().double().cpu(), b.detach().double().cpu()
    (torch.relu(xr @ Wr.t() + br) * gout[rows].double().cpu()).sum().backward()
    _grad_check("node_features (sampled rows)", x.grad[rows].cpu().numpy(), xr.grad.numpy())
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad[1_048_560:].abs().max()) > 0.0


@pytest.mark.parametrize("d", [128, 64])
def test_input_projection_weight_gradient_through_edge_outer(d, monkeypatch):
    """InputProjFn.backward on a training plan with node_feat_dim == hidden_dim and >= 65,536 rows takes dW / db from
    ghf_edge_outer over the identity "edges" (autograd.py): against float64 autograd of relu(x W^T + b) (reference
    hypergnn.py:261), and against the ghf_group_outer chain it replaces."""
    from graph_hypernetwork_forge_amd import autograd as A
    N, E, R = 70_000, 90_000, 3
    ei, rel = synth.make_graph_arrays(N, E, R, seed=31)
    t = lambda a: torch.from_numpy(a).to(DEV)                       # noqa: E731
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    tp = A.build_train_plan(t(ei), t(rel), plan, d, DEV)
    g = torch.Generator(device="cpu").manual_seed(9)
    x0, W0, b0 = torch.randn(N, d, generator=g), 0.2 * torch.randn(d, d, generator=g), 0.1 * torch.randn(d, generator=g)
    gout = torch.randn(N, d, generator=g)
    grads = {}
    for on in (True, False):
        monkeypatch.setattr(A, "_IP_EDGE_OUTER", on)
        W, b = W0.to(DEV).requires_grad_(True), b0.to(DEV).requires_grad_(True)
        h0 = A.InputProjFn.apply(x0.to(DEV), W, b, tp)
        (h0 * gout.to(DEV)).sum().backward()
        grads[on] = (W.grad.cpu().numpy(), b.grad.cpu().numpy())
    assert tp.ident is not None and tp.ident[0].numel() == N
    Wr, br = W0.double().requires_grad_(True), b0.double().requires_grad_(True)
    (torch.relu(x0.double() @ Wr.t() + br) * gout.double()).sum().backward()
    for on in (True, False):
        _grad_check(f"input_proj.weight (edge_outer {on})", grads[on][0], Wr.grad.numpy())
        _grad_check(f"input_proj.bias (edge_outer {on})", grads[on][1], br.grad.numpy())


def test_training_generator_side_stream_changes_no_bit(monkeypatch):
    """Large graphs train with the generators on a side stream (their backward then runs beside the message layers' gradient
    kernels).  Forced on for a small graph, three steps: output and every gradient bit for bit what the single-stream schedule
    computes."""
    cfg = cases.MODELS["c3"]
    g = synth.make_kg(1500, 16000, 9, cfg.node_feat_dim, seed=77, kind="powerlaw")
    ei, texts = torch.from_numpy(g.edge_index).to(DEV), g.edge_texts()
    gout = torch.from_numpy(synth.normal(32, "gout", (1500, cfg.hidden_dim))).to(DEV)

    def run(side: bool):
        monkeypatch.setattr(HyperGNN, "SIDE_STREAM_MIN_EDGES", 0 if side else 1 << 60)
        model = make_model(cfg, cfg.params()).train()
        x = torch.from_numpy(g.node_features).to(DEV).requires_grad_(True)
        for _ in range(3):                                             # (the streams are reused from the second step on)
            model.zero_grad(set_to_none=True)
            x.grad = None
            out = model(x, ei, texts)
            (out * gout).sum().backward()
        torch.cuda.synchronize()
        return out.detach(), x.grad, {k: p.grad for k, p in model.named_parameters()}

    out0, xg0, g0 = run(False)
    out1, xg1, g1 = run(True)
    assert torch.equal(out0, out1) and torch.equal(xg0, xg1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_training_mode_dropout_matches_reference_and_its_gradients(golden_dir, monkeypatch):
    """train() with dropout 0.25 (reference hypergnn.py:293-294, weight_generator.py:96-107): with the masks the reference drew
    (tests/golden/g_dropout.npz) handed to the HIP path in place of its own draws, the forward equals the reference's
    training-mode output and every gradient equals float64 autograd through the oracle with the same masks; with its own
    draws the masks have the right rate and scale; eval() is untouched."""
    from test_oracle_golden import DROPOUT_CASE as c, dropout_case
    from graph_hypernetwork_forge_amd.models.weight_generator import WeightGenerator as WG
    params, g, texts, drop, want = dropout_case(golden_dir)
    model = HyperGNN(c["T"], c["F"], c["d"], c["L"], dropout=c["p"]).to(DEV)
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    model.train()
    x, ei = torch.from_numpy(g.node_features).to(DEV), torch.from_numpy(g.edge_index).to(DEV)
    queue = {"gen": [m.to(DEV) for m in drop["gen"]], "layers": [m.to(DEV) for m in drop["layers"]]}
    seen = []

    def gen_mask(self, shape, device):
        seen.append(("gen", tuple(shape)))
        return queue["gen"].pop(0)

    def layer_mask(self, shape, device):
        seen.append(("layer", tuple(shape)))
        return queue["layers"].pop(0)
    with monkeypatch.context() as mp_:
        mp_.setattr(WG, "_draw_mask", gen_mask)
        mp_.setattr(HyperGNN, "_draw_mask", layer_mask)
        out = model(x, ei, texts)
        assert seen == [("gen", tuple(drop["gen"][0].shape)), ("layer", (c["N"], c["d"]))] * c["L"], "the reference's draw order"
        assert_close(out.detach().cpu().numpy(), want, "training-mode forward with the reference's masks")
        gout = synth.normal(5, "gout", (c["N"], c["d"]))
        (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    ref_p = {k: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True) for k, v in params.items()}
    ref = O.forward(ref_p, torch.from_numpy(g.node_features).double(), g.edge_index, texts, variant="factorised",
                    dtype=torch.float64, drop=drop)
    (ref * torch.from_numpy(gout).double()).sum().backward()
    for k, p_ in model.named_parameters():
        assert p_.grad is not None, f"no gradient on {k}"
        _grad_check(k, p_.grad.cpu().numpy(), ref_p[k].grad.numpy())
    # its own draws: Bernoulli(1 - p) / (1 - p), different every call; under no_grad too (the reference drops whenever training)
    drawn = model._draw_mask((4000, c["d"]), DEV)
    assert all(v == 0.0 or abs(v - 1 / (1 - c["p"])) < 1e-6 for v in np.unique(drawn.cpu().numpy()).tolist())
    assert abs(float((drawn > 0).float().mean()) - (1 - c["p"])) < 0.02
    with torch.no_grad():
        a, b = model(x, ei, texts), model(x, ei, texts)
    assert not torch.allclose(a, b, atol=1e-3) and not np.allclose(a.cpu().numpy(), want, atol=1e-2)
    with pytest.raises(NotImplementedError):
        model.forward_planned(x, model.plan_for(ei, texts, c["N"], DEV))
    model.eval()
    with torch.no_grad():
        e1, e2 = model(x, ei, texts), model(x, ei, texts)
    assert torch.equal(e1, e2)
    assert_close(e1.cpu().numpy(), O.forward(params, g.node_features, g.edge_index, texts, variant="factorised").numpy(), "eval")


def test_relu_kink_instance_lands_on_one_side_of_the_float64_oracle():
    """The waived case of the round-1 fuzz sweep (tests/fuzz_parity.py --seed 33, case 22: d=128 N=750 E=13290 R=18 L=3),
    pinned.  One hidden pre-activation of generator 0's W_msg head — relation 0, unit 26 — is +9.0e-9 in float64 against a
    mean magnitude of 0.13: float32 arithmetic decides the sign of that ReLU by summation order, and the gradient of the
    head's first Linear moves by 4e-3 (relative L2) with it.  The HIP gradient must equal, to 1e-5, the float64 oracle's on
    the side of the kink the HIP forward took (read from ghf_weightgen_acts) — the oracle as is, or with that bias moved by
    twice the pre-activation — and every other parameter's too: the discrepancy is the kink, nothing else."""
    d, N, E, R, L, T, F, seed = 128, 750, 13290, 18, 3, 64, 8, 805761091
    g = synth.make_kg(N, E, R, F, seed=seed, kind="uniform")
    ei = g.edge_index.copy()
    ei[1, : E // 5] = ei[0, : E // 5]                                   # the sweep's self loops and duplicates
    ei[:, E // 5: 2 * (E // 5)] = ei[:, : E // 5][:, : 2 * (E // 5) - E // 5]
    texts = g.edge_texts()
    params = synth.hypergnn_params(T, F, d, L, seed=seed % 1000 + 1, log_scale=0.0, randomize_ln=True)
    head = "weight_generators.0.generators.W_msg."
    uniq, _ = O.relation_ids(texts)
    z = O.text_encode(params, uniq, dtype=torch.float64)
    pre = z @ torch.from_numpy(params[head + "0.weight"]).double().t() + torch.from_numpy(params[head + "0.bias"]).double()
    r, u = divmod(int(pre.abs().argmin()), pre.size(1))
    assert (r, u) == (0, 26) and 0.0 < float(pre[r, u]) < 1e-7 * float(pre.abs().mean()), "the instance changed"
    others = torch.cat([pre[:r, u], pre[r + 1:, u]]).abs().min()
    assert float(others) > 1e3 * float(pre[r, u]), "moving the bias must flip this relation's unit only"

    model = HyperGNN(T, F, d, L).to(DEV).train()
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    x = torch.from_numpy(g.node_features).to(DEV)
    gout = synth.normal(seed % 977, "fz", (N, d))
    out = model(x, torch.from_numpy(ei).to(DEV), texts)
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    gen = model.weight_generators[0]
    with torch.no_grad():
        te = model.text_encoder(list(uniq), DEV)
        acts = _native.weightgen_acts(te, gen._head_params(), T, gen.hidden_dim, gen.num_hidden)    # [head][layer][r][unit]
    hip_active = bool(acts[0, 0, r, u] > 0)

    def oracle_grads(p):
        rp = {k: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True) for k, v in p.items()}
        ro = O.forward(rp, torch.from_numpy(g.node_features).double(), ei, texts, variant="factorised", dtype=torch.float64)
        (ro * torch.from_numpy(gout).double()).sum().backward()
        return {k: v.grad.numpy() for k, v in rp.items()}

    flipped = dict(params)
    fb = params[head + "0.bias"].astype(np.float64)
    fb[u] -= 2.0 * float(pre[r, u])
    flipped[head + "0.bias"] = fb                                        # float64: the move is far below float32 spacing
    plain_g, flip_g = oracle_grads(params), oracle_grads(flipped)
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))    # noqa: E731
    key = head + "0.weight"
    assert rel(plain_g[key], flip_g[key]) > 1e-3, "the kink is what moves this gradient"
    want = plain_g if hip_active else flip_g
    for k, p_ in model.named_parameters():
        if np.linalg.norm(want[k]) < 1e-12:
            continue
        e = rel(p_.grad.cpu().numpy(), want[k])
        assert e < (1e-5 if k == key else 2e-4), f"{k}: {e:.2e} against the oracle on the HIP side of the kink (active={hip_active})"


def test_training_like_the_reference_tests():
    """reference tests/test_hypergnn.py:183-226 (backward runs, an SGD step changes parameters, the margin loss of
    demo.py:79-101 goes down under Adam) on the HIP path."""
    kg = ToyKnowledgeGraph(feat_dim=16)
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    torch.manual_seed(0)
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16, num_layers=2).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    before = {n: p.clone().detach() for n, p in model.named_parameters()}
    opt.zero_grad()
    model(x, ei, kg.edge_texts).sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    opt.step()
    assert sum(not torch.equal(before[n], p.detach()) for n, p in model.named_parameters()) > 0
    torch.manual_seed(1)
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16, num_layers=2).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    src, dst = ei
    losses = []
    for _ in range(15):
        opt.zero_grad()
        embs = model(x, ei, kg.edge_texts)
        pos = model.score_triple(embs[src], embs[dst])
        perm = torch.randperm(dst.size(0)).to(DEV)
        neg = model.score_triple(embs[src], embs[dst[perm]])
        loss = torch.clamp(1.0 - pos + neg, min=0.0).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    a = torch.randn(9, 16, device=DEV, requires_grad=True)
    b = torch.randn(9, 16, device=DEV, requires_grad=True)
    g = torch.randn(9, device=DEV)
    model.score_triple(a, b).backward(g)
    assert torch.allclose(a.grad, g[:, None] * b.detach()) and torch.allclose(b.grad, g[:, None] * a.detach())


@pytest.mark.parametrize("name", ["small", "c2", "c3"])
def test_captured_hip_graph_replays_the_forward(name):
    """HyperGNN.graphed: the warm forward captured into a HIP graph gives the eager result bit for bit, follows new
    features copied into its input and parameters updated in place."""
    cfg = cases.MODELS[name]
    g = synth.make_kg(1500, 12000, 6, cfg.node_feat_dim, seed=77, kind="powerlaw")
    model = make_model(cfg)
    x, ei, texts = torch.from_numpy(g.node_features).to(DEV), torch.from_numpy(g.edge_index).to(DEV), g.edge_texts()
    with torch.no_grad():
        eager = model(x, ei, texts).clone()
    graphed = model.graphed(x, ei, texts)
    assert torch.equal(graphed.replay(), eager)
    x2 = torch.from_numpy(synth.normal(78, "x2", tuple(x.shape))).to(DEV)
    with torch.no_grad():
        eager2 = model(x2, ei, texts).clone()
        assert not torch.equal(eager2, eager)
    assert torch.equal(graphed.replay(x2), eager2)
    with torch.no_grad():
        model.layer_norms[0].bias.add_(0.5)
        model.weight_generators[0].log_scales["W_msg"].add_(0.3)
        eager3 = model(x2, ei, texts).clone()
    assert torch.equal(graphed(), eager3) and not torch.equal(eager3, eager2)
    with pytest.raises(ValueError):
        graphed.replay(x2[:-1])


@pytest.mark.parametrize("d,N,E,R,kind", [(256, 700, 9000, 9, "uniform"), (256, 300, 20000, 5, "powerlaw"), (384, 90, 60, 7, "uniform"),
                                          (256, 1500, 1200, 40, "powerlaw")])
@pytest.mark.parametrize("exact,runs", [(False, False), (True, False), (False, True), (True, True)])
def test_wide_rows_layer_matches_oracle(d, N, E, R, kind, exact, runs, monkeypatch):
    """csrc/message_rs.hip (d % 128 == 0, d >= 256): per-edge results in relation order + destination sums + tail against
    the oracle and against the generic kernel; tiles shorter than 128 edges, relations without edges, hubs, isolated rows,
    row ranges, NO_TAIL and RAW_SUM.  runs: the rows of the two passes are runs of equal (destination, relation) whose
    source rows are summed first (long runs cut at RS_RUN_MAX — 16 here, so that the power-law hubs have cut runs); the
    exact kernel then runs the plan's per-edge twin."""
    from graph_hypernetwork_forge_amd import plan as plan_mod
    from graph_hypernetwork_forge_amd.plan import build_rs
    if exact:
        monkeypatch.setenv("GHF_KERNEL", "rs32")                         # pass 1 on fp32 MFMAs instead of two fp16 pieces
    ei, rel, h, Wm, Ws, b, gamma, beta = _layer_inputs(N, E, R, d, seed=11 + d + R, kind=kind)
    rel = np.where(rel == R - 1, 0, rel)                                # the last relation stays empty
    t = lambda a: torch.from_numpy(a).to(DEV)                           # noqa: E731
    th = torch.from_numpy
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    assert plan.block_nodes == 1 and _native.rs_supported(d)
    monkeypatch.setattr(plan_mod, "RS_HUB_ROWS", 700 if not runs else 150)   # a hub's rows in chunks at this size
    monkeypatch.setattr(plan_mod, "RS_RUN_MAX", 16)
    rs = build_rs(plan, runs=runs)
    if runs:
        key = ei[1].astype(np.int64) * R + rel
        _, n = np.unique(key, return_counts=True)
        assert rs.rows == int((-(-n // 16)).sum()) == int(rs.off[-1]) and rs.rows < E
        assert rs.run_start.numel() - 1 == int((n // 16 + (n % 16 >= 2)).sum()), "rows of two or more edges have a summed source row"
        assert abs(float(rs.cnt.sum()) - E) < 0.5
    else:
        assert rs.slice_tab.size(0) >= E // 128 and int(rs.off[-1]) == E and rs.run_start is None
    assert (rs.hub_of is not None) == (kind == "powerlaw" and E > 5000), "the power-law cases must exercise the hub path"
    Y = torch.full((rs.rows, d), float("nan"), device=DEV)
    _native.edge_transform_fwd(t(h), rs, t(Wm), t(Ws), t(b), Y)
    if not (exact and runs):                                            # (the exact kernel wrote its own per-edge results)
        assert bool(torch.isfinite(Y).all()), "every row of the per-row results is written"
    agg = O.message_passing_factorised(th(h), th(ei), th(rel), th(Wm), th(Ws), th(b))
    ref = O.layer_tail(agg, th(h), th(gamma), th(beta))
    out = torch.empty(N, d, device=DEV)
    hs_out = _native.alloc_split(N, d, _native.WLAYOUT_SPLIT2H, DEV)
    _native.segment_tail_fwd(Y, rs, t(h), t(gamma), t(beta), 1e-5, out, h_split_out=hs_out)
    assert_close(out.cpu().numpy(), ref.numpy(), "wide-row layer")
    assert torch.equal(hs_out, _native.split_rows(out, _native.WLAYOUT_SPLIT2H)), "pass 2's pieces = ghf_split_rows of its rows"
    again = torch.empty_like(out)
    _native.edge_transform_fwd(t(h), rs, t(Wm), t(Ws), t(b), Y)
    _native.segment_tail_fwd(Y, rs, t(h), t(gamma), t(beta), 1e-5, again)
    assert torch.equal(out, again)
    raw = torch.empty_like(out)
    _native.segment_tail_fwd(Y, rs, None, None, None, 0.0, raw, flags=_native.GHF_FLAG_NO_TAIL)
    assert_close(raw.cpu().numpy(), agg.numpy(), "wide-row layer, no tail")
    part = torch.full_like(out, 7.0)
    _native.segment_tail_fwd(Y, rs, t(h), t(gamma), t(beta), 1e-5, part, row0=N // 3, rows=N // 4)
    assert torch.equal(part[N // 3: N // 3 + N // 4], out[N // 3: N // 3 + N // 4]) and (part[: N // 3] == 7.0).all()
    gen = torch.empty_like(out)                                         # the generic kernel on the same plan
    _native.message_layer_fwd(t(h), plan, t(Wm), t(Ws), t(b), _native.WLAYOUT_NATURAL, t(gamma), t(beta), 1e-5, gen)
    assert_close(out.cpu().numpy(), gen.cpu().numpy(), "wide-row layer vs generic kernel")


def test_wide_rows_forward_and_sharding(monkeypatch):
    """HyperGNN.forward at hidden 256 takes the relation-stationary layer (and the generic one under GHF_KERNEL=generic);
    both equal the oracle, and the chunked multi-GPU driver gives the same rows (world-1 NCCL group)."""
    import torch.distributed as dist
    from graph_hypernetwork_forge_amd.dist import ShardedHyperGNN
    d, N, E, R = 256, 1300, 15000, 11
    g = synth.make_kg(N, E, R, 24, seed=5150, kind="powerlaw")
    params = synth.hypergnn_params(32, 24, d, 2, seed=9, log_scale=-0.5, randomize_ln=True)
    model = HyperGNN(32, 24, d, 2).to(DEV).eval()
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    x, ei, texts = torch.from_numpy(g.node_features).to(DEV), torch.from_numpy(g.edge_index).to(DEV), g.edge_texts()
    ref = O.forward(params, g.node_features, g.edge_index, texts, variant="factorised").numpy()
    with torch.no_grad():
        out = model(x, ei, texts)
        assert model.plan_for(ei, texts, N, DEV).rs is not None, "hidden 256 must take the relation-stationary layer"
        assert_close(out.cpu().numpy(), ref, "hidden 256 forward")
        monkeypatch.setenv("GHF_KERNEL", "generic")
        model.clear_plan_cache()
        assert_close(model(x, ei, texts).cpu().numpy(), ref, "hidden 256 forward, generic kernel")
        assert model.plan_for(ei, texts, N, DEV).rs is None
        monkeypatch.delenv("GHF_KERNEL")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29519")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        sharded = ShardedHyperGNN(model, chunks=3)(x, ei, texts)
        assert_close(sharded.cpu().numpy(), ref, "hidden 256, chunked driver")
    finally:
        dist.destroy_process_group()


def test_training_at_hidden_256():
    """A hidden size without destination-block kernels still trains (CSR plan, generic kernels in the recorded forward and
    the backward): every gradient against autograd through the float64 oracle."""
    d, N, E, R = 256, 200, 800, 5
    g = synth.make_kg(N, E, R, 16, seed=77, kind="powerlaw")
    params = synth.hypergnn_params(32, 16, d, 2, seed=3, log_scale=-0.5, randomize_ln=True)
    model = HyperGNN(32, 16, d, 2).to(DEV).train()
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    x, ei, texts = torch.from_numpy(g.node_features).to(DEV), torch.from_numpy(g.edge_index).to(DEV), g.edge_texts()
    gout = synth.normal(5, "g256", (N, d))
    out = model(x, ei, texts)
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    ref_p = {k: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True) for k, v in params.items()}
    ref = O.forward(ref_p, torch.from_numpy(g.node_features).double(), g.edge_index, texts, variant="factorised", dtype=torch.float64)
    (ref * torch.from_numpy(gout).double()).sum().backward()
    assert_close(out.detach().cpu().numpy(), ref.detach().float().numpy(), "hidden 256, recorded forward")
    for k, p in model.named_parameters():
        _grad_check(k, p.grad.cpu().numpy(), ref_p[k].grad.numpy())


def test_many_relations_take_the_relation_stationary_layer():
    """Hidden 128 with 200 relations: the inference plan is a CSR plan for csrc/message_rs.hip (the block kernel's time grows
    with the relation count), the plan of a forward that records gradients keeps the block geometry; both equal the oracle."""
    d, N, E, R = 128, 900, 20000, 200
    g = synth.make_kg(N, E, R, 16, seed=321, kind="uniform")
    params = synth.hypergnn_params(32, 16, d, 2, seed=12, log_scale=-0.5, randomize_ln=True)
    model = HyperGNN(32, 16, d, 2).to(DEV)
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    x, ei, texts = torch.from_numpy(g.node_features).to(DEV), torch.from_numpy(g.edge_index).to(DEV), g.edge_texts()
    ref = O.forward(params, g.node_features, g.edge_index, texts, variant="factorised").numpy()
    model.eval()
    with torch.no_grad():
        out = model(x, ei, texts)
    plan = model.plan_for(ei, texts, N, DEV)
    assert plan.block_nodes == 1 and plan.rs is not None
    assert_close(out.cpu().numpy(), ref, "hidden 128, 200 relations, inference")
    rec = model(x, ei, texts)                                           # parameters require grad: recorded forward
    assert rec.requires_grad and model.plan_for(ei, texts, N, DEV, training=True).block_nodes > 1
    assert_close(rec.detach().cpu().numpy(), ref, "hidden 128, 200 relations, recorded")
    rec.sum().backward()
    assert all(p.grad is not None for p in model.parameters())


def test_the_binding_shown_in_integration_md_runs():
    """INTEGRATION.md §2 is executable: its three code blocks, pasted onto modules that hold the reference's parameters
    under the reference's attribute names, reproduce the golden outputs through the C ABI alone."""
    import re
    import torch.nn as nn
    md = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", md, flags=re.S)
    binding = [b for b in blocks if "_ghf.py" in b.splitlines()[0]][0]
    fwd = [b for b in blocks if b.lstrip().startswith("# graph_hypernetwork_forge/models/hypergnn.py")][0]
    gen = [b for b in blocks if b.lstrip().startswith("# graph_hypernetwork_forge/models/weight_generator.py")][0]
    ns = {"nn": nn, "torch": torch}
    exec(binding.replace('"libghf_hip.so"', repr(_native.lib_path())), ns)
    exec(fwd, ns)
    exec(gen, ns)
    for name in ("g2_toy", "g3_mid32", "g6_c3"):
        (case,) = cases.graph_cases(only=[name])
        model = make_model(cases.MODELS[case.model])
        for g in model.weight_generators:
            g.generate_into = ns["generate_into"].__get__(g)
        with torch.no_grad():
            out = ns["forward"](model, torch.from_numpy(case.node_features).to(DEV), torch.from_numpy(case.edge_index).to(DEV),
                                case.edge_texts)
            ref = model(torch.from_numpy(case.node_features).to(DEV), torch.from_numpy(case.edge_index).to(DEV), case.edge_texts)
        assert_close(out.cpu().numpy(), ref.cpu().numpy(), f"INTEGRATION.md binding, {name}")


def test_row_range_only_touches_its_rows(kernel):
    d, N, E, R = 128, 2000, 20000, 16
    ei, rel, h, Wm, Ws, b, gamma, beta = _layer_inputs(N, E, R, d, seed=5, kind="uniform")
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    W = _pack_weights(plan, Wm, Ws)[0]
    full = torch.empty(N, d, device=DEV)
    _native.message_layer_fwd(t(h), plan, W, None, t(b), plan.wlayout, t(gamma), t(beta), 1e-5, full)
    part = torch.full((N, d), 7.0, device=DEV)
    bn = plan.block_nodes
    _native.message_layer_fwd(t(h), plan, W, None, t(b), plan.wlayout, t(gamma), t(beta), 1e-5, part, row0=2 * bn, rows=3 * bn)
    assert torch.equal(part[2 * bn:5 * bn], full[2 * bn:5 * bn])
    assert (part[:2 * bn] == 7.0).all() and (part[5 * bn:] == 7.0).all()


def test_message_passing_seam_per_edge_weights():
    """HyperGNN._message_passing keeps the reference's per-edge-weight signature (hypergnn.py:160-165)."""
    torch.manual_seed(3)
    N, E, d = 40, 150, 16
    h = torch.randn(N, d)
    ei = torch.randint(0, N, (2, E))
    rw = {"W_msg": torch.randn(E, d, d) * 0.2, "W_self": torch.randn(E, d, d) * 0.2, "bias": torch.randn(E, d)}
    model = make_model(cases.MODELS["small"])
    with torch.no_grad():
        out = model._message_passing(h.to(DEV), ei.to(DEV), {k: v.to(DEV) for k, v in rw.items()})
    ref = O.message_passing_reference_shaped(h, ei, rw["W_msg"], rw["W_self"], rw["bias"])
    assert_close(out.cpu().numpy(), ref.numpy(), "_message_passing")


# ---- behaviour contract of the drop-in (reference tests/test_hypergnn.py) ---------------------

def test_errors_and_cache():
    kg = ToyKnowledgeGraph(feat_dim=16)
    model = make_model(cases.MODELS["small"])
    x, ei = kg.node_features.to(DEV), kg.edge_index.to(DEV)
    with pytest.raises(ValueError):
        model(x, ei, kg.edge_texts[:-1])
    with pytest.raises(NotImplementedError):
        model.forward_planned(x, model.plan_for(ei, kg.edge_texts, x.size(0), DEV))   # explicit plans: inference only
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            model(kg.node_features, kg.edge_index, kg.edge_texts)     # CPU tensors: no fallback
    with torch.no_grad():
        a = model(x, ei, kg.edge_texts)
        b = model(x, ei, kg.edge_texts)
    assert model._plans.hits >= 1 and torch.equal(a, b)
    assert a.shape == (kg.num_nodes, model.hidden_dim) and torch.isfinite(a).all()


def test_relations_edited_in_place_follow_the_reference():
    """The reference maps the strings to ids on every call (hypergnn.py:264-268): editing one entry of the SAME list object
    between two forwards must change the result accordingly, not hit the cached plan."""
    (case,) = cases.graph_cases(only=["g3_mid32"])
    cfg = cases.MODELS[case.model]
    params = cfg.params()
    model = make_model(cfg, params)
    x, ei = torch.from_numpy(case.node_features).to(DEV), torch.from_numpy(case.edge_index).to(DEV)
    texts = list(case.edge_texts)
    with torch.no_grad():
        a = model(x, ei, texts)
        i = len(texts) // 2 + 3                                          # (not an end, not a strided position)
        texts[i] = next(t for t in texts if t != texts[i])               # that edge now carries another relation
        b = model(x, ei, texts)
    ref = O.forward(params, case.node_features, case.edge_index, texts, variant="factorised").numpy()
    assert_close(b.cpu().numpy(), ref, "after the in-place edit")
    assert not torch.equal(a, b)


def test_long_relation_list_edited_at_an_unsampled_position_follows_the_reference():
    """Beyond 2^17 edges the plan cache's key samples the list; the hit is then confirmed entry by entry on the host while the GPU
    runs the forward on the cached plan (HyperGNN.forward / plan.same_relations).  An in-place edit at a position the key does
    not sample must change the result as the reference's per-call id mapping would (hypergnn.py:264-268)."""
    from graph_hypernetwork_forge_amd import plan as plan_mod
    cfg = cases.MODELS["small"]
    params = cfg.params()
    model = make_model(cfg, params)
    N, E, R = 4000, 300_000, 9
    ei_np, rel = synth.make_graph_arrays(N, E, R, seed=41)
    names = [f"relation_{i:04d}" for i in range(R)]
    texts = [names[r] for r in rel.tolist()]
    x_np = synth.normal(41, "x", (N, cfg.node_feat_dim))
    x, ei = torch.from_numpy(x_np).to(DEV), torch.from_numpy(ei_np).to(DEV)
    with torch.no_grad():
        a = model(x, ei, texts)
        a2 = model(x, ei, texts)
        assert torch.equal(a, a2) and model._plans.hits >= 1 and model._plans.stale == 0
        sampled = set(plan_mod._SAMPLE_IDX[E][0])
        i = next(p for p in range(E // 2, E) if p not in sampled)
        texts[i] = names[(rel[i] + 1) % R]                                # that edge now carries another relation
        b = model(x, ei, texts)
        assert model._plans.stale == 1
        b2 = model(x, ei, texts)                                          # (the fresh plan is cached and verified in turn)
    assert torch.equal(b, b2) and not torch.equal(a, b)
    keep = ei_np[1] == ei_np[1][i]                                        # the edited edge's destination row, against the oracle
    rows = np.array([ei_np[1][i]])
    ref = O.forward(params, x_np, ei_np, texts, variant="factorised").numpy()
    assert_close(b.cpu().numpy()[rows], ref[rows], "the edited edge's destination row")
    assert_close(b.cpu().numpy(), ref, "after the in-place edit of a 300 k-entry list")
    assert keep.any()


def test_text_encoder_encode_one():
    """reference tests/test_hypergnn.py:44-63: encode_one gives [text_dim], equal strings equal rows, '' and non-ASCII work."""
    cfg = cases.MODELS["small"]
    enc = make_model(cfg).text_encoder
    with torch.no_grad():
        v = enc.encode_one("located_in", DEV)
        assert v.shape == (cfg.text_dim,) and torch.isfinite(v).all()
        assert torch.equal(v, enc.encode_one("located_in", DEV)) and not torch.equal(v, enc.encode_one("works_at", DEV))
        batch = enc(["located_in", "", "caf\u00e9"], DEV)
        assert torch.equal(batch[0], v) and torch.equal(batch[1], enc.encode_one("", DEV))
        assert torch.equal(batch[2], enc.encode_one("caf\u00e9", DEV))


def test_captured_graph_survives_cache_eviction():
    """A GraphedForward keeps the plan (and the token matrices) its captured launches point at: running other graphs through
    the model's small plan cache, and clearing it, must not change what a replay computes."""
    cfg = cases.MODELS["small"]
    model = make_model(cfg)
    kg0 = synth.make_kg(300, 2400, 5, cfg.node_feat_dim, seed=50)
    x0, ei0, t0 = torch.from_numpy(kg0.node_features).to(DEV), torch.from_numpy(kg0.edge_index).to(DEV), kg0.edge_texts()
    with torch.no_grad():
        want = model(x0, ei0, t0).clone()
    g = model.graphed(x0, ei0, t0)
    assert torch.equal(g.replay(), want)
    with torch.no_grad():
        for s in range(6):                                               # more graphs (and relation sets) than both LRUs hold
            kg = synth.make_kg(250 + 10 * s, 2000, 9 + s, cfg.node_feat_dim, seed=60 + s)
            texts = [t + f"_{s}" for t in kg.edge_texts()]
            model(torch.from_numpy(kg.node_features).to(DEV), torch.from_numpy(kg.edge_index).to(DEV), texts)
    model.clear_plan_cache()
    model.text_encoder._tokens.clear()
    junk = [torch.randn(1 << 20, device=DEV) for _ in range(8)]          # whatever was freed gets reused
    torch.cuda.synchronize()
    assert torch.equal(g.replay(), want)
    del junk


def _adversarial_model(d, F, rows_outlier=True):
    """A model whose first-layer input rows (or whose generated weights) carry one entry 2^30 above the rest, aimed at a
    zero partner: the case the two-fp16-piece kernels cannot hold and the fp32 reference can."""
    cfg = cases.ModelCfg(text_dim=16, node_feat_dim=F, hidden_dim=d, num_layers=2, seed=909, log_scale=0.0, randomize_ln=True)
    p = cfg.params()
    p["input_proj.weight"] = np.eye(d, F, dtype=np.float32)            # h0 = relu(x)
    p["input_proj.bias"] = np.zeros(d, np.float32)
    for l in range(cfg.num_layers):
        for head in ("W_msg", "W_self"):
            k = max(int(n.split(".")[4]) for n in p if n.startswith(f"weight_generators.{l}.generators.{head}."))
            W, b = p[f"weight_generators.{l}.generators.{head}.{k}.weight"], p[f"weight_generators.{l}.generators.{head}.{k}.bias"]
            if rows_outlier:
                if l == 0:                                              # input column 0 meets zero weights: rows [0, d) of the flat [d*d]
                    W[:d] = 0.0
                    b[:d] = 0.0
            elif l == 0 and head == "W_msg":
                b[5 * d + 7] = 2.0 ** 20                                # one weight (i = 5, o = 7) 2^20+ above the rest of its matrix
    return cfg, p


@pytest.mark.parametrize("d,what", [(128, "rows"), (128, "weights"), (256, "rows")])
def test_range_guard_routes_wide_inputs_to_the_exact_kernels(d, what, monkeypatch):
    """One feature 2^30 above the rest of its row whose weight rows are zero (rows), or one generated weight 2^20 above the
    rest of its matrix that only ever meets zeros (weights): two fp16 pieces lose the small entries, the reference's fp32
    bmm (hypergnn.py:202,228) does not.  The cutting kernels flag it, the forward repeats on the exact kernels and matches
    the oracle; with the guard off the result is visibly wrong (the test is not vacuous)."""
    F, N, E, R = d, 600, 5000, 5
    cfg, params = _adversarial_model(d, F, rows_outlier=what == "rows")
    kg = synth.make_kg(N, E, R, F, seed=31)
    x = np.abs(kg.node_features).astype(np.float32) + 0.1
    if what == "rows":
        x[::3, 0] *= 2.0 ** 30                                           # a third of the rows: column 0 dwarfs the rest
    else:
        x[:, 5] = -1.0                                                   # relu -> exactly 0: the huge weight's input column
    ei, texts = kg.edge_index, kg.edge_texts()
    ref = O.forward(params, x, ei, texts, variant="factorised").numpy()
    model = make_model(cfg, params)
    with torch.no_grad():
        out = model(torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV), texts)
    assert model.last_range_flags & (_native.RANGE_ROWS if what == "rows" else _native.RANGE_WEIGHTS)
    assert_close(out.cpu().numpy(), ref, f"guarded forward d={d} {what}")
    g = model.graphed(torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV), texts)      # the captured forward is guarded too
    assert_close(g.replay().cpu().numpy(), ref, f"guarded replay d={d} {what}")
    monkeypatch.setenv("GHF_RANGE_GUARD", "0")
    model2 = make_model(cfg, params)
    with torch.no_grad():
        raw = model2(torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV), texts)
    with pytest.raises(AssertionError):
        assert_close(raw.cpu().numpy(), ref, "unguarded")
    monkeypatch.delenv("GHF_RANGE_GUARD")
    # well-scaled inputs never trip it
    model3 = make_model(cfg, cfg.params())
    with torch.no_grad():
        model3(torch.from_numpy(kg.node_features).to(DEV), torch.from_numpy(ei).to(DEV), texts)
    assert model3.last_range_flags == 0


def _blind_spot_model(d, F, small, what):
    """The case the 1/8 rule does not see: only `small` of d entries (10 %) lie far below the rest.
    rows: layer 0's generated W_msg / W_self are zero on the LARGE input columns, so the far-down entries of an outlier row
    carry its whole message; weights: layer 0's matrices are 2^30 larger on input rows >= small, which only ever meet zeros."""
    cfg = cases.ModelCfg(text_dim=16, node_feat_dim=F, hidden_dim=d, num_layers=2, seed=911, log_scale=0.0, randomize_ln=True)
    p = cfg.params()
    p["input_proj.weight"] = np.eye(d, F, dtype=np.float32)            # h0 = relu(x)
    p["input_proj.bias"] = np.zeros(d, np.float32)
    for head in ("W_msg", "W_self"):
        k = max(int(n.split(".")[4]) for n in p if n.startswith(f"weight_generators.0.generators.{head}."))
        W, b = p[f"weight_generators.0.generators.{head}.{k}.weight"], p[f"weight_generators.0.generators.{head}.{k}.bias"]
        if what == "rows":
            W[small * d:] = 0.0                                        # flat [d*d] = [input k][output o]: rows k >= small
            b[small * d:] = 0.0
        else:
            W[small * d:] *= 2.0 ** 30
            b[small * d:] *= 2.0 ** 30
    return cfg, p


@pytest.mark.parametrize("d,what", [(128, "rows"), (128, "weights"), (256, "rows"), (256, "weights")])
def test_range_guard_has_no_blind_spot_below_one_eighth(d, what, monkeypatch):
    """10 % of a row's (of a relation matrix's) entries 2^30 below the rest, the large ones meeting zeros: fewer than the 1/8
    GHF_RANGE_ROWS / GHF_RANGE_WEIGHTS count, and still a case two fp16 pieces cannot hold while the reference's fp32 bmm
    (hypergnn.py:202,228) can.  GHF_RANGE_WEAK_W (a relation matrix with an input row far below the others: include/ghf.h
    states the bound that holds without one) routes it to the exact kernels; with the guard off the result is wrong."""
    F, N, E, R = d, 600, 5000, 5
    small = d // 10
    cfg, params = _blind_spot_model(d, F, small, what)
    kg = synth.make_kg(N, E, R, F, seed=37)
    x = np.abs(kg.node_features).astype(np.float32) + 0.1
    if what == "rows":
        x[::3, small:] *= 2.0 ** 30                                      # a third of the rows: 90 % of the columns dwarf the rest
    else:
        x[:, small:] = -1.0                                              # relu -> exactly 0 where the huge weights are
    ei, texts = kg.edge_index, kg.edge_texts()
    ref = O.forward(params, x, ei, texts, variant="factorised").numpy()
    model = make_model(cfg, params)
    with torch.no_grad():
        out = model(torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV), texts)
    assert model.last_range_flags & _native.RANGE_WEAK_W
    if what == "rows" or d == 128:       # (wide rows: ghf_weights_pack_rs counts per 32 x 32 tile, and the tiles of the small rows do see them)
        assert not model.last_range_flags & (_native.RANGE_ROWS if what == "rows" else _native.RANGE_WEIGHTS), "built to stay under the 1/8 count"
    assert_close(out.cpu().numpy(), ref, f"guarded forward d={d} {what}")
    monkeypatch.setenv("GHF_RANGE_GUARD", "0")
    model2 = make_model(cfg, params)
    with torch.no_grad():
        raw = model2(torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV), texts)
    with pytest.raises(AssertionError):
        assert_close(raw.cpu().numpy(), ref, "unguarded")
    monkeypatch.delenv("GHF_RANGE_GUARD")
    # the same rows on generic weights (no weak input row): no bit, and the two-piece kernels are within tolerance although
    # 10 % of those rows' entries lie 2^30 down — the bound of ghf.h
    if what == "rows":
        cfg3 = cases.ModelCfg(text_dim=16, node_feat_dim=F, hidden_dim=d, num_layers=2, seed=911, log_scale=0.0, randomize_ln=True)
        p3 = cfg3.params()
        p3["input_proj.weight"], p3["input_proj.bias"] = np.eye(d, F, dtype=np.float32), np.zeros(d, np.float32)
        model3 = make_model(cfg3, p3)
        with torch.no_grad():
            out3 = model3(torch.from_numpy(x).to(DEV), torch.from_numpy(ei).to(DEV), texts)
        assert model3.last_range_flags == 0
        assert_close(out3.cpu().numpy(), O.forward(p3, x, ei, texts, variant="factorised").numpy(), f"generic weights d={d}")


def test_forward_ids_equals_forward(golden_dir):
    """The pre-tokenised overload (relation ids + one string per relation) gives the forward's result."""
    (case,) = cases.graph_cases(only=["g3_mid32"])
    model = make_model(cases.MODELS[case.model])
    x, ei = torch.from_numpy(case.node_features).to(DEV), torch.from_numpy(case.edge_index).to(DEV)
    unique, ids = relation_ids(case.edge_texts)
    with torch.no_grad():
        a = model(x, ei, case.edge_texts)
        b = model.forward_ids(x, ei, torch.from_numpy(ids).to(DEV), unique)
        c = model.forward_ids(x, ei, torch.from_numpy(ids).to(DEV), unique)
        ids_d = torch.from_numpy(ids).to(DEV)
        hits = model._plans.hits
        d = model.forward_ids(x, ei, ids_d, unique)
        e = model.forward_ids(x, ei, ids_d, unique)
        assert model._plans.hits == hits + 1                         # same tensors: the plan is reused
        assert torch.equal(a, b) and torch.equal(b, c) and torch.equal(c, d) and torch.equal(d, e)
        with pytest.raises(ValueError):
            model.forward_ids(x, ei, ids_d[:-1], unique)
        with pytest.raises(IndexError):
            model.forward_ids(x, ei, ids_d + len(unique), unique)


def test_relation_order_does_not_matter():
    """Relabelling relations / shuffling edges only permutes W[r] and the summation order."""
    (case,) = cases.graph_cases(only=["g6_c3"])
    model = make_model(cases.MODELS[case.model])
    x = torch.from_numpy(case.node_features).to(DEV)
    perm = np.argsort(synth.raw_u64(9, "shuffle", case.edge_index.shape[1]), kind="stable")
    with torch.no_grad():
        a = model(x, torch.from_numpy(case.edge_index).to(DEV), case.edge_texts)
        b = model(x, torch.from_numpy(np.ascontiguousarray(case.edge_index[:, perm])).to(DEV),
                  [case.edge_texts[i] for i in perm.tolist()])
    assert_close(b.cpu().numpy(), a.cpu().numpy(), "edge shuffle")


# ---- BASELINE config 3 at full size: size-independent properties + sampled rows vs the oracle --

@pytest.mark.parametrize("N,E,R,d", [(1_000_000, 10_000_000, 64, 128), (500_000, 5_000_000, 32, 64)])
def test_full_size_c3_layer_properties(N, E, R, d, kernel):
    """BASELINE config 3, and config 2's shape grown to where hidden 64 takes the two-piece kernel by default
    (plan.D64_PIECES_MIN_EDGES)."""
    _skip_unless_kernel_exists(kernel, d)
    ei, rel = synth.make_graph_arrays(N, E, R, seed=1003)
    g = torch.Generator(device="cpu").manual_seed(1)
    h = torch.randn(N, d, generator=g)
    Wm, Ws = synth.normal(11, "Wm", (R, d, d), std=0.1), synth.normal(11, "Ws", (R, d, d), std=0.1)
    b = synth.normal(11, "b", (R, d), std=0.3)
    gamma, beta = np.ones(d, np.float32), np.zeros(d, np.float32)
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    assert plan.E == E and int(plan.indeg.sum().item()) == E
    W = _pack_weights(plan, Wm, Ws)[0]
    h_d = h.to(DEV)
    out1, out2 = torch.empty_like(h_d), torch.empty_like(h_d)
    args = (h_d, plan, W, None, t(b), plan.wlayout, t(gamma), t(beta), 1e-5)
    _native.message_layer_fwd(*args, out1)
    _native.message_layer_fwd(*args, out2)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2), "the block kernels must be bitwise reproducible"
    assert torch.isfinite(out1).all()
    # LayerNorm rows: zero mean, unit (biased) variance
    assert out1.mean(dim=1).abs().max().item() < 1e-4
    assert (out1.var(dim=1, unbiased=False) - 1).abs().max().item() < 1e-2
    # nodes without in-edges: exactly LayerNorm(ReLU(h))
    iso = (plan.indeg == 0).nonzero().flatten()[:4096]
    assert iso.numel() > 0
    want = torch.nn.functional.layer_norm(torch.relu(h_d[iso]), (d,), t(gamma), t(beta), 1e-5)
    assert_close(out1[iso].cpu().numpy(), want.cpu().numpy(), "isolated rows")
    # sampled destination rows against the oracle on their in-edge subgraph
    rows = np.unique(synth.randint(5, "rows", 300, N))
    keep = np.isin(ei[1], rows)
    sub_ei, sub_rel = ei[:, keep], rel[keep]
    th = torch.from_numpy
    ref = O.message_passing_factorised(h, th(sub_ei), th(sub_rel), th(Wm), th(Ws), th(b))
    ref = O.layer_tail(ref, h, th(gamma), th(beta))[rows]
    assert_close(out1[t(rows)].cpu().numpy(), ref.numpy(), f"sampled rows of the {E // 1_000_000}M-edge layer")


@pytest.mark.parametrize("N,E,R,d,launches", [(1_000_000, 10_000_000, 64, 128, 5), (500_000, 5_000_000, 32, 64, 8),
                                              (100_000, 1_000_000, 32, 64, 8)])
def test_block_kernel_is_bitwise_reproducible_over_a_few_launches(N, E, R, d, launches, monkeypatch):
    """A smoke check, not a proof: the two-piece block kernel at full size gives the same bits launch after launch (rows in
    order, chunks in order, no atomics).  Round 3's race in the hidden-64 instance was found by a long version of this loop and
    closed in round 4 by its cause (csrc/message_bx.hip, "The indexing mode's switch": profiles/r04_hazard_bisect.txt) — the
    correctness gates are the oracle comparisons (test_forward_c2_full_size_default_kernel, test_full_size_c3_layer_properties,
    test_hidden_64_gradient_pass_instances_match_the_oracle_at_half_a_million_edges)."""
    monkeypatch.setenv("GHF_KERNEL", "bx")
    ei, rel = synth.make_graph_arrays(N, E, R, seed=1003)
    h = torch.randn(N, d, generator=torch.Generator(device="cpu").manual_seed(1)).to(DEV)
    Wm, Ws = synth.normal(11, "Wm", (R, d, d), std=0.1), synth.normal(11, "Ws", (R, d, d), std=0.1)
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    assert plan.wlayout == _native.WLAYOUT_SPLIT2H
    W = _pack_weights(plan, Wm, Ws)[0]
    hs = _native.split_rows(h, plan.wlayout)
    args = (h, plan, W, None, t(synth.normal(11, "b", (R, d), std=0.3)), plan.wlayout, t(np.ones(d, np.float32)),
            t(np.zeros(d, np.float32)), 1e-5)
    first, out = torch.empty_like(h), torch.empty_like(h)
    _native.message_layer_fwd(*args, first, h_split=hs)
    differing = 0
    for _ in range(launches):
        _native.message_layer_fwd(*args, out, h_split=hs)
        differing += int((out != first).any().item())
    assert differing == 0, f"{differing} of {launches} launches differ from the first"


def test_hidden_64_default_kernel_follows_the_graph_size(monkeypatch):
    """plan.D64_PIECES_MIN_EDGES: small graphs keep the exact kernel (no range-guard sync), large ones take two fp16 pieces."""
    from graph_hypernetwork_forge_amd import plan as plan_mod
    monkeypatch.delenv("GHF_KERNEL", raising=False)
    ei, rel = synth.make_graph_arrays(3000, 20000, 5, seed=3)
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    assert build_plan(t(ei), t(rel), [""] * 5, 3000, 64, DEV).wlayout == _native.WLAYOUT_FRAG16
    monkeypatch.setattr(plan_mod, "D64_PIECES_MIN_EDGES", 10_000)
    big = build_plan(t(ei), t(rel), [""] * 5, 3000, 64, DEV)
    assert (big.wlayout, big.block_nodes) == (_native.WLAYOUT_SPLIT2H, 192)


@pytest.mark.parametrize("runs", [False, None])
def test_full_size_c5_shard_properties(runs):
    """One GPU's share of BASELINE config 5 (power-law KG, 4 M rows resident, 8 M in-edges owned, 256 relations, hidden 256)
    through the relation-stationary layer — with the graph's real hubs (in-degrees far above plan.RS_HUB_ROWS, no patched
    threshold): bitwise reproducible, LayerNorm moments, isolated rows, and sampled rows INCLUDING the hubs against a
    float64 evaluation of their in-edge subgraph (reference statement: models/hypergnn.py:201-230, 288-296).  runs=False: one
    row per edge, the hubs' rows summed in chunks; runs=None: what the plan picks for this graph — one row per run of equal
    (destination, relation), the hubs' source rows summed first."""
    from graph_hypernetwork_forge_amd import plan as plan_mod
    N, E, R, d = 4_000_000, 8_000_000, 256, 256
    ei, rel = synth.make_graph_arrays(N, E, R, seed=1005, kind="powerlaw")
    t = lambda a: torch.from_numpy(a).to(DEV)                                             # noqa: E731
    plan = build_plan(t(ei), t(rel), [""] * R, N, d, DEV)
    assert plan.block_nodes == 1 and plan.E == E and _native.rs_supported(d)
    rs = plan_mod.build_rs(plan, runs=runs)
    deg = np.bincount(ei[1], minlength=N)
    hubs = np.argsort(deg)[-3:]
    assert deg[hubs].min() > 4 * plan_mod.RS_HUB_ROWS, "this shard must hold real hubs"
    if runs is False:
        assert rs.hub_of is not None and rs.run_start is None and rs.rows == E
    else:
        assert rs.run_start is not None and rs.rows <= plan_mod.RS_RUNS_MAX_SHARE * E, "a power-law shard's plan sums its runs first"
    g = torch.Generator(device="cpu").manual_seed(2)
    h = torch.randn(N, d, generator=g)
    Wm, Ws = synth.normal(12, "Wm", (R, d, d), std=0.05), synth.normal(12, "Ws", (R, d, d), std=0.05)
    b = synth.normal(12, "b", (R, d), std=0.3)
    gamma, beta = np.ones(d, np.float32), np.zeros(d, np.float32)
    h_d, Wm_d, Ws_d, b_d = h.to(DEV), t(Wm), t(Ws), t(b)
    Y = rs.scratch(E, d, DEV)
    outs = []
    for _ in range(2):
        out = torch.empty_like(h_d)
        _native.edge_transform_fwd(h_d, rs, Wm_d, Ws_d, b_d, Y)
        _native.segment_tail_fwd(Y, rs, h_d, t(gamma), t(beta), 1e-5, out)
        outs.append(out)
    torch.cuda.synchronize()
    out1 = outs[0]
    assert torch.equal(out1, outs[1]), "the relation-stationary layer must be bitwise reproducible"
    assert torch.isfinite(out1).all()
    assert out1.mean(dim=1).abs().max().item() < 1e-4
    assert (out1.var(dim=1, unbiased=False) - 1).abs().max().item() < 1e-2
    iso = (plan.indeg == 0).nonzero().flatten()[:4096]
    assert iso.numel() > 0
    want = torch.nn.functional.layer_norm(torch.relu(h_d[iso]), (d,), t(gamma), t(beta), 1e-5)
    assert_close(out1[iso].cpu().numpy(), want.cpu().numpy(), "isolated rows")
    # sampled destinations + the three largest hubs, in float64 on their in-edge subgraph
    rows = np.unique(np.concatenate([synth.randint(6, "rows", 200, N), hubs]))
    keep = np.isin(ei[1], rows)
    s_src, s_dst, s_rel = (torch.from_numpy(a[keep]) for a in (ei[0], ei[1], rel))
    pos = torch.full((N,), -1, dtype=torch.int64)
    pos[torch.from_numpy(rows)] = torch.arange(len(rows))
    acc = torch.zeros(len(rows), d, dtype=torch.float64)
    for r in torch.unique(s_rel).tolist():
        e = (s_rel == r).nonzero().flatten()
        c = (h[s_src[e]].double() @ torch.from_numpy(Wm[r]).double() + torch.from_numpy(b[r]).double()
             + h[s_dst[e]].double() @ torch.from_numpy(Ws[r]).double())
        acc.index_add_(0, pos[s_dst[e]], c)
    cnt = torch.from_numpy(np.maximum(deg[rows], 1)).double()[:, None]
    x = torch.relu(acc / cnt + h[torch.from_numpy(rows)].double())
    ref = torch.nn.functional.layer_norm(x, (d,), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), 1e-5)
    assert_close(out1[t(rows)].cpu().numpy(), ref.numpy(), f"sampled rows and hubs (in-degrees {deg[hubs].tolist()}) of the C5 shard")


# ---- the multi-GPU driver on one GPU: NCCL world of 1, 4 overlapped chunks ------------------------------

def _adversarial_graph(d):
    """Inputs and model of test_range_guard_routes_wide_inputs_to_the_exact_kernels (rows)."""
    cfg, params = _adversarial_model(d, d, rows_outlier=True)
    kg = synth.make_kg(600, 5000, 5, d, seed=31)
    x = np.abs(kg.node_features).astype(np.float32) + 0.1
    x[::3, 0] *= 2.0 ** 30
    return cfg, params, x, kg.edge_index, kg.edge_texts()


def _two_rank_worker(rank, world, port, name, ret, kw):
    import torch.distributed as dist
    from graph_hypernetwork_forge_amd.dist import ShardedHyperGNN
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        if name.startswith("adversarial"):
            cfg, params, feats, ei_np, texts = _adversarial_graph(int(name.split(":")[1]))
            model = make_model(cfg, params)
        elif name == "c2_full":
            cfg = cases.MODELS["c2"]
            kg = synth.make_kg(100_000, 1_000_000, 32, cfg.node_feat_dim, 1002, "uniform")
            model = make_model(cfg)
            feats, ei_np, texts = kg.node_features, kg.edge_index, kg.edge_texts()
        else:
            (case,) = cases.graph_cases(only=[name])
            model = make_model(cases.MODELS[case.model])
            feats, ei_np, texts = case.node_features, case.edge_index, case.edge_texts
        runner = ShardedHyperGNN(model, chunks=3, **kw)                  # the product ops: HIP kernels on every rank
        x, ei = torch.from_numpy(feats).to(DEV), torch.from_numpy(ei_np).to(DEV)
        out = runner(x, ei, texts)
        out2 = runner(x, ei, texts)
        torch.cuda.synchronize()
        assert torch.equal(out, out2)
        ret[rank] = (out.cpu().numpy(), runner.last_range_flags, runner._plan.E)
    finally:
        dist.destroy_process_group()


def _run_ranks(world, name, kw):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ret = mp.get_context("spawn").Manager().dict()
    mp.spawn(_two_rank_worker, args=(world, port, name, ret, kw), nprocs=world, join=True)
    assert sorted(ret.keys()) == list(range(world))
    return [ret[r] for r in range(world)]


@pytest.mark.parametrize("name,world,kw", [
    ("g6_c3", 2, {}), ("g5_c2", 3, {}), ("g6_c3", 3, {}),
    # BASELINE config 4 as written: contiguous edge ranges, raw partial sums of ALL rows from the product kernels
    # (GHF_FLAG_RAW_SUM on an edge_range plan: blocks without edges on a rank must come out zero, split blocks combine
    # under a rank-local in-degree), reduction, mean + tail on the owned rows, all-gather
    ("g6_c3", 2, dict(mode="edges")), ("g6_c3", 3, dict(mode="edges")), ("g5_c2", 2, dict(mode="edges")),
    ("g6_c3_powerlaw", 2, dict(mode="edges")), ("g7_c5", 2, dict(mode="edges")),
    # every rank sends its slot straight to each peer; slots of about equal in-edge counts on a power-law graph
    ("g6_c3", 2, dict(exchange="pairs")), ("g5_c2", 3, dict(exchange="pairs")),
    ("g6_c3_powerlaw", 3, dict(balance="edges")), ("g6_c3_powerlaw", 2, dict(balance="edges")), ("g7_c5", 2, dict(balance="edges")),
    # needed rows only (plan-time row lists per chunk and peer; gather-pack, send/recv, scatter); the last layer whole
    ("g6_c3", 2, dict(exchange="sparse")), ("g5_c2", 3, dict(exchange="sparse")), ("g6_c3_powerlaw", 3, dict(exchange="sparse", balance="edges")),
    ("g7_c5", 2, dict(exchange="sparse")),
])
def test_sharded_forward_multi_rank_on_one_gpu(golden_dir, name, world, kw):
    """The whole multi-rank product path — ownership-filtered (or edge-range) plans, chunked launches, per-layer exchange
    (of the split rows the fused tails write at d = 128, of fp32 rows plus a re-split at d = 64, of raw partial sums in
    mode="edges") — with real HIP kernels on every rank: `world` processes share this GPU and exchange through gloo (NCCL
    refuses two ranks on one device); every rank must reproduce the reference (BASELINE configs 3-5)."""
    g = np.load(os.path.join(golden_dir, f"{name}.npz"))
    res = _run_ranks(world, name, kw)
    if kw.get("mode") == "edges":
        (case,) = cases.graph_cases(only=[name])
        assert sum(r[2] for r in res) == case.edge_index.shape[1] and min(r[2] for r in res) > 0, "every rank holds a range of the edges"
    for r in range(world):
        if "out" in g:
            assert_close(res[r][0], g["out"], f"{name} world={world} {kw} rank={r}")
        else:
            assert_close(res[r][0][g["rows"]], g["out_rows"], f"{name} world={world} {kw} rank={r} rows")
        assert np.array_equal(res[r][0], res[0][0])
        assert res[r][1] == 0


@pytest.mark.parametrize("kw", [{}, dict(mode="edges")])
def test_sharded_forward_at_config_2_size(kw):
    """Two ranks on BASELINE config 2 at its own size: every rank's shard (0.5 M edges each) runs message_bx<64>, the kernel the
    single-GPU C2 forward takes; every row against the oracle."""
    c = _c2_full()
    res = _run_ranks(2, "c2_full", kw)
    for r in range(2):
        assert_close(res[r][0], c["ref"], f"config 2 sharded {kw} rank={r}")
        assert np.array_equal(res[r][0], res[0][0]) and res[r][1] == 0


@pytest.mark.parametrize("d,kw", [(128, {}), (128, dict(mode="edges")), (256, {})])
def test_sharded_forward_falls_back_collectively_when_the_range_guard_fires(d, kw):
    """Rows the two-fp16-piece kernels cannot hold (one feature 2^30 above the rest, meeting zero weights): the single-GPU
    forward reruns on the exact kernels, and so does the sharded one — the guard word is reduced over the ranks, every rank
    plans the same shards for the exact kernels and runs again (reference: plain fp32 bmm, hypergnn.py:202,228)."""
    cfg, params, x, ei, texts = _adversarial_graph(d)
    ref = O.forward(params, x, ei, texts, variant="factorised").numpy()
    res = _run_ranks(2, f"adversarial:{d}", kw)
    for r in range(2):
        assert res[r][1] & _native.RANGE_ROWS, "the guard must have fired on some rank and be seen on every rank"
        assert_close(res[r][0], ref, f"sharded fallback d={d} {kw} rank={r}")
        assert np.array_equal(res[r][0], res[0][0])


def test_block_kernel_rows_beyond_two_gib():
    """message_bx addressed the split rows with byte offsets that had to stay below 2 GiB (N <= 4.16 M at
    d = 128).  They now reach 4 GiB - 4 KiB: a graph of 4.3 M nodes whose edges all start in the rows beyond 2 GiB, sampled
    destinations against a float64 evaluation (reference statement: models/hypergnn.py:201-230, 288-296)."""
    N, E, R, d = 4_300_000, 1_000_000, 16, 128
    assert N * (4 * d + 4) > 2 ** 31
    hi0 = (2 ** 31) // (4 * d) + 1000                                   # first row wholly beyond 2 GiB of split rows
    src = hi0 + synth.randint(21, "src", E, N - hi0)
    dst = np.concatenate([synth.randint(21, "dst", E // 2, 200_000), hi0 + synth.randint(21, "dst2", E - E // 2, N - hi0)])
    rel = synth.randint(21, "rel", E, R)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)    # noqa: E731
    plan = build_plan(t(np.stack([src, dst])), t(rel), [""] * R, N, d, DEV)
    assert plan.block_nodes == 384 and plan.wlayout == _native.WLAYOUT_SPLIT2H
    g = torch.Generator(device="cpu").manual_seed(4)
    h = torch.randn(N, d, generator=g)
    Wm, Ws = synth.normal(13, "Wm", (R, d, d), std=0.08), synth.normal(13, "Ws", (R, d, d), std=0.08)
    b = synth.normal(13, "b", (R, d), std=0.3)
    gamma, beta = np.ones(d, np.float32), np.zeros(d, np.float32)
    h_d = h.to(DEV)
    W = _native.weights_pack(t(Wm), t(Ws), False, R, d, _native.WLAYOUT_SPLIT2H)
    out = torch.empty_like(h_d)
    _native.message_layer_fwd(h_d, plan, W, None, t(b), plan.wlayout, t(gamma), t(beta), 1e-5, out)
    torch.cuda.synchronize()
    rows = np.unique(np.concatenate([dst[:150], dst[-150:]]))
    keep = np.isin(dst, rows)
    s_src, s_dst, s_rel = (torch.from_numpy(a[keep]) for a in (src, dst, rel))
    pos = torch.full((N,), -1, dtype=torch.int64)
    pos[torch.from_numpy(rows)] = torch.arange(len(rows))
    acc = torch.zeros(len(rows), d, dtype=torch.float64)
    for r in torch.unique(s_rel).tolist():
        e = (s_rel == r).nonzero().flatten()
        c = (h[s_src[e]].double() @ torch.from_numpy(Wm[r]).double() + torch.from_numpy(b[r]).double()
             + h[s_dst[e]].double() @ torch.from_numpy(Ws[r]).double())
        acc.index_add_(0, pos[s_dst[e]], c)
    cnt = torch.from_numpy(np.maximum(np.bincount(dst, minlength=N)[rows], 1)).double()[:, None]
    xr = torch.relu(acc / cnt + h[torch.from_numpy(rows)].double())
    ref = torch.nn.functional.layer_norm(xr, (d,), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), 1e-5)
    assert_close(out[t(rows)].cpu().numpy(), ref.numpy(), "rows whose sources lie beyond 2 GiB of split rows")


def test_sharded_driver_single_rank_nccl(golden_dir):
    """Exercises dist.ShardedHyperGNN's chunked launches, side-stream in-place all-gathers and plan ownership
    filter on real hardware (world_size 1); the multi-rank logic is covered on CPU by tests/test_dist_gloo.py."""
    import torch.distributed as dist
    from graph_hypernetwork_forge_amd.dist import ShardedHyperGNN
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        for name in ("g6_c3", "g5_c2"):
            (case,) = cases.graph_cases(only=[name])
            g = np.load(os.path.join(golden_dir, f"{name}.npz"))
            model = make_model(cases.MODELS[case.model])
            runner = ShardedHyperGNN(model, chunks=4)
            x, ei = torch.from_numpy(case.node_features).to(DEV), torch.from_numpy(case.edge_index).to(DEV)
            out = runner(x, ei, case.edge_texts)
            out2 = runner(x, ei, case.edge_texts)
            torch.cuda.synchronize()
            assert runner._spec.chunks == 4 and torch.equal(out, out2)
            if "out" in g:
                assert_close(out.cpu().numpy(), g["out"], f"sharded {name}")
            else:
                assert_close(out.cpu().numpy()[g["rows"]], g["out_rows"], f"sharded {name} rows")
    finally:
        dist.destroy_process_group()
