"""The any-width route's cases, checked on the host (test_any_width_gpu.py runs them): at every width the CSR catalogue without
its hub case is what it claims, the float64 references equal the oracle, and the float32 oracle itself lands within half of the
project's bounds — forward at every width, all six gradients at the widths that are differentiated — so a kernel that misses a
bound on such a case is wrong, not unlucky.  Also the arithmetic the GPU file's choice of widths rests on: which widths leave
one live wave, one live thread in the last column group, a fourth column group; which NT give which TG; where W_in is staged in
LDS."""

import numpy as np
import pytest
import torch

import _edge_graphs as G
from _util import ATOL, REL_L2, RTOL
from oracle import hypergnn_oracle as O

CASE_NAMES = [c.name for c in G.any_width_cases()]
PAIRS = [(d, n) for d in G.ANY_FWD_WIDTHS for n in CASE_NAMES]


def test_the_catalogue_and_the_seeds_on_record():
    cases = G.any_width_cases()
    assert CASE_NAMES == ["csr_in_degrees", "csr_relation_sizes_around_the_tile", "csr_runs_around_run_max",
                          "csr_duplicates_and_self_loops", "csr_n1_self_loop", "csr_n2_one_edge"]
    assert [c.name for c in G.edge_cases(1, 0, 0, 0, 100)] == CASE_NAMES[:3] + [G.ANY_NO_HUBS] + CASE_NAMES[3:]
    indeg = np.bincount(cases[0].edge_index[1], minlength=cases[0].N)
    assert {0, 1, 2, 63, 64, 65, 300} <= set(indeg.tolist())          # (what the hub case would add is in-degree alone)
    assert max(c.rel.size for c in cases) <= 800 and set(G.ANY_BWD_WIDTHS) <= set(G.ANY_FWD_WIDTHS)
    assert {1, 2}.isdisjoint(G.ANY_BWD_WIDTHS)
    for (key, name), seed in G.SEED_OVERRIDES.items():
        if key.startswith("any"):
            assert int(key[3:]) in G.ANY_FWD_WIDTHS and name in CASE_NAMES and 7100 <= seed <= 7107, (key, name, seed)


def _oracle(case, d, seed, dtype, grads):
    th = torch.from_numpy
    ins = [th(a).to(dtype).requires_grad_(grads) for a in G.layer_inputs(case, d, seed)]
    h, Wm, Ws, b, gamma, beta = ins
    agg = O.message_passing_factorised(h, th(case.edge_index), th(case.rel), Wm, Ws, b)
    out = O.layer_tail(agg, h, gamma, beta)
    if grads:
        out.backward(th(G.synth.normal(77, "gout", (case.N, d))).to(dtype))
    return agg.detach().numpy(), out.detach().numpy(), [t.grad.numpy() for t in ins] if grads else None


def _ref64(case, d, seed, grads):
    th = torch.from_numpy
    ins = [th(a).double().requires_grad_(grads) for a in G.layer_inputs(case, d, seed)]
    agg, out = G.layer_ref64_torch(ins[0], th(case.edge_index), th(case.rel), *ins[1:])
    if grads:
        out.backward(th(G.synth.normal(77, "gout", (case.N, d))).double())
    return agg.detach().numpy(), out.detach().numpy(), [t.grad.numpy() for t in ins] if grads else None


def _share(got, ref, rtol, atol, l2):
    """The largest share of the bounds (rtol, atol; relative L2) that `got` uses."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rel = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
    return max(float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max()), rel / l2)


def admissibility(d, name, seed):
    """Asserts the references equal the oracle; returns {quantity: share of HALF the bound the float32 oracle uses}."""
    (case,) = [c for c in G.any_width_cases() if c.name == name]
    grads = d in G.ANY_BWD_WIDTHS
    G.realised(case, 1, 0, 0, 0)
    h, Wm, Ws, b, gamma, beta = G.layer_inputs(case, d, seed)
    agg_np, out_np = G.layer_ref64(h, case.edge_index, case.rel, Wm, Ws, b, gamma, beta)
    agg64, out64, g64 = _ref64(case, d, seed, grads)
    o_agg, o_out, o_g = _oracle(case, d, seed, torch.float64, grads)
    for what, a, want in (("out", agg_np, o_agg), ("h'", out_np, o_out), ("out (torch)", agg64, o_agg), ("h' (torch)", out64, o_out)):
        assert np.allclose(a, want, rtol=1e-12, atol=1e-12), f"{what}: max abs diff {np.abs(a - want).max():.3e}"
    names = ("h", "W_msg", "W_self", "bias", "gamma", "beta")
    if grads:
        for n, a, want in zip(names, g64, o_g):
            assert np.allclose(a, want, rtol=1e-11, atol=1e-12 * max(np.abs(want).max(), 1.0)), f"d{n}: {np.abs(a - want).max():.3e}"
    f_agg, f_out, f_g = _oracle(case, d, seed, torch.float32, grads)
    shares = {"out": _share(f_agg, agg_np, RTOL / 2, ATOL / 2, REL_L2 / 2), "h'": _share(f_out, out_np, RTOL / 2, ATOL / 2, REL_L2 / 2)}
    # the tail under the dropout mask the GPU file applies (other rows of LayerNorm input: conditioned on their own)
    mask = G.dropout_mask(case.N, d)
    assert np.allclose(G.tail_ref64(agg_np, h, gamma, beta), out_np, rtol=1e-12, atol=1e-12)
    th = torch.from_numpy
    f_drop = O.layer_tail(th(f_agg), th(h), th(gamma), th(beta), drop=mask).numpy()
    shares["h' (dropout)"] = _share(f_drop, G.tail_ref64(agg_np, h, gamma, beta, mask), RTOL / 2, ATOL / 2, REL_L2 / 2)
    if grads:
        for n, a, want in zip(names, f_g, g64):
            shares["d" + n] = _share(a, want, 1e-4, 1e-5 * max(float(np.abs(want).max()), 1.0), 1e-5)
    return shares


@pytest.mark.parametrize("d,name", PAIRS, ids=[f"any{d}-{n}" for d, n in PAIRS])
def test_reference_equals_the_oracle_and_the_case_is_admissible(d, name):
    seed = G.seed_for(f"any{d}", name)
    shares = admissibility(d, name, seed)
    print(f"FIG anyw host d={d} {name} seed={seed} " + " ".join(f"{k}={v:.2f}" for k, v in shares.items()))
    assert set(shares) == ({"out", "h'", "h' (dropout)"} | ({"dh", "dW_msg", "dW_self", "dbias", "dgamma", "dbeta"} if d in G.ANY_BWD_WIDTHS else set()))
    for what, share in shares.items():
        assert share <= 1.0, f"any{d} {name} seed {seed}: the float32 oracle's {what} uses {share:.2f} of half the bound: another seed"


# ---- the arithmetic behind the widths -----------------------------------------------------------------------------------

def test_the_widths_are_what_the_kernel_geometry_promises():
    geo = {d: G.generic_geometry(d) for d in G.ANY_FWD_WIDTHS}
    # restated without generic_geometry: thread t holds column t + 256 c; a wave is live when one of its lanes has a column
    for d, g in geo.items():
        cols = [[t + G.GEN_TPB * c for t in range(G.GEN_TPB) if t + G.GEN_TPB * c < d] for c in range(G.GEN_MAX_D // G.GEN_TPB)]
        assert sum(map(len, cols)) == d and g["groups"] == sum(1 for c in cols if c) and g["last_group_threads"] == len(cols[g["groups"] - 1])
        assert g["live_waves"] == len({t // G.WAVE for t in range(G.GEN_TPB) if t < d})
    assert [d for d, g in geo.items() if g["live_waves"] == 1] == [1, 2, 3, 63]
    assert {d: g["live_waves"] for d, g in geo.items() if 1 < g["live_waves"] < 4} == {65: 2, 100: 2, 192: 3}
    assert geo[65]["live_waves"] == 2 and 65 - G.WAVE == 1                   # (the second wave has one live lane)
    assert [d for d, g in geo.items() if g["groups"] > 1 and g["last_group_threads"] == 1] == [257, 513, 769]
    assert [d for d, g in geo.items() if g["groups"] == 4] == [769, 1023]    # c = 3
    assert {g["groups"] for g in geo.values()} == {1, 2, 3, 4}
    assert geo[255] == dict(live_waves=4, groups=1, last_group_threads=255)   # one dead thread, in the last wave
    assert geo[1023] == dict(live_waves=4, groups=4, last_group_threads=255) and G.generic_geometry(1024)["last_group_threads"] == 256
    # what the suite ran before: one live wave, c = 0 only
    assert all(G.generic_geometry(d) == dict(live_waves=1, groups=1, last_group_threads=d) for d in (16, 20, 32))
    # none of the widths has another kernel: 64, 128 and the multiples of 128 do
    assert not [d for d in G.ANY_FWD_WIDTHS + G.MODEL_WIDTHS if d == 64 or d % 128 == 0]
    assert [d % 16 == 0 and d <= 256 for d in G.MODEL_WIDTHS] == [False, True, False] and 96 // 16 == 6
    assert [G.generic_geometry(d)["live_waves"] for d in G.MODEL_WIDTHS] == [2, 2, 4]


def test_the_projection_s_instances_and_routes():
    tg = {NT: G.ip_tile_group(NT) for NT in G.IP_NT}
    assert G.IP_NT == tuple(range(1, 17)) and all(NT % tg[NT] == 0 for NT in tg)
    assert [NT for NT in tg if tg[NT] == 1] == [1, 3, 5, 7, 9, 11, 13, 15]
    assert [NT for NT in tg if tg[NT] == 2] == [2, 6, 10, 14]
    assert [NT for NT in tg if tg[NT] == 4] == [4, 8, 12, 16]
    # F: the k loop runs F / 16 times and reads slice min(j + 1, F / 16 - 1) ahead: once (the only slice read twice), odd counts
    assert [F // 16 for F in G.IP_F] == [1, 3, 5] and all(F % 16 == 0 for F in G.IP_F)
    # N = 77: one workgroup, three tiles of 32 rows, the last with 13 live rows; N = 8200: 65 workgroups, the last tile 8 rows
    assert (-(-77 // 128), -(-77 // 32), 77 - 64) == (1, 3, 13) and (-(-8200 // 128), 8200 % 32) == (65, 8)
    for NT in G.IP_NT:
        for F in G.IP_F:
            assert G.ip_route(77, F, 16 * NT) == "mfma"
            fits = 16 * NT * (F + 4) * 4 <= 72 * 1024
            assert G.ip_route(8200, F, 16 * NT) == ("mfma_wlds" if fits else "mfma")
    # W_in fits LDS at every (d, F) of the table except the three widest at F = 80: 224, 240 and 256 x 84 floats are 73.5,
    # 78.75 and 84 KiB
    assert [(16 * NT, F) for NT in G.IP_NT for F in G.IP_F if G.ip_route(8200, F, 16 * NT) == "mfma"] == [(224, 80), (240, 80), (256, 80)]
    assert all(G.ip_route(N, F, d) == "simple" for F, d in G.IP_SIMPLE for N in G.IP_N)
    assert [(F % 16 != 0, d % 16 != 0, d > 256) for F, d in G.IP_SIMPLE] == [(True, True, False), (False, True, False),
                                                                            (False, False, True), (True, True, True)]
    # the fused SPLIT epilogue runs at N = 77: below the two-piece kernel's N >= 1024 at every F
    assert 77 < 1024
