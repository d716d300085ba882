"""Fenced buffers for include/ghf_distance_loss.h, in the pattern of tests/test_distance_sweep_fence_gpu.py with the same
machinery (tests/_fence.py).  The three entry points and the two methods run plain, then with every buffer of the call — inputs
placed, outputs and the workspace allocated through the stand-in torch module — between two 64 KiB bands of 0xFF, then of 0x5A:
no band may change and the three results must be bit-equal.  A workspace one byte short must be refused with nothing written.
Shapes: the scalar path (d = 6), one column step and several (d = 16, 64), both column halves of the backward (d = 130, 256),
C one short of and one past a tile and a slab with the table's last row reachable, B one past an owner tile; each under the
three metrics, with and without ic."""

import numpy as np
import pytest
import torch

import _fence as F
from graph_hypernetwork_forge_amd import HyperGNN, _native, autograd, plan as plan_mod
from graph_hypernetwork_forge_amd.models import hypergnn as hypergnn_mod

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
PATCHED = (_native, plan_mod, autograd, hypergnn_mod)
EINVAL = -1
FENCED = ("ghf_dist_loss_softmax_fwd", "ghf_dist_loss_negsamp_fwd", "ghf_dist_loss_bwd")
SIZE_QUERIES = ("ghf_dist_loss_fwd_workspace_bytes", "ghf_dist_loss_bwd_workspace_bytes")
METRICS = (("l1", _native.DIST_L1), ("l2", _native.DIST_L2), ("complex", _native.DIST_COMPLEX))


def test_every_function_of_the_header_is_fenced_here_or_is_a_size_query():
    """The coverage rule of test_fence_host.py for the fifth header (no GPU needed)."""
    declared = set(_native.distance_loss_header_symbols())
    assert declared and declared == set(_native.DLOSS_SIGNATURES)
    assert declared == set(FENCED) | set(SIZE_QUERIES)
    taking = {s for s, (res, args) in _native.DLOSS_SIGNATURES.items() if res is _native._i32 and _native._sz in args}
    assert taking == set(FENCED)                                         # each of these is also in the refusal test


# (id, d, B, N, subset)
ROWS = [("d64_N257", 64, 5, 257, False), ("d64_N1025_sub", 64, 65, 1025, True), ("d6_N255_scalar", 6, 5, 255, False),
        ("d6_N300_scalar_sub", 6, 65, 300, True), ("d130_N513", 130, 65, 513, False), ("d256_N300_sub", 256, 5, 300, True),
        ("d16_N2100", 16, 1, 2100, False)]
CASES = [(f"{m}_{r[0]}", M) + r[1:] for m, M in METRICS for r in ROWS]


def build(M, d, B, N, subset):
    def inputs():
        rng = np.random.default_rng(1000 * d + N)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        ic = np.unique(np.append(rng.integers(0, N, N // 2), N - 1)) if subset else np.arange(N)   # ends on the table's last row
        target = ic[rng.integers(0, len(ic), B)]
        q = rng.integers(0, N, B)
        target[0] = N - 1                               # the last row of the table
        lists = [np.unique(np.append(rng.integers(0, N, 3), [q[i], N - 1] if i % 2 else [q[i]])) for i in range(B)]
        ptr = np.zeros(B + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([len(l) for l in lists])
        out = dict(embs=t(rng.standard_normal((N, d)).astype(np.float32)), q=t(q), target=t(target), ptr=t(ptr),
                   idx=t(np.concatenate(lists)), rows=t(rng.standard_normal((B, d)).astype(np.float32)),
                   grad=t((0.5 + rng.random(B)).astype(np.float32)), metric=M)
        if subset:
            out["ic"] = t(ic)
        return out
    return inputs


def call_raw(i):
    M, e, t, ic, g = i["metric"], i["embs"], i["target"], i.get("ic"), i["grad"]
    lists = dict(filt_ptr=i["ptr"], filt_idx=i["idx"])
    out = []
    for kw in (dict(iq=i["q"], **lists), dict()):                         # by id with lists; own rows, no iq, no lists
        q = e if kw else i["rows"]
        loss, lse = _native.score_dist_loss_softmax_fwd(M, q, e, t, scale=0.1, ic=ic, **kw)
        nl, lw = _native.score_dist_loss_negsamp_fwd(M, q, e, t, scale=0.1, margin=1.0, adversarial_temperature=0.5, ic=ic, **kw)
        dq1, dc1 = _native.score_dist_loss_bwd(M, _native.NEG_SOFTMAX, q, e, t, lse, g, scale=0.1, ic=ic, **kw)
        dq2, dc2 = _native.score_dist_loss_bwd(M, _native.NEG_NEGSAMP, q, e, t, lw, g, scale=0.1, margin=1.0,
                                               adversarial_temperature=0.5, ic=ic, **kw)
        out += [loss, lse, nl, lw, dq1, dc1, dq2, dc2]
    return tuple(out)


def call_model(i):
    """The methods, recorded and differentiated: the lists built from known edges on the device, the candidates from ids."""
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)
    name = {M: m for m, M in METRICS}[i["metric"]]
    q, t = i["q"], i["target"]
    known = (q, torch.flip(t, (0,)))
    kw = dict(candidates=i["ic"]) if "ic" in i else {}
    out = []
    for fn, more in ((model.softmax_loss_by_distance, {}),
                     (model.negative_sampling_loss_by_distance, dict(margin=1.0, adversarial_temperature=0.5))):
        e = i["embs"].clone().requires_grad_()
        a = fn(e, q, t, name, scale=0.1, known=known, **more, **kw)
        (a * i["grad"]).sum().backward()
        e2, r = i["embs"].clone().requires_grad_(), i["rows"].clone().requires_grad_()
        b = fn(e2, q, t, name, scale=0.1, query_rows=r, filt_ptr=i["ptr"], filt_idx=i["idx"], **more, **kw)
        (b * i["grad"]).sum().backward()
        out += [a.detach(), e.grad, b.detach(), e2.grad, r.grad]
    return tuple(out)


class _Recorder:
    """The loaded library with every entry point's use noted; with `fence`, the three calls are first told one byte less than
    their workspace: they must return GHF_EINVAL and change no byte of any buffer, then the real call goes ahead."""

    def __init__(self, lib, fence=None):
        self._lib, self.called, self.sizes, self.rejected, self._fence = lib, set(), set(), set(), fence

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ghf_"):
            return fn
        self.called.add(name)
        if name in SIZE_QUERIES:
            def query(*args):
                n = fn(*args)
                self.sizes.add(int(n))
                return n
            return query
        if self._fence is None or name not in FENCED:
            return fn
        at = _native.DLOSS_SIGNATURES[name][1].index(_native._sz)

        def call(*args):
            need = int(args[at])
            assert need > 0 and need in self.sizes, f"{name}: told {need} workspace bytes, which the size query never returned"
            torch.cuda.synchronize()
            before = [a.raw.clone() for a in self._fence.allocs]
            rc = fn(*args[:at], need - 1, *args[at + 1:])
            torch.cuda.synchronize()
            assert rc == EINVAL, f"{name}: workspace_bytes = need - 1 = {need - 1} returned {rc}, not GHF_EINVAL"
            for a, b in zip(self._fence.allocs, before):
                assert torch.equal(a.raw, b), f"{name} refused a workspace of need - 1 bytes, yet wrote into {a.name()}"
            self.rejected.add(name)
            return fn(*args)
        return call


@gpu
@pytest.mark.parametrize("row", CASES, ids=[r[0] for r in CASES])
def test_fenced_call(row, monkeypatch):
    rec = _Recorder(_native.load())
    monkeypatch.setattr(_native, "_lib", rec)
    F.run_three(build(*row[1:]), call_raw, PATCHED, monkeypatch, what=row[0])
    assert set(FENCED) | set(SIZE_QUERIES) <= rec.called, f"never called: {sorted(set(FENCED) - rec.called)}"


PICKED = [c for c in CASES if c[0].endswith(("d64_N1025_sub", "d6_N255_scalar", "d130_N513"))]


@gpu
@pytest.mark.parametrize("row", PICKED, ids=[r[0] for r in PICKED])
def test_fenced_methods(row, monkeypatch):
    rec = _Recorder(_native.load())
    monkeypatch.setattr(_native, "_lib", rec)
    F.run_three(build(*row[1:]), call_model, PATCHED, monkeypatch, what=row[0] + " through the methods")
    assert set(FENCED) <= rec.called


@gpu
@pytest.mark.parametrize("row", PICKED, ids=[r[0] for r in PICKED])
def test_a_workspace_one_byte_short_is_refused(row, monkeypatch):
    fence = F.Fence(0xFF)
    rec = _Recorder(_native.load(), fence)
    monkeypatch.setattr(_native, "_lib", rec)
    with F.installed(fence, PATCHED, monkeypatch):
        call_raw(fence.place_tree(build(*row[1:])()))
    fence.check()
    assert set(FENCED) <= rec.rejected, f"not reached with need - 1: {sorted(set(FENCED) - rec.rejected)}"
