"""Fenced buffers for include/ghf_pairwise.h, in the pattern of tests/test_distance_fence_gpu.py with the same machinery
(tests/_fence.py).  The two entry points and HyperGNN.pairwise_loss run plain, then with every buffer of the call — inputs
placed, outputs and the workspace allocated through the stand-in torch module — between two 64 KiB bands of 0xFF, then of
0x5A: no band may change and the three results must be bit-equal.  A workspace one byte short must be refused with nothing
written.  Shapes: each lane-group width, the scalar path, K on both sides of a step of 8 x 64 / L positions and of the
four-wave split, B = 5 (a workgroup of four queries and one of one); each under the four scores, both kinds."""

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
FENCED = ("ghf_pair_fwd", "ghf_pair_bwd")
SCORES = (("dot", _native.PAIR_DOT), ("l1", _native.DIST_L1), ("l2", _native.DIST_L2), ("complex", _native.DIST_COMPLEX))
KINDS = (("hinge", _native.PAIR_HINGE), ("logistic", _native.PAIR_LOGISTIC))


def test_every_function_of_the_header_is_fenced_here_or_is_a_size_query():
    """The coverage rule of test_fence_host.py for the sixth header (no GPU needed)."""
    declared = set(_native.pairwise_header_symbols())
    assert declared and declared == set(_native.PAIR_SIGNATURES)
    loose = {s for s in declared if s not in FENCED and not s.endswith("_workspace_bytes")}
    assert not loose, f"declared in include/ghf_pairwise.h but in no fence row: {sorted(loose)}"
    taking = {s for s, (res, args) in _native.PAIR_SIGNATURES.items() if res is _native._i32 and _native._sz in args}
    assert taking == set(FENCED)                        # each of these is also in the refusal test


# (id, d, K, B, N)
ROWS = [("d128_K17", 128, 17, 5, 300), ("d128_K16", 128, 16, 5, 300), ("d256_K9", 256, 9, 5, 300), ("d64_K33", 64, 33, 5, 300),
        ("d20_K65", 20, 65, 5, 300), ("d6_K9_scalar", 6, 9, 5, 300), ("d128_K1000", 128, 1000, 2, 300)]
CASES = [(f"{m}_{r[0]}", M) + r[1:] for m, M in SCORES for r in ROWS]


def build(M, d, K, B, N):
    def inputs():
        rng = np.random.default_rng(1000 * d + K)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        neg = rng.integers(0, N, (B, K))
        neg[rng.random((B, K)) < 0.2] = -1
        neg[0, K - 1] = N - 1                           # the last row of the table, in the last position
        target = rng.integers(0, N, B)
        q = rng.integers(0, N, B)
        neg[1, 0] = q[1]                                # a zero distance
        lists = [np.unique(np.append(rng.integers(0, N, 3), max(int(neg[i, 0]), 0))) for i in range(B)]
        ptr = np.zeros(B + 1, dtype=np.int64)
        ptr[1:] = np.cumsum([len(l) for l in lists])
        return dict(embs=t(rng.standard_normal((N, d)).astype(np.float32)), q=t(q), target=t(target), neg=t(neg), ptr=t(ptr),
                    idx=t(np.concatenate(lists)), grad=t(rng.standard_normal(B).astype(np.float32)),
                    bias=t(rng.standard_normal(N).astype(np.float32)), metric=M)
    return inputs


def call_raw(i):
    M, e, t, neg = i["metric"], i["embs"], i["target"], i["neg"]
    out = []
    for _, kind in KINDS:
        for normalize in (True, False):
            kw = dict(iq=i["q"], filt_ptr=i["ptr"], filt_idx=i["idx"], scale=2.0 / e.size(1), margin=1.0, normalize=normalize,
                      bias=i["bias"] if M == _native.PAIR_DOT and normalize else None)
            loss, count, active = _native.score_pair_fwd(M, kind, e, e, t, neg, **kw)
            dq, coef = _native.score_pair_bwd(M, kind, e, e, t, neg, count, i["grad"], **kw)
            out += [loss, count, active, dq, coef]
    return tuple(out)


def call_model(i):
    """The method with autograd: the grouping (ghf_group_edges), the scatter over coef and the fold of dq too."""
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)
    name = {M: m for m, M in SCORES}[i["metric"]]
    out = []
    for kind, _ in KINDS:
        e = i["embs"].detach().requires_grad_()
        b = i["bias"].detach().requires_grad_() if name == "dot" else None
        loss, active = model.pairwise_loss(e, i["q"], i["target"], negatives=i["neg"], loss=kind, scale=2.0 / e.size(1),
                                           filt_ptr=i["ptr"], filt_idx=i["idx"], candidate_bias=b, return_active=True,
                                           distance=None if name == "dot" else name)
        (loss * i["grad"]).sum().backward()
        out += [loss.detach(), active, e.grad] + ([] if b is None else [b.grad])
    return tuple(out)


class _Recorder:
    """The loaded library with every entry point's use noted; with `fence`, the functions of FENCED are first told one byte
    less than theirs: they must return GHF_EINVAL and change no byte of any buffer, then the real call goes ahead."""

    def __init__(self, lib, fence=None):
        self._lib, self.called, self.sizes, self.rejected, self._fence = lib, set(), set(), set(), fence

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ghf_"):
            return fn
        self.called.add(name)
        if name == "ghf_pair_workspace_bytes":
            def query(*args):
                n = fn(*args)
                self.sizes.add(int(n))
                return n
            return query
        if self._fence is None or name not in FENCED:
            return fn
        at = _native.PAIR_SIGNATURES[name][1].index(_native._sz)

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
    assert set(FENCED) <= rec.called, f"never called: {sorted(set(FENCED) - rec.called)}"


PICKED = [c for c in CASES if c[0].endswith(("d128_K17", "d6_K9_scalar", "d128_K1000"))]


@gpu
@pytest.mark.parametrize("row", PICKED, ids=[r[0] for r in PICKED])
def test_fenced_method_with_autograd(row, monkeypatch):
    rec = _Recorder(_native.load())
    monkeypatch.setattr(_native, "_lib", rec)
    F.run_three(build(*row[1:]), call_model, PATCHED, monkeypatch, what=row[0] + " through the method")
    scatter = "ghf_segment_axpy" if row[1] == _native.PAIR_DOT else "ghf_dist_rows_grad"
    assert {"ghf_pair_fwd", "ghf_pair_bwd", "ghf_group_edges", scatter} <= rec.called


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
