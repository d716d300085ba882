"""Fenced buffers for include/ghf_pairwise_dot_sweep.h, in the pattern of tests/test_pairwise_sweep_fence_gpu.py with the same
machinery (tests/_fence.py) at seven shapes of the matrix-core sweeps, with and without ic and bias.  The two entry points and
the method run plain, then with every buffer of the call — inputs placed, outputs and the workspace allocated through the
stand-in torch module — between two 64 KiB bands of 0xFF, then of 0x5A: no band may change and the three results must be
bit-equal.  A workspace one byte short must be refused with nothing written."""

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
FENCED = ("ghf_score_pair_fwd", "ghf_score_pair_bwd")
SIZE_QUERIES = ("ghf_score_pair_fwd_workspace_bytes", "ghf_score_pair_bwd_workspace_bytes")
KINDS = (("hinge", _native.PAIR_HINGE), ("logistic", _native.PAIR_LOGISTIC))

# (id, d, B, N, subset, biased): both kernel shapes (d <= 128 | d > 128), d that is no multiple of 4 (the scalar load path) or of
# 32 (the backward's column step), candidate counts at the tile edges (256 | 257, 128 | 129), two query tiles, a table that
# ends on a candidate
CASES = [("d64_N257", 64, 5, 257, False, False), ("d64_N1025_sub_bias", 64, 129, 1025, True, True), ("d6_N255_scalar_bias", 6, 5, 255, False, True),
         ("d22_N300_sub", 22, 65, 300, True, False), ("d130_N513_bias", 130, 65, 513, False, True), ("d256_N300_sub_bias", 256, 5, 300, True, True),
         ("d20_N4200", 20, 1, 4200, False, False)]
PICKED = [c for c in CASES if c[0] in ("d64_N1025_sub_bias", "d6_N255_scalar_bias", "d130_N513_bias")]


def test_every_function_of_the_header_is_fenced_here_or_is_a_size_query():
    """The coverage rule of test_fence_host.py for the eighth header (no GPU needed)."""
    declared = set(_native.pairwise_dot_sweep_header_symbols())
    assert declared and declared == set(_native.PAIRDOT_SIGNATURES)
    assert declared == set(FENCED) | set(SIZE_QUERIES)
    taking = {s for s, (res, args) in _native.PAIRDOT_SIGNATURES.items() if res is _native._i32 and _native._sz in args}
    assert taking == set(FENCED)                                         # each of these is also in the refusal test


def build(d, B, N, subset, biased):
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
                   grad=t((0.5 + rng.random(B)).astype(np.float32)))
        if subset:
            out["ic"] = t(ic)
        if biased:
            out["bias"] = t(rng.standard_normal(N).astype(np.float32))
        return out
    return inputs


def call_raw(i):
    e, t, ic, g, bias = i["embs"], i["target"], i.get("ic"), i["grad"], i.get("bias")
    lists = dict(filt_ptr=i["ptr"], filt_idx=i["idx"])
    out = []
    for kw in (dict(iq=i["q"], **lists), dict()):                         # by id with lists; own rows, no iq, no lists
        q = e if kw else i["rows"]
        for (_, kind), normalize in zip(KINDS, (True, False)):
            more = dict(scale=0.1, margin=1.0, normalize=normalize, ic=ic, bias=bias, **kw)
            loss, dsum, count, active = _native.score_pair_sweep_fwd(kind, q, e, t, **more)
            out += [loss, dsum, count, active]
            out += list(_native.score_pair_sweep_bwd(kind, q, e, t, dsum, count, g, **more))
    return tuple(out)


def call_model(i):
    """The method, recorded and differentiated: the lists built from known edges on the device, the candidates from ids."""
    model = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16)
    q, t = i["q"], i["target"]
    known = (q, torch.flip(t, (0,)))
    kw = dict(candidates=i["ic"]) if "ic" in i else {}
    out = []
    for kind, _ in KINDS:
        e = i["embs"].clone().requires_grad_()
        b = i["bias"].clone().requires_grad_() if "bias" in i else None
        a, act = model.pairwise_loss_by_dot(e, q, t, loss=kind, scale=0.1, known=known, return_active=True, candidate_bias=b, **kw)
        (a * i["grad"]).sum().backward()
        e2, r = i["embs"].clone().requires_grad_(), i["rows"].clone().requires_grad_()
        c = model.pairwise_loss_by_dot(e2, q, t, loss=kind, scale=0.1, normalize=False, query_rows=r, filt_ptr=i["ptr"], filt_idx=i["idx"],
                                       **kw)
        (c * i["grad"]).sum().backward()
        out += [a.detach(), act, e.grad, c.detach(), e2.grad, r.grad] + ([b.grad] if b is not None else [])
    return tuple(out)


class _Recorder:
    """The loaded library with every entry point's use noted; with `fence`, the two calls are first told one byte less than
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
        at = _native.PAIRDOT_SIGNATURES[name][1].index(_native._sz)

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


@gpu
@pytest.mark.parametrize("row", PICKED, ids=[r[0] for r in PICKED])
def test_fenced_method(row, monkeypatch):
    rec = _Recorder(_native.load())
    monkeypatch.setattr(_native, "_lib", rec)
    F.run_three(build(*row[1:]), call_model, PATCHED, monkeypatch, what=row[0] + " through the method")
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
