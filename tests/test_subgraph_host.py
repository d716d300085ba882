"""Host-side checks of the node-batch forward (HyperGNN.forward_nodes) and its subgraph entry points: no GPU needed."""

import ctypes
import os
import re

import pytest
import torch

from graph_hypernetwork_forge_amd import HyperGNN, ToyKnowledgeGraph, _build, _native

SUBGRAPH_CALLS = ("ghf_subgraph_workspace_bytes", "ghf_subgraph_hops", "ghf_subgraph_nodes", "ghf_subgraph_edges")


def test_subgraph_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(_build.INCLUDE, "ghf.h")) as f:
        text = f.read()
    assert re.search(r"#define GHF_ABI_VERSION 15\b", text)
    lib = _native.load()
    for name in SUBGRAPH_CALLS:
        assert name in _native.header_symbols() and name in _native.SIGNATURES
        assert hasattr(lib, name), f"libghf_hip.so does not export {name}"


def test_subgraph_entry_points_reject_null_and_invalid_arguments_without_a_gpu():
    lib = _native.load()
    assert lib.ghf_subgraph_workspace_bytes(1000, 5000, 2) >= 2 * 4 * 5001
    assert lib.ghf_subgraph_workspace_bytes(1000, 5000, 0) == 0
    assert lib.ghf_subgraph_workspace_bytes(0, 5000, 2) == 0
    assert lib.ghf_subgraph_workspace_bytes(1000, -1, 2) == 0
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below fails its checks on the host
    ws = ctypes.c_void_p(1 << 20)
    nb = lib.ghf_subgraph_workspace_bytes(1000, 5000, 2)
    assert lib.ghf_subgraph_hops(None, None, 1000, 5000, 4, 1, fake, 3, 2, ws, nb, fake, None) == -1
    assert b"null" in lib.ghf_last_error()
    assert lib.ghf_subgraph_hops(fake, fake, 1000, 5000, 4, 1, fake, 3, 2, None, nb, fake, None) == -1
    assert lib.ghf_subgraph_hops(fake, fake, 1000, 5000, 4, 1, fake, 3, 0, ws, nb, fake, None) == -1      # k = 0
    assert lib.ghf_subgraph_hops(fake, fake, 1000, 5000, 0, 1, fake, 3, 2, ws, nb, fake, None) == -1      # R = 0
    assert lib.ghf_subgraph_hops(fake, fake, 1000, 5000, 4, 1, fake, -1, 2, ws, nb, fake, None) == -1     # S < 0
    assert lib.ghf_subgraph_hops(fake, fake, 1000, 5000, 4, 1, fake, 3, 2, ws, nb - 1, fake, None) == -1  # small workspace
    assert b"workspace" in lib.ghf_last_error()
    assert lib.ghf_subgraph_hops(fake, fake, 1000, 5000, 4, 1, fake, 3, 2, ctypes.c_void_p((1 << 20) + 4), nb, fake,
                                 None) == -1                                                              # misaligned
    assert lib.ghf_subgraph_hops(fake, fake, 1 << 20, 5000, 1 << 13, 1, fake, 3, 2, ws, 1 << 40, fake, None) == -1  # keys > 32 bits
    assert lib.ghf_subgraph_nodes(None, 1000, 2, ws, nb, fake, fake, fake, None) == -1
    assert lib.ghf_subgraph_nodes(fake, 1000, 2, ws, nb, fake, None, fake, None) == -1
    assert lib.ghf_subgraph_nodes(fake, 0, 2, ws, nb, fake, fake, fake, None) == -1
    assert lib.ghf_subgraph_nodes(fake, 1000, 0, ws, nb, fake, fake, fake, None) == -1
    assert lib.ghf_subgraph_edges(fake, fake, 1000, 5000, 4, 384, fake, fake, 2, ws, nb, None, fake, fake, None) == -1
    assert lib.ghf_subgraph_edges(fake, fake, 1000, 5000, 4, 384, None, fake, 2, ws, nb, fake, fake, fake, None) == -1
    assert lib.ghf_subgraph_edges(fake, fake, 1000, 5000, 4, 384, fake, fake, 2, ws, nb, fake, fake, None, None) == -1
    assert lib.ghf_subgraph_edges(fake, fake, 1000, 5000, 4, 0, fake, fake, 2, ws, nb, fake, fake, fake, None) == -1


def _toy():
    kg = ToyKnowledgeGraph(feat_dim=16)
    m = HyperGNN(text_dim=32, node_feat_dim=16, hidden_dim=16).eval()
    return kg, m, list(kg.relation_types), torch.tensor([kg.relation_types.index(t) for t in kg.edge_texts])


@pytest.mark.parametrize("ids", [True, False])
def test_forward_nodes_validates_before_any_device_work(ids):
    kg, m, rel_texts, rel = _toy()

    def call(x, texts_or_rel, nodes, ei=kg.edge_index):
        with torch.no_grad():
            if ids:
                return m.forward_nodes_ids(x, ei, texts_or_rel, rel_texts, nodes)
            return m.forward_nodes(x, ei, texts_or_rel, nodes)

    good = rel if ids else kg.edge_texts
    bad = rel[:-1] if ids else kg.edge_texts[:-1]
    x = kg.node_features
    with pytest.raises(ValueError):                                     # texts / relation ids do not match the edges
        call(x, bad, torch.tensor([0, 1]))
    with pytest.raises(ValueError):                                     # wrong feature width
        call(x[:, :8], good, torch.tensor([0, 1]))
    with pytest.raises(ValueError):                                     # 2-D nodes
        call(x, good, torch.tensor([[0, 1]]))
    with pytest.raises(TypeError):                                      # float nodes
        call(x, good, torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError):                                     # not a tensor
        call(x, good, [0, 1])
    with pytest.raises(RuntimeError, match="no CPU"):                   # CPU features: fail loudly, no fallback
        call(x, good, torch.tensor([0, 1]))
    with pytest.raises(RuntimeError, match="no CPU"):
        call(x, good, torch.tensor([-8, 7], dtype=torch.int32))         # (the ends of [-N, N) are valid ids)


def test_forward_nodes_out_of_range_ids_raise_index_error():
    """As indexing raises: the check runs on the ids before anything else needs the device (the fake device tensor below
    only has to report is_cuda)."""
    kg, m, _, _ = _toy()

    class OnDevice(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    x = kg.node_features.as_subclass(OnDevice)
    for bad in ([0, 8], [-9], [100]):
        with pytest.raises(IndexError):
            HyperGNN._seed_ids(torch.tensor(bad), x)
    got = HyperGNN._seed_ids(torch.tensor([3, -1, -8, 3], dtype=torch.int32), x)
    assert got.dtype == torch.int64 and got.tolist() == [3, 7, 0, 3]
