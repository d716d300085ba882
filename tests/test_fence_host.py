"""The fence harness (tests/_fence.py) proves itself on the CPU: plain Python functions on CPU tensors stand in for kernels.

Also here, because they need no GPU: the AST pass that keeps the fence from going blind as the package grows (no device
allocation through a spelling the stand-in torch module does not intercept) and the coverage rule of the GPU case table (every
entry of include/ghf.h is exercised by a row of test_fence_gpu.CASES or stands on the exempt list with a reason)."""

import ast
import os
import re
import types

import pytest
import torch

import _fence as F
from graph_hypernetwork_forge_amd import _native

SRC = os.path.dirname(os.path.abspath(_native.__file__))
PATCHED_FILES = ("_native.py", "plan.py", "autograd.py")
DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64, torch.float32, torch.bool)     # every dtype the package allocates


def _module():
    """A stand-in for one of the package's modules: code that reaches torch through a module global named `torch`."""
    return types.SimpleNamespace(torch=torch)


# ---- the three-run property on host "kernels" ----------------------------------------------------------------------------

def test_a_clean_function_passes(monkeypatch):
    mod = _module()

    def kernel(inputs):
        x, = inputs
        ws = mod.torch.empty(x.numel(), dtype=torch.float32)          # scratch, fully written before it is read
        ws.copy_(x * 2)
        out = mod.torch.empty_like(x)
        out.copy_(ws + 1)
        return out, mod.torch.zeros(3, dtype=torch.int64), mod.torch.full((2, 2), 7.0)

    got = F.run_three(lambda: (torch.arange(5, dtype=torch.float32),), kernel, [mod], monkeypatch, cpu=True)
    assert torch.equal(got[0], torch.arange(5, dtype=torch.float32) * 2 + 1)
    assert mod.torch is torch, "the patch outlived the runs"


@pytest.mark.parametrize("fill", F.FILLS)
@pytest.mark.parametrize("side,at", [("before", -1), ("after", 0)])
def test_one_byte_next_to_the_interior_is_reported(fill, side, at):
    fence = F.Fence(fill, cpu=True)
    proxy = fence.torch()
    first = proxy.empty(4, dtype=torch.float32)
    victim = proxy.empty((3, 5), dtype=torch.int16)
    fence.check()
    a = fence.allocs[1]
    a.raw[a.off + (a.nbytes if side == "after" else 0) + at] = fill ^ 0x01          # through the raw buffer
    with pytest.raises(F.FenceError) as err:
        fence.check()
    msg = str(err.value)
    want = a.nbytes if side == "after" else -1
    assert f"{side} the interior" in msg and f"offsets {want}..{want} " in msg, msg
    assert "torch.empty (3, 5) torch.int16 (30 bytes)" in msg and "test_fence_host.py:" in msg, msg
    assert "(4,)" not in msg, "the clean allocation was blamed too"
    assert first.numel() == 4 and victim.shape == (3, 5)


def test_far_ends_of_both_bands_are_watched():
    fence = F.Fence(0x5A, cpu=True)
    fence.alloc((7,), torch.uint8, "cpu")
    a = fence.allocs[0]
    a.raw[a.off - F.BAND] = 0
    a.raw[a.off + a.nbytes + F.BAND - 1] = 0
    found = fence.damage()
    assert len(found) == 2 and f"offsets {-F.BAND}..{-F.BAND} " in found[0] and f"offsets {7 + F.BAND - 1}..{7 + F.BAND - 1} " in found[1]


def test_reliance_on_uninitialised_scratch_is_reported(monkeypatch):
    mod = _module()

    def kernel(inputs):
        x, = inputs
        ws = mod.torch.empty(8, dtype=torch.int32)
        ws[:4] = x                                                    # half of the scratch is never written ...
        return (ws.sum().reshape(1),)                                 # ... and all of it is read

    with pytest.raises(F.FenceError, match="depends on bytes the call never wrote"):
        F.run_three(lambda: (torch.arange(4, dtype=torch.int32),), kernel, [mod], monkeypatch, cpu=True, what="sum of scratch")
    sums = []
    for fill in F.FILLS:
        fence = F.Fence(fill, cpu=True)
        with F.installed(fence, [mod], monkeypatch):
            sums.append(int(kernel((torch.arange(4, dtype=torch.int32),))[0]))
        fence.check()
    assert sums[0] != sums[1], "the two fills gave the same sum"


def test_a_read_past_a_placed_input_meets_the_band(monkeypatch):
    def kernel(inputs):
        x, = inputs
        past = torch.as_strided(x, (x.numel() + 1,), (1,))            # one element past the end: the band under a fence
        return (past.sum().reshape(1),)

    with pytest.raises(F.FenceError, match="depends on bytes"):
        F.run_three(lambda: (torch.ones(16, dtype=torch.int64)[:4].contiguous(),), kernel, [], monkeypatch, cpu=True)


def test_difference_names_the_output_and_the_element():
    a = (torch.zeros(4), {"k": torch.arange(6, dtype=torch.int64).view(2, 3)}, None, 3)
    b = (torch.zeros(4), {"k": torch.arange(6, dtype=torch.int64).view(2, 3).clone()}, None, 3)
    assert F.difference(a, b) is None
    b[1]["k"][1, 1] = -9
    assert "output 1" in F.difference(a, b) and "flat index 4" in F.difference(a, b)
    assert F.difference(torch.tensor([0.0]), torch.tensor([-0.0])) is not None, "the comparison is on bits, not on values"
    nan = torch.tensor([float("nan")])
    assert F.difference(nan, nan.clone()) is None
    assert F.difference(torch.zeros(2), torch.zeros(3)) is not None and F.difference(torch.zeros(2), None) is not None


# ---- the stand-in module --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_every_spelling_shape_and_dtype(dtype):
    for fill in F.FILLS:
        fence = F.Fence(fill, cpu=True)
        t = fence.torch()
        like = torch.zeros(3, 5, dtype=torch.float32)
        made = [t.empty(6, dtype=dtype), t.empty(2, 3, dtype=dtype), t.empty((2, 3), dtype=dtype), t.empty([2, 3], dtype=dtype),
                t.empty(torch.Size([2, 3]), dtype=dtype), t.empty(0, dtype=dtype), t.empty((0, 3), dtype=dtype),
                t.empty_like(like, dtype=dtype), t.zeros(4, dtype=dtype), t.zeros((2, 2), dtype=dtype), t.zeros_like(like, dtype=dtype),
                t.ones(5, dtype=dtype), t.ones_like(like, dtype=dtype), t.full((3,), 1, dtype=dtype), t.full([2, 2], 1, dtype=dtype),
                t.full_like(like, 1, dtype=dtype), t.empty(3, dtype=dtype, device="cpu"), t.empty(size=(2, 2), dtype=dtype)]
        shapes = [(6,), (2, 3), (2, 3), (2, 3), (2, 3), (0,), (0, 3), (3, 5), (4,), (2, 2), (3, 5), (5,), (3, 5), (3,), (2, 2), (3, 5),
                  (3,), (2, 2)]
        assert len(fence.allocs) == len(made)
        for got, shape in zip(made, shapes):
            assert tuple(got.shape) == shape and got.dtype == dtype and got.is_contiguous()
            assert got.data_ptr() % F.ALIGN == 0
        poison = torch.full((1,), fill, dtype=torch.uint8)
        assert bool((made[1].view(torch.uint8) == poison).all()), "an `empty` interior is poisoned with the fill"
        assert bool((made[8].view(torch.uint8) == 0).all()) and bool((made[10].view(torch.uint8) == 0).all())
        one = torch.ones((), dtype=dtype)
        assert bool((made[11] == one).all()) and bool((made[13] == one).all()) and bool((made[15] == one).all())
        fence.check()
    assert torch.equal(F.Fence(0xFF, cpu=True).torch().empty(2, dtype=torch.int32), torch.tensor([-1, -1], dtype=torch.int32))
    assert bool(torch.isnan(F.Fence(0xFF, cpu=True).torch().empty(2)).all()), "0xFF is NaN as fp32"
    big = F.Fence(0x5A, cpu=True).torch().empty(1)
    assert bool(torch.isfinite(big).all()) and float(big) > 1e15, "0x5A is a large finite float"


def test_defaults_follow_torch():
    t = F.Fence(0x5A, cpu=True).torch()
    assert t.empty(3).dtype == torch.get_default_dtype() and t.full((2,), 3).dtype == torch.int64 and t.full((2,), 2.5).dtype == torch.float32
    src = torch.zeros(4, 6).t()                                     # dense, not contiguous: *_like keeps the strides
    assert t.empty_like(src).stride() == torch.empty_like(src).stride()
    assert t.zeros(2, requires_grad=True).requires_grad
    assert t.float32 is torch.float32 and t.Tensor is torch.Tensor and t.cuda is torch.cuda and t.device("cpu") == torch.device("cpu")


def test_the_interior_ends_exactly_at_its_byte_count():
    fence = F.Fence(0xFF, cpu=True)
    for n in (0, 1, 3, 255, 256, 257, 4097):
        t = fence.alloc((n,), torch.uint8, "cpu")
        a = fence.allocs[-1]
        assert a.nbytes == n and a.off >= F.BAND and a.raw.numel() - a.off - n >= F.BAND
        assert (a.raw.data_ptr() + a.off) % 256 == 0 and (n == 0 or t.data_ptr() == a.raw.data_ptr() + a.off)
        assert bool((a.raw[a.off + n:] == 0xFF).all()) and bool((a.raw[:a.off] == 0xFF).all())


def test_cpu_and_pinned_tensors_pass_through_on_a_device_fence():
    fence = F.Fence(0xFF)                                             # as the GPU tests build it: only device tensors are fenced
    t = fence.torch()
    a, b, c = t.zeros(1, dtype=torch.int32), t.empty(4, device="cpu"), t.full((N := 5,), -1, dtype=torch.int32)
    d = t.empty_like(torch.zeros(3))
    assert not fence.allocs and a.dtype == torch.int32 and b.numel() == 4 and c.numel() == N and d.numel() == 3
    assert F.Fence(0xFF).torch()._fenced("cuda:0") and F.Fence(0xFF).torch()._fenced(torch.device("cuda", 1))


def test_zero_is_no_fill():
    with pytest.raises(ValueError):
        F.Fence(0)


def test_place_copies_into_a_fenced_buffer_once():
    fence = F.Fence(0x5A, cpu=True)
    x = torch.arange(12, dtype=torch.int64).view(3, 4)
    y = fence.place(x)
    assert torch.equal(x, y) and y.data_ptr() != x.data_ptr() and fence.owns(y) and fence.place(y) is y
    nest = fence.place_tree({"a": [x, (x.t(), 3)], "b": None})
    assert nest["b"] is None and nest["a"][1][1] == 3 and torch.equal(nest["a"][1][0], x.t()) and nest["a"][1][0].is_contiguous()
    assert len(fence.allocs) == 3
    fence.check()


# ---- the package may allocate device tensors through intercepted spellings only -------------------------------------------

def unfenced_allocations(source: str, name: str = "<source>"):
    """Calls in `source` that allocate a tensor through a spelling the stand-in module does not route through the fence, and
    imports that would reach torch past the module global `torch`."""
    found = []
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, ast.ImportFrom) and node.module and node.module.split(".")[0] == "torch":
            bad = [a.name for a in node.names if a.name in F.ALLOCATING_FUNCTIONS]
            found += [f"{name}:{node.lineno}: from torch import {n}" for n in bad]
        if isinstance(node, ast.Import):
            found += [f"{name}:{node.lineno}: import torch as {a.asname}" for a in node.names if a.name == "torch" and a.asname not in (None, "torch")]
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
            continue
        attr, base = node.func.attr, node.func.value
        if isinstance(base, ast.Name) and base.id == "torch":
            if attr in F.ALLOCATING_FUNCTIONS and attr not in F.INTERCEPTED:
                found.append(f"{name}:{node.lineno}: torch.{attr}")
        elif attr in F.ALLOCATING_METHODS:
            found.append(f"{name}:{node.lineno}: .{attr}")
    return found


def test_the_ast_pass_sees_what_it_is_there_for():
    bad = "import torch\nimport torch as th\nfrom torch import zeros\n" \
          "def f(x):\n    a = x.new_empty(3)\n    b = torch.empty_strided((2,), (1,))\n    c = x.y.new_zeros(2)\n    return torch.empty(3)\n"
    got = unfenced_allocations(bad)
    assert [g.split(": ")[1] for g in got] == ["import torch as th", "from torch import zeros", ".new_empty", "torch.empty_strided", ".new_zeros"]
    assert set(F.INTERCEPTED) <= set(F.ALLOCATING_FUNCTIONS)
    for name in F.INTERCEPTED:
        assert name in F.TorchProxy.__dict__, f"the stand-in does not route torch.{name}"


@pytest.mark.parametrize("fname", PATCHED_FILES)
def test_no_allocation_goes_round_the_fence(fname):
    with open(os.path.join(SRC, fname)) as f:
        source = f.read()
    assert "\nimport torch\n" in source, f"{fname} no longer reaches torch through a module global named torch"
    found = unfenced_allocations(source, fname)
    assert not found, "allocations the fence cannot see (use torch.empty / zeros / ones / full or their _like forms):\n" + "\n".join(found)


# ---- every ABI entry is exercised by the GPU case table or exempt for a reason ---------------------------------------------

EXEMPT = {            # entries that write no device memory
    "ghf_abi_version": "returns a constant",
    "ghf_last_error": "returns a host string",
    "ghf_message_config": "writes four host integers",
    "ghf_set_range_flag": "registers a pointer; writes nothing (the registered word is compared across the runs instead)",
    "ghf_host_checksum64": "host memory only",
    "ghf_host_word_ids": "host memory only",
}
EXEMPT_PATTERNS = {r"ghf_\w+_supported": "a query: returns an int", r"ghf_\w+_(bytes|floats)": "a size query",
                   r"ghf_\w+_max_\w+": "a size query"}


def uncovered(symbols, covered):
    return sorted(s for s in symbols if s not in covered and s not in EXEMPT
                  and not any(re.fullmatch(p, s) for p in EXEMPT_PATTERNS))


def test_every_entry_point_is_fenced_or_exempt():
    import test_fence_gpu as T
    symbols = _native.header_symbols()
    assert set(symbols) == set(_native.SIGNATURES), "include/ghf.h and _native.SIGNATURES name different functions"
    covered = set()
    for case in T.CASES:
        assert case.symbols, f"case {case.id} names no entry point"
        unknown = set(case.symbols) - set(symbols)
        assert not unknown, f"case {case.id} names {sorted(unknown)}, which include/ghf.h does not declare"
        covered |= set(case.symbols)
    stale = [s for s in EXEMPT if s not in symbols]
    assert not stale, f"exempt entries that no longer exist: {stale}"
    both = sorted(s for s in covered if s in EXEMPT or any(re.fullmatch(p, s) for p in EXEMPT_PATTERNS))
    assert not both, f"entries both exempt and claimed by a case: {both}"
    missing = uncovered(symbols, covered)
    assert not missing, f"entry points no row of test_fence_gpu.CASES exercises: {missing}"
    assert uncovered(symbols, covered - {"ghf_dot"}) == ["ghf_dot"], "the coverage rule does not notice a missing row"
    assert len({c.id for c in T.CASES}) == len(T.CASES), "case ids repeat"
    sized = {s for s in symbols if _native.SIGNATURES[s][0] is _native._i32 and _native._sz in _native.SIGNATURES[s][1]}
    refused = {s for c in T.REJECT for s in c.symbols}
    assert len(sized) > 30 and sized <= refused, f"entry points that take workspace_bytes and are in no rejection case: {sorted(sized - refused)}"
