"""Fenced buffers: every tensor a call allocates sits between two poisoned bands, so that a store next to an output or a
scratch buffer, and a result that depends on bytes the call never wrote, stop being silent.

    raw uint8 buffer:   [ band (>= BAND bytes of `fill`) | interior (exactly nbytes, 256-byte aligned) | band (BAND bytes) ]

What this sees: WRITES outside a buffer's documented size (a band byte changes), and READS that change a result — an
uninitialised scratch word or a load past an input's end gives other bits under the fill 0xFF (NaN as fp32, -1 as an
integer, all flags set) than under 0x5A (a large finite float, a large positive index) or than in an ordinary allocation.
What it cannot see: a stray read whose value never reaches a result, and a write further away than one band (64 KiB: the
widest row the project handles, d = 1024 fp32 = 4 KiB, times a 16-row MFMA tile — one whole stray tile still lands inside).

Imports the host side of torch only; nothing here needs a GPU.
"""

from __future__ import annotations

import contextlib
import os
import sys
from typing import Callable, List, Optional, Sequence

import torch as _torch

BAND = 64 * 1024
ALIGN = 256
FILLS = (0xFF, 0x5A)

# torch.<name> spellings the stand-in module routes through the fence; the AST pass of test_fence_host.py holds the
# package's modules to this list
INTERCEPTED = ("empty", "empty_like", "zeros", "zeros_like", "ones", "ones_like", "full", "full_like")
# every spelling that allocates a tensor of a given size without computing it from other tensors
ALLOCATING_FUNCTIONS = INTERCEPTED + ("empty_strided", "empty_permuted", "rand", "rand_like", "randn", "randn_like", "randint",
                                      "randint_like", "eye", "zeros_strided")
ALLOCATING_METHODS = ("new_empty", "new_empty_strided", "new_zeros", "new_ones", "new_full", "new_tensor")
_HERE = os.path.abspath(__file__)


class FenceError(AssertionError):
    pass


class _Alloc:
    __slots__ = ("raw", "off", "nbytes", "shape", "dtype", "where", "kind")

    def __init__(self, raw, off, nbytes, shape, dtype, where, kind):
        self.raw, self.off, self.nbytes, self.shape, self.dtype, self.where, self.kind = raw, off, nbytes, shape, dtype, where, kind

    def name(self) -> str:
        return f"{self.kind} {tuple(self.shape)} {self.dtype} ({self.nbytes} bytes) allocated at {self.where}"


def _caller() -> str:
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    return "?" if f is None else f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno}"


class Fence:
    """Allocator of fenced tensors with bands of the byte `fill`.  `cpu`: also fence the CPU tensors the stand-in torch module
    is asked for (the host tests; on the GPU only device tensors are fenced, CPU and pinned ones pass through)."""

    def __init__(self, fill: int, cpu: bool = False) -> None:
        if not 0 < int(fill) < 256:
            raise ValueError("the fill is a non-zero byte: reliance on zeroed scratch is one of the things to catch")
        self.fill, self.cpu = int(fill), cpu
        self.allocs: List[_Alloc] = []

    # ---- allocation -------------------------------------------------------------------------------------------------
    def alloc(self, shape, dtype, device, kind: str = "empty", stride=None) -> _torch.Tensor:
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        item = _torch.empty(0, dtype=dtype).element_size()
        nbytes = n * item
        raw = _torch.empty(BAND + ALIGN - 1 + nbytes + BAND, dtype=_torch.uint8, device=device)
        raw.fill_(self.fill)
        off = BAND + (-(raw.data_ptr() + BAND)) % ALIGN
        t = raw[off:off + nbytes].view(dtype)
        t = t.view(shape) if stride is None else t.as_strided(shape, stride)
        assert (raw.data_ptr() + off) % ALIGN == 0, "the interior is not 256-byte aligned"
        assert nbytes == 0 or t.data_ptr() == raw.data_ptr() + off          # (torch gives a tensor without elements no address)
        assert raw.numel() - (off + nbytes) >= BAND and off >= BAND
        self.allocs.append(_Alloc(raw, off, nbytes, shape, dtype, _caller(), kind))
        return t

    def owns(self, t: _torch.Tensor) -> bool:
        p = t.data_ptr()
        return any(a.raw.data_ptr() + a.off == p and a.raw.device == t.device for a in self.allocs)

    def place(self, t: _torch.Tensor) -> _torch.Tensor:
        """A copy of `t` (same shape, dtype, device, contiguous) in a fenced buffer: a read past its end meets the band."""
        if self.owns(t) and t.is_contiguous():
            return t
        out = self.alloc(t.shape, t.dtype, t.device, kind="placed input")
        out.copy_(t.detach())
        return out.requires_grad_(t.requires_grad) if t.requires_grad else out

    def place_tree(self, x):
        """`place` over every tensor of a nest of tuples, lists and dicts; anything else is returned as it is."""
        if isinstance(x, _torch.Tensor):
            return self.place(x)
        if isinstance(x, tuple) and hasattr(x, "_fields"):
            return type(x)(*[self.place_tree(v) for v in x])
        if isinstance(x, (tuple, list)):
            return type(x)(self.place_tree(v) for v in x)
        if isinstance(x, dict):
            return {k: self.place_tree(v) for k, v in x.items()}
        return x

    # ---- the check --------------------------------------------------------------------------------------------------
    def damage(self) -> List[str]:
        if any(a.raw.is_cuda for a in self.allocs):
            _torch.cuda.synchronize()
        found = []
        for a in self.allocs:
            end = a.off + a.nbytes
            for side, band, origin in (("before", a.raw[:a.off], -a.off), ("after", a.raw[end:], a.nbytes)):
                bad = (band != self.fill).nonzero()
                if bad.numel():
                    lo, hi = int(bad[0]) + origin, int(bad[-1]) + origin
                    found.append(f"{a.name()}: {bad.numel()} byte(s) changed {side} the interior, offsets {lo}..{hi} relative to "
                                 f"its start (fill 0x{self.fill:02X})")
        return found

    def check(self) -> None:
        found = self.damage()
        if found:
            raise FenceError("a band no longer holds its fill:\n  " + "\n  ".join(found))

    # ---- the stand-in for the torch module -----------------------------------------------------------------------------
    def torch(self) -> "TorchProxy":
        return TorchProxy(self)


class TorchProxy:
    """Forwards every attribute to torch, except the allocation spellings of INTERCEPTED: those answer from the fence when the
    tensor asked for lives on a fenced device (and is not pinned)."""

    def __init__(self, fence: Fence) -> None:
        self.__dict__["_fence"] = fence

    def __getattr__(self, name):
        return getattr(_torch, name)

    def _fenced(self, device) -> bool:
        device = _torch.device(device) if device is not None else _torch.empty(0).device
        return device.type != "cpu" or self._fence.cpu

    def _make(self, name, args, kwargs):
        real = getattr(_torch, name)
        like = name.endswith("_like")
        device = kwargs.get("device", args[0].device if like else None)
        if kwargs.get("pin_memory") or kwargs.get("out") is not None or not self._fenced(device):
            return real(*args, **kwargs)
        meta = real(*args, **{**kwargs, "device": "meta"})              # torch's own reading of sizes, dtype and strides
        device = _torch.device(device) if device is not None else _torch.empty(0).device
        stride = None if meta.is_contiguous() else meta.stride()
        t = self._fence.alloc(meta.shape, meta.dtype, device, kind=f"torch.{name}", stride=stride)
        if name.startswith("zeros"):
            t.zero_()
        elif name.startswith("ones"):
            t.fill_(1)
        elif name.startswith("full"):
            t.fill_(kwargs["fill_value"] if "fill_value" in kwargs else args[1])
        return t.requires_grad_() if kwargs.get("requires_grad") else t


def _route(name):
    def f(self, *args, **kwargs):
        return self._make(name, args, kwargs)
    f.__name__ = name
    return f


for _name in INTERCEPTED:
    setattr(TorchProxy, _name, _route(_name))


# ---- comparison of runs ----------------------------------------------------------------------------------------------
_INT_OF = {1: _torch.uint8, 2: _torch.int16, 4: _torch.int32, 8: _torch.int64}


def bits(t: _torch.Tensor) -> _torch.Tensor:
    t = t.detach().contiguous()
    return t.view(_torch.uint8) if t.dtype == _torch.bool else t.view(_INT_OF[t.element_size()])


def difference(a, b) -> Optional[str]:
    """None when the two outputs (tensors, None, numbers, or nests of them) hold the same bits, else a description."""
    if isinstance(a, _torch.Tensor) or isinstance(b, _torch.Tensor):
        if not (isinstance(a, _torch.Tensor) and isinstance(b, _torch.Tensor)):
            return f"{type(a).__name__} against {type(b).__name__}"
        if a.shape != b.shape or a.dtype != b.dtype:
            return f"{tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
        x, y = bits(a), bits(b)
        if _torch.equal(x, y):
            return None
        bad = (x.reshape(-1) != y.reshape(-1)).nonzero().reshape(-1)
        i = int(bad[0])
        return (f"{bad.numel()} of {x.numel()} elements differ, first at flat index {i}: "
                f"{a.detach().contiguous().reshape(-1)[i].item()!r} against {b.detach().contiguous().reshape(-1)[i].item()!r}")
    if isinstance(a, dict) and isinstance(b, dict):
        if a.keys() != b.keys():
            return f"keys {sorted(a)} against {sorted(b)}"
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(b)]
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        if len(a) != len(b):
            return f"{len(a)} outputs against {len(b)}"
        for i, (u, v) in enumerate(zip(a, b)):
            d = difference(u, v)
            if d is not None:
                return f"output {i}: {d}"
        return None
    return None if a == b else f"{a!r} against {b!r}"


@contextlib.contextmanager
def installed(fence: Fence, modules: Sequence, monkeypatch):
    """`module.torch` is the fence's stand-in inside the block, for every module given."""
    proxy = fence.torch()
    with monkeypatch.context() as m:
        for mod in modules:
            m.setattr(mod, "torch", proxy)
        yield proxy


def run_three(build_inputs: Callable, call: Callable, modules: Sequence, monkeypatch, cpu: bool = False, what: str = ""):
    """The property every entry point should have: the same bits whatever surrounds its buffers.  `call(build_inputs())` runs
    plain, then fenced under each fill with the inputs placed; after each fenced run every band must hold its fill, and the
    three results must be bit-equal.  Returns the plain result."""
    plain = call(build_inputs())
    for fill in FILLS:
        fence = Fence(fill, cpu=cpu)
        with installed(fence, modules, monkeypatch):
            got = call(fence.place_tree(build_inputs()))
        assert fence.allocs, f"{what}: nothing was allocated through the fence"
        found = fence.damage()
        if found:
            raise FenceError(f"{what}: a band no longer holds its fill:\n  " + "\n  ".join(found))
        diff = difference(plain, got)
        if diff is not None:
            raise FenceError(f"{what}: the result under fill 0x{fill:02X} is not the plain run's — it depends on bytes the call "
                             f"never wrote (uninitialised scratch, or a read past a buffer's end): {diff}")
    return plain
