"""A guard-band arena for the C ABI's memory contract (include/nsm_hip.h): every buffer a test hands to the library is a
view of ONE tensor of seeded random bytes, so a write outside a declared extent lands in bytes the test still knows.

The suite's other files give every buffer a ``torch`` tensor of its own.  The caching allocator rounds each up to 512 bytes
and never places two back to back, and most outputs start as zeros: a record written one slot past ``capacity``, a queue
half one entry too long, or an output the entry forgot to initialise all pass.  Here

* ``carve`` hands out a typed view of EXACTLY the bytes asked for, on a 256-byte boundary; the bytes behind it, up to the
  next region, are guard.  Every region keeps at least ``GUARD`` = 4096 guard bytes on both sides, the last one included.
  A wavefront's largest single burst in this library is 64 records of 16 bytes (1024 B); the guard is four times that.
* the view keeps the arena's random bytes -- the poison.  Random, not a constant, so that a kernel storing that constant is
  still seen; no byte of the pattern is zero, so "left as it was" can be told from "zeroed".
* ``check`` compares every byte outside the carved regions with the host copy, ``unchanged`` a whole region (inputs),
  ``poison`` gives the bytes a region started with (outputs the header says are left alone).

Alignment stays at 256 bytes on purpose -- what any allocator grants.  A kernel that assumed MORE alignment than the header
grants would show up as a GPU fault, not as a failed assertion; the alignment contract is out of scope here.  Reads outside
an extent are not detected either, unless they change a result (the surroundings are random bytes, not zeros).
"""
import copy
import ctypes
import dataclasses
from typing import Dict, Optional, Tuple

import numpy as np
import torch

GUARD = 4096
ALIGN = 256


class ArenaError(AssertionError):
    pass


class Arena:
    def __init__(self, nbytes: int, device, seed: int = 0) -> None:
        self.nbytes = int(nbytes)
        self.host = np.random.default_rng(seed).integers(1, 256, size=self.nbytes, dtype=np.uint8)  # (no zero byte)
        self.buf = torch.from_numpy(self.host.copy()).to(device)
        self.base = self.buf.data_ptr()
        self.regions: Dict[str, Tuple[int, int]] = {}  # name -> (start, end), in carving order
        self._cursor = 0
        self._carved = np.zeros(self.nbytes, dtype=bool)

    # ---------------------------------------------------------------------------------------------------------- carving
    def carve(self, name: str, nbytes: int, dtype=torch.uint8, shape=None) -> torch.Tensor:
        """A view of exactly ``nbytes`` bytes as ``dtype`` (and ``shape``), starting on a 256-byte boundary at least
        ``GUARD`` bytes behind the previous region, still holding the arena's random bytes."""
        if name in self.regions:
            raise ValueError(f"region {name!r} carved twice")
        nbytes = int(nbytes)
        item = torch.empty(0, dtype=dtype).element_size()
        if nbytes < 0 or nbytes % item:
            raise ValueError(f"region {name!r}: {nbytes} bytes are no whole number of {dtype} elements")
        start = self._cursor + GUARD
        start += -(self.base + start) % ALIGN
        end = start + nbytes
        if end + GUARD > self.nbytes:
            raise ValueError(f"region {name!r}: the arena of {self.nbytes} bytes is full ({end + GUARD} needed)")
        self.regions[name] = (start, end)
        self._carved[start:end] = True
        self._cursor = end
        view = self.buf[start:end].view(dtype)
        return view if shape is None else view.view(shape)

    def ptr(self, name: str) -> int:
        """The region's device address (an empty view has no ``data_ptr`` of its own)."""
        return self.base + self.regions[name][0]

    def view(self, name: str, dtype=torch.uint8) -> torch.Tensor:
        start, end = self.regions[name]
        return self.buf[start:end].view(dtype)

    def fill(self, name: str, tensor) -> torch.Tensor:
        """Copy ``tensor`` (its bytes, exactly the region's size) in; the host copy follows."""
        start, end = self.regions[name]
        data = tensor.detach().cpu().contiguous().numpy() if isinstance(tensor, torch.Tensor) else np.ascontiguousarray(tensor)
        raw = np.frombuffer(data.tobytes(), dtype=np.uint8)
        if raw.size != end - start:
            raise ValueError(f"region {name!r} holds {end - start} bytes, got {raw.size}")
        self.host[start:end] = raw
        self.buf[start:end] = torch.from_numpy(self.host[start:end].copy()).to(self.buf.device)
        return self.buf[start:end]

    def zero(self, name: str) -> None:
        """A counter the header marks "caller zeroes"."""
        start, end = self.regions[name]
        self.fill(name, np.zeros(end - start, dtype=np.uint8))

    # --------------------------------------------------------------------------------------------------------- checking
    def _now(self) -> np.ndarray:
        return self.buf.cpu().numpy()

    def _where(self, offset: int) -> str:
        """``offset`` relative to the nearest region's edge."""
        best = None
        for name, (start, end) in self.regions.items():
            for dist, text in ((start - offset, "before the start of"), (offset - end + 1, "behind the end of")):
                if dist > 0 and (best is None or dist < best[0]):
                    best = (dist, f"{dist} byte(s) {text} {name!r}")
            if start <= offset < end:
                return f"byte {offset - start} of {name!r}"
        return best[1] if best else "no region carved"

    def _report(self, what: str, diff: np.ndarray, origin: int = 0) -> None:
        at = np.flatnonzero(diff)
        if at.size:
            first, last = int(at[0]) + origin, int(at[-1]) + origin
            raise ArenaError(f"{what}: {at.size} byte(s) changed, arena offsets {first} .. {last}: first {self._where(first)}, "
                             f"last {self._where(last)}")

    def check(self, unchanged=()) -> None:
        """Every byte outside the carved regions still equals the host copy, else ``ArenaError`` with the first and last
        differing offset, the nearest region's name and the distance from its edge.  ``unchanged``: regions to compare as
        ``unchanged()`` does, from the same snapshot."""
        now = self._now()
        self._report("guard bytes written", (now != self.host) & ~self._carved)
        for name in unchanged:
            start, end = self.regions[name]
            self._report(f"region {name!r} written", now[start:end] != self.host[start:end], start)

    def unchanged(self, name: str) -> None:
        """The whole region still equals the host copy (an input, or an output the entry must not have touched)."""
        start, end = self.regions[name]
        now = self.buf[start:end].cpu().numpy()
        self._report(f"region {name!r} written", now != self.host[start:end], start)

    def read(self, name: str, dtype=np.uint8) -> np.ndarray:
        start, end = self.regions[name]
        return self.buf[start:end].cpu().numpy().view(dtype)

    def poison(self, name: str, dtype=np.uint8) -> np.ndarray:
        """What the region held when it was carved (or last filled), as ``dtype``."""
        start, end = self.regions[name]
        return self.host[start:end].copy().view(dtype)


def nbytes_of(*tensors: Optional[torch.Tensor]) -> int:
    """Arena bytes that re-homing ``tensors`` takes, guards and alignment included."""
    return sum(t.numel() * t.element_size() + GUARD + ALIGN for t in tensors if t is not None)


def _tensors_of(obj):
    if dataclasses.is_dataclass(obj):
        return {f.name: getattr(obj, f.name) for f in dataclasses.fields(obj) if isinstance(getattr(obj, f.name), torch.Tensor)}
    return {k: v for k, v in obj.items() if isinstance(v, torch.Tensor)}


def table_bytes(*tables) -> int:
    return sum(nbytes_of(*_tensors_of(t[1] if isinstance(t, tuple) else t).values()) for t in tables)


def rehome(table, arena: Arena, prefix: Optional[str] = None):
    """A copy of ``table`` whose tensors are arena views of exactly the original sizes, filled with the original bytes and
    named ``prefix.column`` (default prefix: the table's type and a running number): a ``SetTable`` / ``StrTable`` / ``LevelItems`` (``struct()`` then hands the library arena
    pointers), or an any-grid operand of wide.py -- a ``(ctypes struct, dict of tensors)`` pair, whose copy has every pointer
    field that named one of the tensors redirected."""
    if prefix is None:
        kind = type(table[0] if isinstance(table, tuple) else table).__name__
        prefix = f"{kind}{sum(1 for name in arena.regions if name.startswith(kind))}"
    if isinstance(table, tuple):
        struct, keep = table
        new_struct = type(struct)()
        ctypes.memmove(ctypes.byref(new_struct), ctypes.byref(struct), ctypes.sizeof(struct))
        new_keep = dict(keep)
        for key, t in _tensors_of(keep).items():
            new_keep[key] = _move(t, arena, f"{prefix}.{key}")
            for field, _ in struct._fields_:
                if getattr(struct, field) == t.data_ptr() and t.numel():
                    setattr(new_struct, field, arena.ptr(f"{prefix}.{key}"))
        return new_struct, new_keep
    out = copy.copy(table)
    for key, t in _tensors_of(table).items():
        setattr(out, key, _move(t, arena, f"{prefix}.{key}"))
    return out


def _move(t: torch.Tensor, arena: Arena, name: str) -> torch.Tensor:
    view = arena.carve(name, t.numel() * t.element_size(), t.dtype, tuple(t.shape))
    arena.fill(name, t)
    return view


def input_names(arena: Arena, *prefixes: str):
    return [name for name in arena.regions if name.startswith(tuple(p + "." for p in prefixes))]
