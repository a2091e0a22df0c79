"""Poisoned buffers and guard bands for the kernel output-contract tests (tests/test_gpu_buffer_contract.py).

Every engine and most tests allocate with ``torch.zeros``, and many correct values here are exactly 0, so a skipped store, a read
before write or a store past the end of a buffer can go unseen.  This module gives a test buffers that make those visible:

- ``guarded(shape, dtype, device)`` allocates ``[guard | payload | guard]`` in ONE allocation.  Each guard is at least 4 KiB of a
  fixed byte pattern and the payload starts 256-byte aligned (the alignment a fresh torch tensor has, so the kernels take the same
  vector-store paths).  ``check_guards()`` names the buffer and the first changed byte, counted from the payload's start or end.
- ``shift`` (a multiple of the element size, default 0) DISPLACES the payload: it starts ``shift`` bytes past a 256-byte boundary,
  the pointer a C caller gets who carves arrays out of one pool, or slot t of a rollout buffer whose rows are an odd number of
  elements.  ``Arena(device, policy=...)`` derives every buffer's shift: ``"one"`` = one element of the buffer's own dtype,
  ``"mixed"`` = a residue that is a function of the buffer's NAME (float32 / int32 1..3 elements, float64 / int64 one element, uint8
  1..15 elements), so that the inputs and outputs of one launch are aligned differently from each other -- a kernel that peels to
  align its loads and reuses the peel for its stores shows up.  ``keep_aligned`` names the buffers whose documented contract demands
  an alignment (include/pdegym.h says so at the parameter): they stay at shift 0 (tests/test_gpu_pointer_alignment.py).
- ``poison_(t)`` fills a float or flag tensor with a recognisable pattern: the NaN 0x7FC0DEAD (float32), the NaN 0x7FF8DEADDEADBEEF
  (float64), 0xA5 (uint8).  The kernels produce canonical NaNs, so "still holds the poison bits" is an exact test.  Integer buffers
  that a kernel indexes with are never filled with arbitrary bits (a faulty reset would turn that into a wild access): poison them with
  an in-range wrong value of the caller's choosing (``fill_int_``).
- ``assert_written`` / ``assert_untouched`` compare bit patterns on a boolean mask or on an index expression.

Plain helper module (not a conftest): imported by the tests that need it.
"""
from __future__ import annotations

import zlib

import torch

GUARD_BYTES = 4096
ALIGN = 256
GUARD_BYTE = 0xC3              # float32 0xC3C3C3C3 = -391.5: neither zero, nor NaN, nor the poison
POISON_F32 = 0x7FC0DEAD
POISON_F64 = 0x7FF8DEADDEADBEEF
POISON_U8 = 0xA5

_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.uint8: torch.uint8, torch.int32: torch.int32,
             torch.int64: torch.int64}
_POISON = {torch.float32: POISON_F32, torch.float64: POISON_F64, torch.uint8: POISON_U8}


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's elements as same-width integers (bit patterns; NaN payloads and -0.0 stay distinct)."""
    return t.view(_INT_VIEW[t.dtype])


def poison_value(dtype) -> int:
    if dtype not in _POISON:
        raise TypeError(f"{dtype} is not poisoned with a bit pattern: integer buffers take an in-range wrong value (fill_int_)")
    return _POISON[dtype]


def poison_(t: torch.Tensor) -> torch.Tensor:
    """Fill ``t`` in place with the poison pattern of its dtype (float32, float64, uint8 only)."""
    bits(t).fill_(poison_value(t.dtype))
    return t


def fill_int_(t: torch.Tensor, value: int) -> torch.Tensor:
    """Integer state (time_index, reset_count, stage, days, ...): a wrong value that is still IN RANGE for every index the kernel forms."""
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"fill_int_ is for integer buffers, not {t.dtype}")
    t.fill_(int(value))
    return t


def _mask(t: torch.Tensor, where) -> torch.Tensor:
    """Boolean mask over ``t`` of the elements ``where`` picks: None (all), a boolean mask (broadcast to t), or an index expression."""
    if where is None:
        return torch.ones(t.shape, dtype=torch.bool, device=t.device)
    if torch.is_tensor(where) and where.dtype == torch.bool:      # a per-instance [B] mask covers the instance's whole row(s)
        w = where.to(t.device)
        return w.reshape(tuple(w.shape) + (1,) * (t.dim() - w.dim())).expand(t.shape)
    m = torch.zeros(t.shape, dtype=torch.bool, device=t.device)
    m[where] = True
    return m


def _check(t: torch.Tensor, where, bad_of, what: str, name: str):
    m = _mask(t, where)
    bad = bad_of(bits(t)) & m
    if bool(bad.any()):
        first = tuple(int(i) for i in torch.nonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {int(m.sum())} element(s) {what}; first at index {first}")


def assert_untouched(t: torch.Tensor, where=None, name: str = "buffer"):
    """Every element selected by ``where`` still holds the poison bits of its dtype."""
    p = poison_value(t.dtype)
    _check(t, where, lambda x: x != p, "that must be left alone were written", name)


def assert_written(t: torch.Tensor, where=None, name: str = "buffer", like: torch.Tensor | None = None):
    """Every element selected by ``where`` no longer holds the poison bits; with ``like``, it equals ``like`` bit for bit."""
    p = poison_value(t.dtype)
    _check(t, where, lambda x: x == p, "that must be written still hold the poison", name)
    if like is not None:
        assert_bits_equal(t, like, where, name)


def assert_bits_equal(a: torch.Tensor, b: torch.Tensor, where=None, name: str = "buffer"):
    """``a`` equals ``b`` bit for bit on the selection (e.g. the poisoned run against the clean one)."""
    b = b.to(a.device)
    if a.shape != b.shape or a.dtype != b.dtype:
        raise AssertionError(f"{name}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}")
    bb = bits(b)
    _check(a, where, lambda x: x != bb, "differ from the reference run", name)


class Guarded:
    """One ``[guard | payload | guard]`` allocation; ``t`` is the contiguous payload."""

    def __init__(self, name: str, shape, dtype, device, pinned: bool = False, shift: int = 0):
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        shift = int(shift)
        if not 0 <= shift < ALIGN or shift % item:
            raise ValueError(f"shift {shift} of '{name}' is not a multiple of the element size {item} below {ALIGN}")
        self.name, self.nbytes, self.shift = name, numel * item, shift
        # the head guard is GUARD_BYTES + shift: the payload starts `shift` bytes past a 256-byte boundary.  The tail guard starts
        # right at the payload's end (a one-element overrun lands in it) and runs to the next 256-byte boundary past another GUARD_BYTES
        head = GUARD_BYTES + shift
        tail = GUARD_BYTES + (-(shift + self.nbytes)) % ALIGN
        total = head + self.nbytes + tail
        if pinned:
            base = torch.empty(total + ALIGN, dtype=torch.uint8, pin_memory=True)
        else:
            base = torch.empty(total + ALIGN, dtype=torch.uint8, device=device)
        skip = (-base.data_ptr()) % ALIGN               # (the HIP allocator's blocks are aligned already; host memory may not be)
        self.raw = base[skip:skip + total]
        self.raw.fill_(GUARD_BYTE)
        self.t = self.raw[head:head + self.nbytes].view(dtype).view(shape)
        self.t.zero_()
        self._head = self.raw[:head]
        self._tail = self.raw[head + self.nbytes:]

    def check_guards(self):
        """Raise AssertionError naming the first changed guard byte: its distance before the payload, or after its end."""
        for part, before in ((self._head, True), (self._tail, False)):
            bad = part != GUARD_BYTE
            if bool(bad.any()):
                idx = torch.nonzero(bad)
                if before:
                    off = part.numel() - int(idx[-1].item())       # the changed byte closest to the payload
                    raise AssertionError(f"guard of '{self.name}' changed {off} byte(s) BEFORE the payload "
                                         f"({int(bad.sum())} byte(s) in all)")
                off = int(idx[0].item())
                raise AssertionError(f"guard of '{self.name}' changed at byte +{off} AFTER the payload end "
                                     f"({self.nbytes} bytes; {int(bad.sum())} byte(s) in all)")


def guarded(shape, dtype, device, pinned: bool = False, name: str = "buffer", shift: int = 0):
    """Allocate a guarded buffer: returns (payload tensor, check_guards).  The payload starts zero-filled."""
    g = Guarded(name, shape, dtype, device, pinned, shift)
    return g.t, g.check_guards


POLICIES = (None, "one", "mixed")


def policy_shift(policy, name: str, dtype) -> int:
    """Bytes past a 256-byte boundary at which the payload of buffer ``name`` starts under ``policy`` (see the module docstring)."""
    if policy is None:
        return 0
    item = torch.empty((), dtype=dtype).element_size()
    if policy == "one":
        return item
    if policy == "mixed":
        h = zlib.crc32(name.encode())                   # deterministic: the same name gets the same residue in every process
        if item == 1:
            return 1 + h % 15
        if item == 4:
            return 4 * (1 + h % 3)
        return item                                     # 8-byte elements: the one residue mod 16 that is not aligned
    raise ValueError(f"unknown displacement policy {policy!r}: one of {POLICIES}")


class Arena:
    """Named guarded buffers of one test case: ``a.new(name, shape, dtype)`` returns the payload; ``a.check()`` checks every guard."""

    def __init__(self, device, pinned: bool = False, policy: str | None = None, keep_aligned=()):
        policy_shift(policy, "", torch.uint8)           # (refuses an unknown policy here, not at the first buffer)
        self.device, self.pinned, self.bufs = device, pinned, {}
        self.policy, self.keep_aligned = policy, frozenset(keep_aligned)

    def shift_of(self, name: str, dtype) -> int:
        return 0 if name in self.keep_aligned else policy_shift(self.policy, name, dtype)

    def new(self, name: str, shape, dtype, pinned: bool | None = None):
        g = Guarded(name, shape, dtype, self.device, self.pinned if pinned is None else pinned, self.shift_of(name, dtype))
        self.bufs[name] = g
        return g.t

    def like(self, name: str, src: torch.Tensor):
        """A guarded copy of ``src``."""
        t = self.new(name, src.shape, src.dtype)
        t.copy_(src)
        return t

    def check(self):
        if self.device is not None and torch.device(self.device).type == "cuda":
            torch.cuda.synchronize()
        for g in self.bufs.values():
            g.check_guards()
