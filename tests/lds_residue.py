"""LDS residue for the kernel tests (tests/test_gpu_lds_residue.py): every kernel launch finds a chosen bit pattern in LDS.

LDS is not cleared between launches.  In this suite the kernel that ran before is nearly always the same kernel on similar data, so
what a workgroup finds in LDS is finite and plausible, and a kernel that reads one word it did not write passes every comparison.
``dirtied(pattern)`` makes the residue a pattern that cannot pass:

- ``"nan"``  0x7FF8DEAD_7FC0BEEF: every aligned 32-bit word is a quiet float32 NaN, every aligned 64-bit word a quiet float64 NaN;
- ``"huge"`` 0x7F7FFFFF_7F7FFFFF: finite and enormous in both views -- a leak into a sum changes bits but survives ``isfinite``;
- ``"ones"`` all bits set: a NaN as a float, -1 as an index, true as a flag.

Inside the context every export of ``_native.EXPORTS`` whose last parameter is the stream is wrapped: the wrapper first enqueues one
``lds_dirty`` launch (tests/hip/lds_residue.hip) on that same stream, then makes the real call.  The dirty launch is an ordinary
launch on the caller's stream, so it is captured into graphs along with the call.  ENTER THE CONTEXT BEFORE an engine or backend is
constructed: ``backend.py`` prepares calls that capture the function object.  On exit the originals are put back, and a wrapper
that a prepared call still holds becomes a pass-through.

The context counts entry calls and dirty launches; a test asserts ``entry_calls > 0`` and ``dirty_launches == entry_calls`` (a run
that dirtied nothing cannot pass).

KNOWN LIMIT: an entry point that makes several launches (the loss heads, FusedAdam, the backward passes, the f64 256x256 passes) is
dirtied before its FIRST launch only; its later launches find what the earlier ones left.  The product has no hook to change that.

Plain helper module (not a conftest): imported by the tests that need it.
"""
from __future__ import annotations

import ctypes as C

PATTERN_NAN = 0x7FF8DEAD_7FC0BEEF
PATTERN_HUGE = 0x7F7FFFFF_7F7FFFFF
PATTERN_ONES = 0xFFFFFFFF_FFFFFFFF
PATTERNS = {"nan": PATTERN_NAN, "huge": PATTERN_HUGE, "ones": PATTERN_ONES}

GROUPS_PER_CU = 8          # workgroups of one dirty launch, per CU (each asks for the largest LDS segment one workgroup may have)
SEEN_CAP = 1 << 16         # entries of the __smid() table a test hands to dirty()


def build_lib(force: bool = False) -> str:
    """tests/hip/lds_residue.hip -> pdecontrolgym_amd/lib/libpdegym_lds_residue.so, rebuilt when the source is newer
    (pdecontrolgym_amd/build.py: build_lds_residue, next to the HBM probe's recipe)."""
    from pdecontrolgym_amd import build
    return build.build_lds_residue(force)


_residue = None


def load():
    """The residue library (built on demand), prototypes declared."""
    global _residue
    if _residue is None:
        import torch  # noqa: F401  (first: one HIP runtime in the process, the one torch has loaded)
        lib = C.CDLL(build_lib())
        lib.lds_residue_info.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.lds_residue_info.restype = C.c_int
        lib.lds_dirty.argtypes = [C.c_uint64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.lds_dirty.restype = C.c_int
        lib.lds_witness.argtypes = [C.c_uint64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.lds_witness.restype = C.c_int
        lib.lds_pad_probe.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        lib.lds_pad_probe.restype = C.c_int
        _residue = lib
    return _residue


def info():
    """(CU count, bytes of LDS one dirty workgroup fills) of the current device."""
    cus, nbytes = C.c_int32(0), C.c_int32(0)
    if load().lds_residue_info(C.byref(cus), C.byref(nbytes)) != 0:
        raise RuntimeError("lds_residue_info failed: no HIP device, or the LDS segment size was refused")
    return cus.value, nbytes.value


def pattern_of(pattern) -> int:
    if isinstance(pattern, str):
        if pattern not in PATTERNS:
            raise ValueError(f"unknown LDS pattern {pattern!r}: one of {sorted(PATTERNS)}")
        return PATTERNS[pattern]
    return int(pattern) & 0xFFFFFFFF_FFFFFFFF


def dirty(pattern, stream, seen=None, groups_per_cu: int = GROUPS_PER_CU):
    """One lds_dirty launch on ``stream`` (a raw stream pointer); ``seen``: an int32 device tensor of SEEN_CAP zeros, or None."""
    rc = load().lds_dirty(pattern_of(pattern), None if seen is None else seen.data_ptr(), 0 if seen is None else seen.numel(),
                          groups_per_cu, stream)
    if rc != 0:
        raise RuntimeError("lds_dirty: the launch failed")


def witness(pattern, lds_bytes: int, grid: int, stream):
    """Launch lds_witness; returns (matching words per workgroup, __smid() per workgroup) as int64 / int32 device tensors."""
    import torch
    partial = torch.full((grid, 256), -1, dtype=torch.int32, device="cuda")
    smid = torch.full((grid,), -1, dtype=torch.int32, device="cuda")
    rc = load().lds_witness(pattern_of(pattern), lds_bytes, grid, partial.data_ptr(), smid.data_ptr(), stream)
    if rc != 0:
        raise RuntimeError(f"lds_witness: the launch failed ({lds_bytes} bytes, {grid} workgroups)")
    return partial.to(torch.int64).sum(dim=1), smid


def pad_probe(x, write_pad: bool, stream):
    """lds_pad_probe on the float32 device row ``x``: a kernel that stages the row "zero-padded to a multiple of four" and writes the
    pad (``write_pad``) or leaves it as found.  Returns [sum of row * w with w = 0 in the pad, plain sum of the padded row]."""
    import torch
    assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous()
    out = torch.full((2,), -1.0, dtype=torch.float32, device=x.device)
    if load().lds_pad_probe(x.data_ptr(), x.numel(), int(bool(write_pad)), out.data_ptr(), stream) != 0:
        raise RuntimeError("lds_pad_probe: the launch failed")
    return out


def stream_exports(lib, names=None):
    """The exports whose LAST parameter is the stream: the declared prototype ends in a ``void*`` (include/pdegym.h names it
    ``stream`` in every such entry point, and no entry point ends in another pointer; tests/test_lds_residue_helper.py holds
    this list to the header)."""
    if names is None:
        from pdecontrolgym_amd import _native as N
        names = N.EXPORTS
    out = []
    for name in names:
        at = getattr(getattr(lib, name), "argtypes", None)
        if at and at[-1] is C.c_void_p:
            out.append(name)
    return out


class _State:
    def __init__(self):
        self.live = True
        self.entry_calls = 0
        self.dirty_launches = 0
        self.by_entry = {}


_active = None


class dirtied:
    """Context manager: see the module docstring.  ``lib`` and ``dirty_fn`` are for the tests of this helper (a fake library
    object; ``dirty_fn(pattern_bits, stream)``); by default the product library and lds_dirty."""

    def __init__(self, pattern, lib=None, dirty_fn=None, names=None):
        self.pattern = pattern_of(pattern)
        self._lib, self._dirty_fn, self._names = lib, dirty_fn, names
        self._state = _State()
        self._saved = {}

    entry_calls = property(lambda self: self._state.entry_calls)
    dirty_launches = property(lambda self: self._state.dirty_launches)
    by_entry = property(lambda self: dict(self._state.by_entry))

    def _wrap(self, name, real):
        state, pattern, dirty_fn = self._state, self.pattern, self._dirty_fn

        def entry(*args):
            if state.live:
                state.entry_calls += 1
                state.by_entry[name] = state.by_entry.get(name, 0) + 1
                dirty_fn(pattern, args[-1])
                state.dirty_launches += 1
            return real(*args)

        entry.__name__ = name
        entry.argtypes, entry.restype = real.argtypes, getattr(real, "restype", None)
        entry.lds_dirtied_original = real
        return entry

    def __enter__(self):
        global _active
        if _active is not None:
            raise RuntimeError("dirtied() does not nest: the exports are wrapped already")
        if self._lib is None:
            from pdecontrolgym_amd import _native as N
            self._lib = N.load()
        if self._dirty_fn is None:
            info()                       # (the LDS opt-in of the dirty kernel happens here, outside of any stream capture)
            self._dirty_fn = lambda pattern, stream: dirty(pattern, stream)
        _active = self
        try:
            for name in stream_exports(self._lib, self._names):
                real = getattr(self._lib, name)
                self._saved[name] = real
                setattr(self._lib, name, self._wrap(name, real))
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        global _active
        self._state.live = False                     # wrappers that a prepared call still holds: pass-throughs from here on
        for name, real in self._saved.items():
            setattr(self._lib, name, real)
        self._saved = {}
        _active = None
        return False

    def check(self, *entries, exact=False):
        """What every test asserts: something was dirtied, every entry call was, and the named entry points were among them --
        with ``exact``, they and no other: a call that went round the wrappers (an engine built outside the context holds the
        unwrapped functions) then shows as a named entry point that was never counted."""
        assert self.entry_calls > 0, "no entry point was called inside dirtied(): the case proved nothing"
        assert self.dirty_launches == self.entry_calls, (self.dirty_launches, self.entry_calls)
        for e in entries:
            assert self._state.by_entry.get(e, 0) > 0, f"{e} was not called inside dirtied(): {sorted(self._state.by_entry)}"
        if exact:
            assert sorted(self._state.by_entry) == sorted(set(entries)), f"entry points called inside dirtied(): {sorted(self._state.by_entry)}"
