"""Guarded allocations for the memory-contract tests (include/posecnn_hip.h, "Conventions"): the library touches only the
caller's outputs and a workspace of exactly `pcnn_*_workspace_bytes`, never writes its inputs, and its results do not
depend on what the memory held before the call.

`GuardedTorch` stands in for `torch` inside posecnn_amd.ops / posecnn_amd.icp (monkeypatch.setattr(ops, "torch", proxy)).
Every `empty` / `empty_like` / `zeros` on a guarded device becomes an arena [guard | body | guard]: each guard is 1 MiB of
0xA5 bytes (one 64 x 4096 f32 fc block, so a store a whole block too far still lands in it) and the body is the returned
contiguous view. Pattern P1 starts the body at 0 mod 256 and fills `empty` bodies with 0xFF bytes (NaN, -1, 255); P2
starts it at 16 mod 256 (the ABI's minimum alignment) and fills them with the largest finite float, or zero bytes for
integer types. `zeros` stays zeros. `embed` puts an input into the same layout and remembers the whole arena, which must
come back byte for byte. `check()` verifies every arena after the work has finished.

Nothing here is specific to the GPU: the same code guards CPU tensors (the harness's own self-tests)."""
import traceback

import numpy as np
import torch as _torch

GUARD_BYTES = 1 << 20
GUARD_BYTE = 0xA5
PATTERNS = ("P1", "P2")
_BODY_OFFSET = {"P1": 0, "P2": 16}


class GuardError(AssertionError):
    pass


def poison_bytes(pattern, dtype):
    """The byte image of one element of an `empty` body under `pattern` (numpy dtype or torch dtype)."""
    if isinstance(dtype, _torch.dtype):
        dtype = _torch.empty((), dtype=dtype).numpy().dtype if dtype != _torch.uint16 else np.dtype(np.uint16)
    dtype = np.dtype(dtype)
    if pattern == "P1":
        return np.full(dtype.itemsize, 0xFF, np.uint8)
    if dtype.kind == "f":
        return np.array([np.finfo(dtype).max], dtype).view(np.uint8)
    return np.zeros(dtype.itemsize, np.uint8)


def _site():
    """The innermost frame outside this module: the allocating call site."""
    for fr in reversed(traceback.extract_stack()[:-1]):
        if fr.filename != __file__:
            return "%s:%d (%s)" % (fr.filename.rsplit("/", 1)[-1], fr.lineno, fr.name)
    return "?"


class Arena:
    __slots__ = ("buf", "start", "nbytes", "shape", "dtype", "site", "kind", "snapshot", "body")

    def describe(self):
        return "%s %s %s from %s" % (self.kind, tuple(self.shape), str(self.dtype).replace("torch.", ""), self.site)


class GuardedTorch:
    """`torch` with guarded `empty`, `empty_like` and `zeros` on the device types in `devices`; every other attribute
    (and every allocation elsewhere) is the real torch."""

    def __init__(self, pattern, devices=("cuda",)):
        if pattern not in _BODY_OFFSET:
            raise ValueError("pattern must be one of %s" % (PATTERNS,))
        self.pattern = pattern
        self.devices = tuple(devices)
        self.arenas = []

    def __getattr__(self, name):
        return getattr(_torch, name)

    # ---- allocation ---------------------------------------------------------------------------------------------
    def _guarded(self, device):
        return _torch.device(device).type in self.devices

    def _arena(self, shape, dtype, device, kind):
        shape = tuple(int(s) for s in shape)
        itemsize = _torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        buf = _torch.empty(nbytes + 2 * GUARD_BYTES + 512, dtype=_torch.uint8, device=device)
        start = (-buf.data_ptr()) % 256 + GUARD_BYTES + _BODY_OFFSET[self.pattern]
        buf.fill_(GUARD_BYTE)
        a = Arena()
        a.buf, a.start, a.nbytes, a.shape, a.dtype, a.site, a.kind, a.snapshot = buf, start, nbytes, shape, dtype, _site(), kind, None
        a.body = buf[start:start + nbytes].view(dtype).view(shape)
        self.arenas.append(a)
        return a

    def _poison(self, a):
        raw = a.buf[a.start:a.start + a.nbytes]
        if self.pattern == "P1":
            raw.fill_(0xFF)
        elif a.dtype.is_floating_point:
            a.body.fill_(_torch.finfo(a.dtype).max)
        else:
            raw.fill_(0)

    @staticmethod
    def _shape(size):
        if len(size) == 1 and isinstance(size[0], (tuple, list, _torch.Size)):
            return tuple(size[0])
        return tuple(size)

    def empty(self, *size, dtype=None, device=None):
        dtype = dtype or _torch.get_default_dtype()
        device = _torch.device(device) if device is not None else _torch.get_default_device()
        if not self._guarded(device):
            return _torch.empty(*size, dtype=dtype, device=device)
        a = self._arena(self._shape(size), dtype, device, "empty")
        self._poison(a)
        return a.body

    def empty_like(self, t, dtype=None, device=None):
        return self.empty(tuple(t.shape), dtype=dtype or t.dtype, device=device if device is not None else t.device)

    def zeros(self, *size, dtype=None, device=None):
        dtype = dtype or _torch.get_default_dtype()
        device = _torch.device(device) if device is not None else _torch.get_default_device()
        if not self._guarded(device):
            return _torch.zeros(*size, dtype=dtype, device=device)
        a = self._arena(self._shape(size), dtype, device, "zeros")
        a.buf[a.start:a.start + a.nbytes].zero_()
        return a.body

    def embed(self, value, device, mutable=False, kind="input"):
        """An input inside a guarded arena (numpy array or tensor; the bytes are copied as they are). Unless `mutable`
        (an argument written in place by contract), the whole arena must be unchanged at `check()`."""
        if isinstance(value, _torch.Tensor):
            src = value.detach().contiguous()
            shape, dtype = tuple(src.shape), src.dtype
            raw = src.reshape(-1).view(_torch.uint8) if src.numel() else None
        else:
            arr = np.ascontiguousarray(value)
            shape = arr.shape
            dtype = _torch.uint16 if arr.dtype == np.uint16 else _torch.from_numpy(arr[:0].reshape(-1)).dtype
            raw = _torch.from_numpy(arr.reshape(-1).view(np.uint8).copy()) if arr.size else None
        device = _torch.device(device)
        a = self._arena(shape, dtype, device, kind + (" (written in place)" if mutable else ""))
        if raw is not None:
            a.buf[a.start:a.start + a.nbytes].copy_(raw.to(device))
        if not mutable:
            a.snapshot = a.buf.clone()
        return a.body

    def refresh(self, t, value):
        """Copy new contents into an embedded input (same size) and take them as its reference bytes."""
        a = self.arena_of(t)
        src = value if isinstance(value, _torch.Tensor) else _torch.from_numpy(np.ascontiguousarray(value))
        a.body.copy_(src.to(a.body.device).view(a.body.shape))
        if a.snapshot is not None:
            a.snapshot = a.buf.clone()

    def arena_of(self, t):
        p = t.data_ptr()
        for a in self.arenas:
            if a.buf.data_ptr() + a.start == p and a.nbytes == t.numel() * t.element_size():
                return a
        raise KeyError("not a guarded tensor")

    # ---- verification -------------------------------------------------------------------------------------------
    def check(self):
        """Every guard intact and every read-only input byte-identical. Call after the work has finished
        (torch.cuda.synchronize() for device work)."""
        if not self.arenas:
            return
        flags = []
        for a in self.arenas:
            end = a.start + a.nbytes
            flags.append(_torch.stack([(a.buf[:a.start] != GUARD_BYTE).any(), (a.buf[end:] != GUARD_BYTE).any(),
                                       (a.buf != a.snapshot).any() if a.snapshot is not None else (a.buf[:0] != 0).any()]))
        flags = _torch.stack(flags).cpu().numpy()
        problems = []
        for a, (lo, hi, changed) in zip(self.arenas, flags):
            end = a.start + a.nbytes
            if lo:
                bad = (a.buf[:a.start] != GUARD_BYTE).nonzero()
                problems.append("%s: guard BEFORE the body hit, farthest store %d bytes before its start (%d bytes hit)" % (
                    a.describe(), a.start - int(bad[0]), len(bad)))
            if hi:
                bad = (a.buf[end:] != GUARD_BYTE).nonzero()
                problems.append("%s: guard AFTER the body hit, first store at byte %d past its end (%d bytes hit)" % (
                    a.describe(), int(bad[0]), len(bad)))
            if changed and not (lo or hi):
                bad = (a.buf != a.snapshot).nonzero()
                problems.append("%s: input modified, first changed byte at body offset %d (%d bytes)" % (
                    a.describe(), int(bad[0]) - a.start, len(bad)))
        if problems:
            raise GuardError("memory contract violated (pattern %s):\n  %s" % (self.pattern, "\n  ".join(problems)))


class Recorder:
    """Stands in for the ctypes library handle and logs every `pcnn_*` entry looked up on it."""

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.startswith("pcnn_"):
            self.calls.append(name)
        return fn


def to_numpy(t):
    t = t.detach()
    if t.dtype == _torch.uint16:
        t = t.view(_torch.int16)
        return t.cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _index_mask(shape, index):
    m = np.zeros(shape, bool)
    m[index] = True
    return m


def compare_patterns(runs, keep=None, zero=None):
    """runs: {pattern: {name: numpy array}}. Every output must be bit-identical between the patterns outside its
    `keep` region (left untouched by contract: it must still hold that pattern's poison), and zero inside its `zero`
    region."""
    keep, zero = keep or {}, zero or {}
    names = set(runs[PATTERNS[0]])
    for p in PATTERNS:
        if set(runs[p]) != names:
            raise GuardError("pattern %s returned %s, %s returned %s" % (PATTERNS[0], sorted(names), p, sorted(runs[p])))
    for name in sorted(names):
        a, b = (np.ascontiguousarray(runs[p][name]) for p in PATTERNS)
        if a.shape != b.shape or a.dtype != b.dtype:
            raise GuardError("%s: shape / dtype differ between patterns" % name)
        kept = _index_mask(a.shape, keep[name]) if name in keep else np.zeros(a.shape, bool)
        ab, bb = a.view(np.uint8).reshape(a.shape + (a.itemsize,)), b.view(np.uint8).reshape(b.shape + (b.itemsize,))
        diff = (ab != bb).any(-1) & ~kept
        if diff.any():
            i = tuple(np.argwhere(diff)[0])
            raise GuardError("%s: depends on the memory's previous contents: %d elements differ between %s and %s, "
                             "first at %s (%r vs %r) — an unwritten or uninitialised element" % (
                                 name, int(diff.sum()), PATTERNS[0], PATTERNS[1], i, a[i], b[i]))
        for p in PATTERNS:
            arr = np.ascontiguousarray(runs[p][name])
            raw = arr.view(np.uint8).reshape(arr.shape + (arr.itemsize,))
            if name in keep:
                untouched = (raw == poison_bytes(p, arr.dtype)).all(-1)
                bad = kept & ~untouched
                if bad.any():
                    raise GuardError("%s (%s): %d elements of the region documented as untouched were written, first at %s" % (
                        name, p, int(bad.sum()), tuple(np.argwhere(bad)[0])))
            if name in zero:
                zm = _index_mask(arr.shape, zero[name])
                bad = zm & (raw != 0).any(-1)
                if bad.any():
                    raise GuardError("%s (%s): %d elements of the documented zero region are not +0, first at %s" % (
                        name, p, int(bad.sum()), tuple(np.argwhere(bad)[0])))
