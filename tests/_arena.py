"""Guarded placement of device memory for the memory-contract tests (tests/test_memory_contract.py).

An Arena is ONE uint8 CUDA tensor.  ``place(nbytes)`` / ``put(tensor)`` / ``empty(shape, dtype)`` hand out views of it
whose first byte is on a 256-byte boundary (what torch's allocator and hipMalloc give a caller, and what the workspace
text of include/cgps.h relies on) and whose neighbours are at least GUARD = 64 KiB of memory that belongs to nobody:
every byte of the arena that is not inside a view is guard.  A kernel that writes a little past the end (or before the
start) of what it was given lands in a guard, in memory this process owns, and ``assert_guards`` sees it; a kernel that
reads there, or reads a slot of its workspace that it never wrote, gets the poison byte, and the results of a run with
0xFF poison (NaN in both precisions, -1 as an int) and of a run with 0x00 poison differ.

Nothing here writes outside the arena's own tensor, and a view never has spare bytes behind it: a workspace view has
``numel() == nbytes`` exactly (not torch's 512-byte allocation granule, not the grow-only cache of ``_hip._scratch``)."""
import contextlib

import torch

GUARD = 64 * 1024
ALIGN = 256


def _up(n, a=ALIGN):
    return (n + a - 1) // a * a


def capacity_for(sizes):
    """Bytes an arena needs for views of these sizes, every one between two guards."""
    return sum(_up(int(n)) + GUARD + ALIGN for n in sizes) + GUARD + ALIGN


def nbytes_of(shape, dtype):
    n = 1
    for s in shape:
        n *= int(s)
    return n * torch.empty((), dtype=dtype).element_size()


class Arena:
    def __init__(self, capacity, device="cuda"):
        self.buf = torch.empty(int(capacity) + ALIGN, dtype=torch.uint8, device=device)
        self._skew = (-self.buf.data_ptr()) % ALIGN          # (0 with torch's allocator; not assumed)
        self._pos = 0                                        # one past the last view, from the skewed start
        self.views = []                                      # (name, offset into buf, nbytes), in placement order
        self._names = {}                                     # (data_ptr, nbytes) of a handed-out view -> index

    # ---- placement ------------------------------------------------------------------------------------------------
    def place(self, nbytes, name=None):
        """uint8 view of exactly nbytes bytes, 256-byte aligned, GUARD bytes of nobody's memory on both sides"""
        nbytes = int(nbytes)
        off = self._skew + _up(self._pos + GUARD)
        if off + nbytes + GUARD > self.buf.numel():
            raise RuntimeError("arena of %d bytes is full: view %r of %d bytes at offset %d" % (self.buf.numel(), name, nbytes, off))
        self._pos = off - self._skew + nbytes
        v = self.buf[off:off + nbytes]
        assert v.numel() == nbytes and (nbytes == 0 or v.data_ptr() % ALIGN == 0)
        self._names[(v.data_ptr(), nbytes)] = len(self.views)
        self.views.append((name or "view%d" % len(self.views), off, nbytes))
        return v

    def empty(self, shape, dtype, name=None):
        """typed view of that shape; its bytes are whatever the arena holds there (the poison, after ``poison``)"""
        shape = tuple(int(s) for s in shape)
        return self.place(nbytes_of(shape, dtype), name).view(dtype).reshape(shape)

    def put(self, t, name=None):
        """a copy of t (made contiguous) inside the arena"""
        v = self.empty(t.shape, t.dtype, name)
        v.copy_(t)
        return v

    # ---- guards ---------------------------------------------------------------------------------------------------
    def _index(self, which):
        if isinstance(which, str):
            hits = [i for i, (n, _, _) in enumerate(self.views) if n == which]
            assert len(hits) == 1, (which, [n for n, _, _ in self.views])
            return hits[0]
        return self._names[(which.data_ptr(), which.numel() * which.element_size())]

    def gaps(self):
        """[(lo, hi, view before or None, view after or None)]: every stretch of the arena outside the views"""
        out, lo, prev = [], 0, None
        for i, (_, off, n) in enumerate(self.views):
            out.append((lo, off, prev, i))
            lo, prev = off + n, i
        out.append((lo, self.buf.numel(), prev, None))
        return out

    def poison(self, byte, interiors=()):
        """fill every guard, and the interiors of the views listed (by name or by the tensor handed out), with `byte`"""
        for lo, hi, _, _ in self.gaps():
            self.buf[lo:hi].fill_(byte)
        for w in interiors:
            _, off, n = self.views[self._index(w)]
            self.buf[off:off + n].fill_(byte)

    def interior(self, which):
        _, off, n = self.views[self._index(which)]
        return self.buf[off:off + n]

    def assert_guards(self, byte):
        """every guard byte still holds `byte` (compared on the device; one word comes back unless something is wrong)"""
        gaps = self.gaps()
        bad = torch.stack([(self.buf[lo:hi] != byte).any() for lo, hi, _, _ in gaps])
        if not bool(bad.any()):
            return
        msgs = []
        for (lo, hi, before, after), b in zip(gaps, bad.tolist()):
            if not b:
                continue
            idx = torch.nonzero(self.buf[lo:hi] != byte).flatten()
            first, last = lo + int(idx[0]), lo + int(idx[-1])
            where = []
            if before is not None:
                n, off, nb = self.views[before]
                where.append("%d .. %d bytes past the END of %r (%d bytes)" % (first - (off + nb), last - (off + nb), n, nb))
            if after is not None:
                n, off, nb = self.views[after]
                where.append("%d .. %d bytes before the START of %r" % (off - last, off - first, n))
            msgs.append("%d guard bytes changed: %s" % (idx.numel(), "; ".join(where)))
        raise AssertionError("written outside the views of the arena (poison 0x%02X): " % byte + " | ".join(msgs))

    # ---- routing the library wrappers' own allocations into the arena --------------------------------------------------
    @contextlib.contextmanager
    def exact_scratch(self, hip_module):
        """Inside the block ``_hip._scratch`` -- behind every ``_hip.*workspace`` -- hands out a fresh view of EXACTLY the
        bytes asked for (``numel() == nbytes``), between guards, instead of its grow-only cache.  ``self.scratch`` lists the
        views in the order of the calls; a view's name carries ``self.label``, which the test sets to the operation."""
        self.scratch = []

        def scratch(cache, nbytes, device):
            v = self.place(nbytes, "workspace %d (%s)" % (len(self.scratch), getattr(self, "label", "")))
            assert v.numel() == nbytes
            self.scratch.append(v)
            return v
        old = hip_module._scratch
        hip_module._scratch = scratch
        try:
            yield self
        finally:
            hip_module._scratch = old

    @contextlib.contextmanager
    def route_allocations(self):
        """Inside the block the four allocation functions the wrappers use for their CUDA outputs (``torch.empty``,
        ``torch.zeros``, ``torch.empty_like``, ``torch.full``) return views of the arena, zero / fill semantics kept;
        ``torch.empty`` keeps whatever the arena holds there, i.e. the poison.  CPU tensors and everything torch
        allocates internally (``.to``, ``.clone``, ``cat`` ...) are untouched.  ``self.allocated`` lists the views."""
        real = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "full")}
        self.allocated = []

        def is_cuda(device):
            return device is not None and torch.device(device).type == "cuda"

        def size_of(args, kw):
            if "size" in kw:
                return tuple(kw.pop("size"))
            if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
                return tuple(args[0])
            return tuple(args)

        def view(shape, dtype):
            v = self.empty(shape, dtype or torch.get_default_dtype(), "alloc%d" % len(self.allocated))
            self.allocated.append(v)
            return v

        def empty(*args, **kw):
            if not is_cuda(kw.get("device")):
                return real["empty"](*args, **kw)
            return view(size_of(args, dict(kw)), kw.get("dtype"))

        def zeros(*args, **kw):
            if not is_cuda(kw.get("device")):
                return real["zeros"](*args, **kw)
            return view(size_of(args, dict(kw)), kw.get("dtype")).zero_()

        def full(size, fill_value, **kw):
            if not is_cuda(kw.get("device")):
                return real["full"](size, fill_value, **kw)
            dt = kw.get("dtype") or torch.tensor(fill_value).dtype
            return view(tuple(size), dt).fill_(fill_value)

        def empty_like(t, **kw):
            dev = kw.get("device", t.device)
            if not is_cuda(dev):
                return real["empty_like"](t, **kw)
            return view(tuple(t.shape), kw.get("dtype") or t.dtype)

        new = {"empty": empty, "zeros": zeros, "empty_like": empty_like, "full": full}
        for n, f in new.items():
            setattr(torch, n, f)
        try:
            yield self
        finally:
            for n, f in real.items():
                setattr(torch, n, f)
