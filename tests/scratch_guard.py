"""Poisoned, guarded scratch for tests (imported like detinit.py; not a conftest, nothing here runs by itself).

``with guarded_scratch(fill=...):`` replaces, by plain attribute patching that is undone on exit,

* ``tomosar2height_amd._lib.workspace``: the buffer a launch gets is a uint8 view of exactly ``max(nbytes, 1)`` bytes, 512-byte
  aligned, inside a larger allocation with a guard band of ``GUARD`` (64 KiB) bytes of 0xFF on either side;
* ``torch.empty`` / ``empty_like`` / ``empty_strided`` / ``Tensor.new_empty``: the same call, then a fill of the new tensor's
  whole storage.  Only tensors on a device type in ``device_types`` are touched.

What a buffer holds when it is handed out:

=========  ==========================  =====================  ===================================  ====================================
``fill``   raw workspace               ... at an integer site  typed floating tensor                typed integer / bool tensor
=========  ==========================  =====================  ===================================  ====================================
"nan"      0xFF bytes                  recorded, else zero    0xFF bytes (NaN in f16/bf16/f32/f64)  stale from ``record``, else zero
"stale"    the recorded run's buffer   recorded               0xFF bytes                           stale from ``record`` (required)
"zero"     zero                        recorded, else zero    zero                                 zero
"record"   zero                        zero                   0xFF bytes                           zero
=========  ==========================  =====================  ===================================  ====================================

"record" is the fill of the run whose ``.log`` a stale run replays: its raw workspaces start from zero, so a slot that neither
run writes holds zero in the replay, never 0xFF.  ``nan_sites``: under "stale", a raw workspace whose call site contains one of
these strings (``"ops.py:222"``) holds floating data only and gets a fresh 0xFF buffer instead of the recorded one.

Integer tensors, and raw workspaces that hold integers, never get 0xFF: a kernel that used an unwritten one as an index would turn a latent bug into a wild address.
``int_sites`` is the mirror of ``nan_sites`` for that rule: a raw workspace whose call site matches one of them holds the recorded
run's bytes whenever a ``record`` is being replayed and zero otherwise, under EVERY fill, and whatever ``nan_sites`` says.  The
default, ``INT_SITES``, names the tile builds (``TileIndex.__init__`` / ``_init_ragged`` in tile.py: sort keys, histograms, scans).
A stale value is what the SAME call sequence left there on another input of the same shape, so it is in range for the shape.
``record=`` takes the ``.log`` of an earlier ``guarded_scratch`` block; the allocation sequence (kind and byte count) of the
replaying block must equal the recorded one -- any difference raises ``ScratchGuardError``, there is no fall-back.

A site is a substring of ``"<file>:<line> (<function>)"``, or a tuple of substrings that must all occur.

Workspaces that outlive the block (``fresh_sites``, default ``FRESH_SITES``: the split-weight buffers of grid.py's
``SplitWeightCache._get``, which live as long as their weight and are updated in place).  The view keeps its banded allocation
alive and the bands are checked when the block exits, so outliving it is harmless.  But under "stale" the recorded run's buffer
itself may still be some live weight's cache entry, and handing it out again would alias two entries.  The choice made here: such
a site gets a FRESH banded buffer holding a COPY of the recorded bytes (the recording model need not be dropped first).  The
allocation-sequence check (kind, byte count) holds for these sites like for any other.  They hold packed 16-bit planes and a
trailer of scale and exponent, never an index, so under "nan" (or as a ``nan_sites`` member) they take 0xFF.

On exit: ``torch.cuda.synchronize()`` (side streams are in use), then every guard band is compared byte for byte; a damaged
one raises ``ScratchGuardError`` naming the call site of the allocation.  Every buffer is kept alive until then.
Not for use under hipGraph capture.

Does NOT catch: a READ outside a buffer; a race that is usually won; anything under capture; an overrun of a typed tensor (an
output, an index list kept by its caller) -- only ``_lib.workspace`` buffers are banded, which since the tile builds and the
split-weight cache allocate through it is every raw byte buffer of the package (test_scratch_guard_cpu.py reads the sources).
"""
import sys

import torch

GUARD = 64 * 1024
ALIGN = 512
FILLS = ("nan", "stale", "zero", "record")
_TORCH_FUNCS = ("empty", "empty_like", "empty_strided")
_THIS = __file__.rsplit(".", 1)[0]
_REAL_EMPTY = torch.empty            # (the builtin, taken before any block patches it)
INT_SITES = ("/tile.py:",)           # raw workspaces of integers: TileIndex.__init__ / _init_ragged (the only two of that file)
FRESH_SITES = (("/grid.py:", "(_get)"),)     # SplitWeightCache._get: the buffer lives on in the cache


class ScratchGuardError(AssertionError):
    pass


def _bytes_of(t):
    """uint8 view of the whole storage behind ``t`` (any strides, any dtype)."""
    return _REAL_EMPTY(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())


def _call_site():
    f = sys._getframe(2)
    while f is not None and (f.f_code.co_filename.rsplit(".", 1)[0] == _THIS or "/torch/" in f.f_code.co_filename):
        f = f.f_back
    return "<unknown>" if f is None else f"{f.f_code.co_filename}:{f.f_lineno} ({f.f_code.co_name})"


def _hit(site, keys):
    return any(all(p in site for p in ((k,) if isinstance(k, str) else k)) for k in keys)


class guarded_scratch:
    def __init__(self, fill="nan", device_types=("cuda",), record=None, guard=GUARD, nan_sites=(), int_sites=INT_SITES,
                 fresh_sites=FRESH_SITES):
        if fill not in FILLS:
            raise ValueError(f"fill must be one of {FILLS}")
        if fill == "stale" and record is None:
            raise ValueError('fill="stale" needs record= (the .log of the recording run)')
        if guard < GUARD:
            raise ValueError(f"guard bands are at least {GUARD} bytes")
        self.fill, self.device_types, self.record, self.guard = fill, tuple(device_types), record, guard
        self.nan_sites, self.int_sites, self.fresh_sites = tuple(nan_sites), tuple(int_sites), tuple(fresh_sites)
        self.log = []              # ("ws" | "typed", nbytes, tensor, ...) in allocation order; holds every buffer alive
        self._next = 0
        self._saved = None

    # ------------------------------------------------------------------------------------------------- allocation
    def _recorded(self, kind, nbytes, site):
        """The recorded run's entry for this allocation, or None when nothing is being replayed."""
        if self.record is None:
            return None
        i, self._next = self._next, self._next + 1
        if i >= len(self.record) or self.record[i][:2] != (kind, nbytes):
            was = "nothing" if i >= len(self.record) else f"{self.record[i][0]} of {self.record[i][1]} bytes"
            raise ScratchGuardError(f"stale replay: allocation {i} is a {kind} of {nbytes} bytes at {site}; the recorded run made "
                                    f"{was} there")
        return self.record[i]

    def _workspace(self, nbytes, device):
        device = torch.device(device)
        n = max(int(nbytes), 1)
        if device.type not in self.device_types:
            return self._real["workspace"](nbytes, device)
        site = _call_site()
        rec = self._recorded("ws", n, site)
        integer = _hit(site, self.int_sites)
        replay = rec is not None and (integer or (self.fill == "stale" and not _hit(site, self.nan_sites)))
        if replay and not _hit(site, self.fresh_sites):
            entry = ("ws", n) + rec[2:5] + (site,)             # the same buffer again, unmodified; its guards are checked again
        else:
            buf = self._real["empty"](n + 2 * self.guard + ALIGN, dtype=torch.uint8, device=device)
            off = self.guard + (-(buf.data_ptr() + self.guard)) % ALIGN
            buf.fill_(0xFF)
            view = buf[off:off + n]
            if replay:
                view.copy_(rec[2])                             # (a buffer that outlives the block: a copy of the recorded bytes)
            elif integer or self.fill in ("zero", "record"):
                view.zero_()
            entry = ("ws", n, view, buf, off, site)
        self.log.append(entry)
        return entry[2]

    def _typed(self, t):
        if not isinstance(t, torch.Tensor) or t.device.type not in self.device_types:
            return t
        raw = _bytes_of(t)
        rec = self._recorded("typed", raw.numel(), None if self.record is None else _call_site())
        if self.fill == "zero":
            raw.zero_()
        elif t.is_floating_point() or t.is_complex():
            raw.fill_(0xFF)
        elif rec is not None:
            raw.copy_(_bytes_of(rec[2]))
        else:
            raw.zero_()
        self.log.append(("typed", raw.numel(), t))
        return t

    # ------------------------------------------------------------------------------------------------- patching
    def __enter__(self):
        from tomosar2height_amd import _lib
        self._real = {"workspace": _lib.workspace, "new_empty": torch.Tensor.new_empty}
        self._real.update({k: getattr(torch, k) for k in _TORCH_FUNCS})
        self._saved = [(_lib, "workspace", _lib.__dict__["workspace"], True)]
        self._saved += [(torch, k, getattr(torch, k), k in torch.__dict__) for k in _TORCH_FUNCS]
        self._saved.append((torch.Tensor, "new_empty", torch.Tensor.new_empty, "new_empty" in torch.Tensor.__dict__))
        real = self._real

        def wrap(k):
            def patched(*a, **kw):
                return self._typed(real[k](*a, **kw))
            patched.__name__ = k
            return patched

        _lib.workspace = self._workspace
        for k in _TORCH_FUNCS:
            setattr(torch, k, wrap(k))
            # the package's own aliases of the allocator (deferred._empty = torch.empty), bound before this block
            for name, mod in list(sys.modules.items()):
                if name.startswith("tomosar2height_amd"):
                    for attr, value in list(getattr(mod, "__dict__", {}).items()):
                        if value is real[k]:
                            self._saved.append((mod, attr, value, True))
                            setattr(mod, attr, getattr(torch, k))
        torch.Tensor.new_empty = wrap("new_empty")
        return self

    def _restore(self):
        for owner, name, value, own in self._saved or ():
            if own:
                setattr(owner, name, value)
            else:
                delattr(owner, name)
        self._saved = None

    def damaged(self):
        """[(call site, nbytes, first damaged offset relative to the view)] over every workspace handed out."""
        out = []
        for _, n, _view, buf, off, site in (e for e in self.log if e[0] == "ws"):
            for lo, hi in ((0, off), (off + n, buf.numel())):
                bad = (buf[lo:hi] != 0xFF).nonzero()
                if bad.numel():
                    out.append((site, n, int(bad[0]) + lo - off))
        return out

    def __exit__(self, etype, evalue, tb):
        self._restore()
        if "cuda" in self.device_types and torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        if etype is not None:
            return False
        if self.record is not None and self._next != len(self.record):
            raise ScratchGuardError(f"stale replay: {self._next} allocations, the recorded run made {len(self.record)}")
        bad = self.damaged()
        if bad:
            raise ScratchGuardError("write outside a workspace: " + "; ".join(
                f"{n}-byte workspace allocated at {site}, byte {o:+d} relative to its start" for site, n, o in bad))
        return False
