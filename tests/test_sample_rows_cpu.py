"""CPU (no GPU needed): what t2h_sample_rows_fwd / _bwd (csrc/bicubic.hip) rest on.

* The cell window of include/t2h.h, restated in numpy: the gather adjoint visits, for pixel p of an axis, the level cells
  lo(p) .. hi(p).  It is right only if that window contains the cell of EVERY point one of whose clamped taps (bicubic) or whose
  rounded index (nearest) is p -- checked here over dense float32 coordinates, every cell and pixel boundary with its float32
  neighbours, points outside [0, 1) (which the tile build clamps into the border cells) and the points of resample_ref.
* Every refusal of the two entry points, before any launch.
* ``ops.sample_plane_mode`` no longer refuses ragged batches.
"""
import ctypes
import inspect

import numpy as np
import pytest

import resample_ref as rr

RESOLUTIONS = (1, 2, 4, 8, 16, 256)


def window(r):
    """(lo, hi) int arrays over the pixels of an axis: include/t2h.h, "The window"."""
    p = np.arange(r, dtype=np.int64)
    if r == 1:
        return np.zeros(1, np.int64), np.zeros(1, np.int64)
    lo = np.maximum(np.maximum(p - 2, 0) * r // (r - 1) - 1, 0)
    hi = np.minimum((p + 2) * r // (r - 1) + 1, r - 1)
    return lo, hi


def build_cell(x, r):
    """Level cell of float32 coordinates on an axis, as csrc/tile_index.hip places them: floor(x R) >> k = floor(x r) inside
    [0, 1) (x R is exact: R is a power of two), clamped into the border cells outside."""
    return np.clip(np.floor(x.astype(np.float64) * r), 0, r - 1).astype(np.int64)


def pixels_reached(x, r):
    """[len(x), 6] pixels of an axis that a float32 coordinate can touch: the four clamped bicubic taps of the float32 product
    x (r - 1) the kernels form, and the nearest index of that product and of the exact product resample_ref uses."""
    fx = x * np.float32(r - 1)
    assert fx.dtype == np.float32
    f = np.floor(fx.astype(np.float64)).astype(np.int64)
    taps = [np.clip(f - 1 + k, 0, r - 1) for k in range(4)]
    near32 = np.rint(np.clip(fx.astype(np.float64), 0.0, r - 1.0)).astype(np.int64)
    near64 = np.rint(np.clip(x.astype(np.float64) * (r - 1), 0.0, r - 1.0)).astype(np.int64)
    return np.stack(taps + [near32, near64], axis=1)


def coordinates(r):
    grid = np.arange(-1024, 5121, dtype=np.float64) / 4096.0                                  # [-0.25, 1.25] in steps of 2^-12
    edges = [np.arange(r + 1) / r]                                                            # cell boundaries
    if r > 1:
        edges += [np.arange(-3, r + 3) / (r - 1), (np.arange(-3, r + 3) + 0.5) / (r - 1)]     # floor and rounding boundaries
    edges = np.concatenate(edges).astype(np.float32)
    below, above = np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf))
    near = [edges, below, above, np.nextafter(below, np.float32(-np.inf)), np.nextafter(above, np.float32(np.inf))]
    pts = np.concatenate([rr.points(q, 3, 300)[..., :2].ravel() for q in (max(r, 2), 5, 9)])
    far = np.asarray([-7.0, -1.0, -2.0 ** -30, 2.0, 9.5, 1e6, -1e6], np.float32)
    return np.unique(np.concatenate([grid.astype(np.float32), *near, pts, far, np.asarray([rr.BELOW_ONE], np.float32)]))


@pytest.mark.parametrize("r", RESOLUTIONS)
def test_cell_window_contains_every_point_that_reaches_the_pixel(r):
    lo, hi = window(r)
    assert (lo >= 0).all() and (hi <= r - 1).all() and (lo <= hi).all()
    assert (hi - lo + 1 <= 8).all()                      # the kernel keeps a window's cell ranges in 8 x 8 lanes
    assert lo[0] == 0 and hi[-1] == r - 1                # the border cells hold the points outside [0, 1)
    if r > 1:
        assert lo[1] == 0 and hi[-2] == r - 1            # a point just outside still has taps on the second pixel
    x = coordinates(r)
    cell, pix = build_cell(x, r), pixels_reached(x, r)
    inside = (lo[pix] <= cell[:, None]) & (cell[:, None] <= hi[pix])
    assert inside.all(), [(float(x[i]), int(cell[i]), pix[i].tolist()) for i in np.nonzero(~inside.all(axis=1))[0][:5]]
    # the taps above are a superset of where resample_ref puts a non-zero weight
    sub = x[:: max(1, len(x) // 500)]
    rows = rr.rows((sub * np.float32(r - 1)).astype(np.float64), r, "cubic")
    reach = pixels_reached(sub, r)
    for i, row in enumerate(rows):
        assert set(np.nonzero(row)[0]) <= set(reach[i, :4].tolist())


def test_cell_window_is_not_vacuous():
    """The same property fails for a window without its one-cell margin at the far end (so the check above can fail)."""
    r = 16
    lo, hi = window(r)
    x = coordinates(r)
    cell, pix = build_cell(x, r), pixels_reached(x, r)
    short = hi - 2
    assert not ((lo[pix] <= cell[:, None]) & (cell[:, None] <= short[pix])).all()


# ------------------------------------------------------------------------------------------------ refusals
def _refusals():
    buf = ctypes.create_string_buffer(256)                 # never read: every row returns before a launch
    p = ctypes.addressof(buf)
    #            plane pts dim off0 B  N    nbits r  C  cl mode out
    good = dict(a=p, pts=p, dim=4, off0=p, B=2, N=-10, nbits=3, r=8, C=5, cl=0, mode=1, out=p)
    rows = [
        (dict(a=None), "null pointer"), (dict(pts=None), "null pointer"), (dict(off0=None), "null pointer"),
        (dict(out=None), "null pointer"),
        (dict(B=0), "bad shape"), (dict(C=0), "bad shape"),
        (dict(B=65), "at most 64 tiles"),
        (dict(dim=1, N=10), "dim=1"), (dict(dim=2), "dim=2"),
        (dict(nbits=0), "nbits=0 outside [1, 10]"), (dict(nbits=11), "nbits=11 outside [1, 10]"),
        (dict(r=0), "power of two"), (dict(r=6), "power of two"), (dict(r=16), "power of two"),
        (dict(mode=2), "mode must be 0 (nearest) or 1 (bicubic)"), (dict(mode=-1), "mode must be 0 (nearest) or 1 (bicubic)"),
    ]
    return good, rows


@pytest.mark.parametrize("entry", ["t2h_sample_rows_fwd", "t2h_sample_rows_bwd"])
def test_sample_rows_refusals(entry):
    from tomosar2height_amd import _lib
    lib = _lib.load()
    good, rows = _refusals()
    for change, message in rows:
        a = dict(good, **change)
        rc = getattr(lib, entry)(a["a"], a["pts"], a["dim"], a["off0"], a["B"], a["N"], a["nbits"], a["r"], a["C"], a["cl"], a["mode"],
                                 a["out"], None)
        text = lib.t2h_last_error_string().decode()
        assert rc == -1, (change, rc)
        assert message in text and text.startswith(entry[4:] + ":"), (change, text)
    # a regular batch takes B above the ragged limit and dim = 2; with zero rows the forward returns before any launch
    a = dict(good, B=65, N=0, dim=2)
    assert lib.t2h_sample_rows_fwd(a["a"], a["pts"], a["dim"], a["off0"], a["B"], a["N"], a["nbits"], a["r"], a["C"], a["cl"], a["mode"],
                                   a["out"], None) == 0


def test_sample_plane_mode_takes_ragged_batches():
    from tomosar2height_amd import _lib, ops
    text = inspect.getsource(ops.sample_plane_mode)
    assert "batches only" not in text and "NotImplementedError" not in text
    assert "t2h_sample_rows_fwd" in inspect.getsource(ops._SampleRows) and "t2h_sample_rows_bwd" in inspect.getsource(ops._SampleRows)
    assert "save_for_backward" not in inspect.getsource(ops._SampleRows)         # the forward keeps nothing but the index
    assert _lib.SIGNATURES["t2h_sample_rows_fwd"] == _lib.SIGNATURES["t2h_sample_rows_bwd"]
