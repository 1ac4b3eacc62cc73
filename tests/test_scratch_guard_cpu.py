"""The scratch-guard harness (tests/scratch_guard.py) proves on CPU tensors, with plain torch stand-ins for a kernel, that it
would fail; and the case table of test_scratch_guard_gpu.py is checked against the size queries the sources export."""
import glob
import os
import re

import pytest
import torch

from scratch_guard import GUARD, ScratchGuardError, guarded_scratch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = ("cpu",)


def _launch(x, ws_floats, reads, overrun=0, written=None):
    """Stand-in for a wrapper + kernel: a workspace of ``ws_floats`` floats, of which the first ``written`` (default ``len(x)``)
    are written -- how many may depend on the input's values, like the rows of a split that got none; the result sums the
    first ``reads`` floats.  ``overrun``: bytes written past the end of the workspace."""
    from tomosar2height_amd import _lib
    ws = _lib.workspace(4 * ws_floats, x.device)
    part = ws.view(torch.float32)
    written = x.numel() if written is None else written
    part[:written] = x[:written]
    if overrun:
        base = ws._base if ws._base is not None else ws             # the kernel only has the pointer: write through it
        start = ws.storage_offset() + ws.numel()
        base[start:start + overrun] = 0
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    out[0] = part[:reads].sum()
    return out


def _under(fill, x, written_a=None, **kw):
    rec = None
    if fill == "stale":
        with guarded_scratch("record", CPU) as a:                   # run A: same calls, another input of the same shape
            _launch(x + 100.0, **dict(kw, written=written_a or kw.get("written")))
        rec = a.log
    with guarded_scratch(fill, CPU, record=rec):
        return _launch(x, **kw)


def test_one_byte_past_the_workspace_is_reported_with_its_call_site():
    x = torch.arange(4.0)
    with pytest.raises(ScratchGuardError) as e:
        with guarded_scratch("zero", CPU):
            _launch(x, ws_floats=4, reads=4, overrun=1)
    msg = str(e.value)
    assert "test_scratch_guard_cpu.py" in msg and "_launch" in msg and "16-byte workspace" in msg and "byte +16" in msg
    with guarded_scratch("zero", CPU):                              # the same launch inside its bytes passes
        _launch(x, ws_floats=4, reads=4)


def test_guard_layout():
    from tomosar2height_amd import _lib
    with guarded_scratch("nan", CPU) as g:
        a, b = _lib.workspace(0, "cpu"), _lib.workspace(1000, torch.device("cpu"))
        e = torch.empty(3, 5)
        i = torch.empty(7, dtype=torch.int64)
    assert a.numel() == 1 and b.numel() == 1000 and a.dtype == b.dtype == torch.uint8
    for _, n, view, buf, off, _site in g.log[:2]:
        assert view.data_ptr() % 512 == 0 and off >= GUARD and buf.numel() - off - n >= GUARD
        assert bool((buf[:off] == 0xFF).all()) and bool((buf[off + n:] == 0xFF).all())
    assert bool((b == 0xFF).all()) and bool(e.isnan().all()) and bool((i == 0).all())
    for dt in (torch.float16, torch.bfloat16, torch.float64):
        with guarded_scratch("nan", CPU):
            assert bool(torch.empty(5, dtype=dt).isnan().all())


def test_unwritten_float_of_the_workspace_shows_in_the_value():
    x = torch.arange(1.0, 7.0)                                      # this input fills four slots, the recorded one all six
    nan = _under("nan", x, ws_floats=6, reads=6, written=4)
    stale = _under("stale", x, ws_floats=6, reads=6, written=4, written_a=6)
    zero = _under("zero", x, ws_floats=6, reads=6, written=4)
    assert bool(nan.isnan().all())
    assert zero.item() == 10.0
    assert stale.item() == 10.0 + 105.0 + 106.0                    # what the recorded run left in slots 4 and 5
    assert not torch.equal(stale.view(torch.int32), zero.view(torch.int32))


def test_well_behaved_launch_is_bit_identical_under_all_fills():
    x = torch.randn(9, generator=torch.Generator().manual_seed(1))
    clean = _launch(x, ws_floats=9, reads=9)
    for fill in ("nan", "stale", "zero"):
        got = _under(fill, x, ws_floats=9, reads=9)
        assert torch.equal(got.view(torch.int32), clean.view(torch.int32)), fill


def test_a_slot_no_run_wrote_is_zero_in_the_stale_replay_and_float_sites_get_nan():
    from tomosar2height_amd import _lib
    with guarded_scratch("record", CPU) as a:
        ws = _lib.workspace(16, "cpu")
        assert bool((ws == 0).all())
        ws[:4] = 7
    with guarded_scratch("stale", CPU, record=a.log):
        again = _lib.workspace(16, "cpu")
        assert again.tolist() == [7] * 4 + [0] * 12 and again.data_ptr() == ws.data_ptr()
    with guarded_scratch("stale", CPU, record=a.log, nan_sites=("test_scratch_guard_cpu.py",)):
        fresh = _lib.workspace(16, "cpu")
        assert bool((fresh == 0xFF).all()) and fresh.data_ptr() != ws.data_ptr()


def test_typed_allocations_are_filled_and_cpu_passes_through_when_not_selected():
    src = torch.zeros(4, 6)
    with guarded_scratch("nan", CPU):
        made = [torch.empty(2, 3), torch.empty_like(src), torch.empty_strided((2, 3), (1, 2)), src.new_empty(5),
                torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)]
    assert all(bool(t.isnan().all()) for t in made)
    with guarded_scratch("nan", ("cuda",)) as g:                    # CPU tensors are not this block's business
        t = torch.empty(4)
        t.fill_(3.0)
    assert g.log == [] and bool((t == 3.0).all())


def test_stale_integers_come_from_the_recorded_run():
    with guarded_scratch("record", CPU) as a:
        idx = torch.empty(4, dtype=torch.int32)
        assert bool((idx == 0).all())
        idx.copy_(torch.tensor([3, 1, 2, 0], dtype=torch.int32))
    with guarded_scratch("stale", CPU, record=a.log):
        again = torch.empty(4, dtype=torch.int32)
        assert again.tolist() == [3, 1, 2, 0] and again.data_ptr() != idx.data_ptr()


def test_patches_are_gone_after_exit_also_after_an_exception():
    from tomosar2height_amd import _lib
    before = (_lib.workspace, torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty,
              "new_empty" in torch.Tensor.__dict__)

    def now():
        return (_lib.workspace, torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty,
                "new_empty" in torch.Tensor.__dict__)

    with guarded_scratch("nan", CPU):
        assert now()[:5] != before[:5]
    assert now() == before
    with pytest.raises(KeyError):
        with guarded_scratch("nan", CPU):
            raise KeyError("boom")
    assert now() == before
    with pytest.raises(ScratchGuardError):
        with guarded_scratch("zero", CPU):
            _launch(torch.ones(2), ws_floats=2, reads=2, overrun=3)
    assert now() == before


def test_stale_run_with_another_size_sequence_fails():
    x = torch.ones(4)
    with guarded_scratch("record", CPU) as a:
        _launch(x, ws_floats=4, reads=4)
    with pytest.raises(ScratchGuardError, match="stale replay"):
        with guarded_scratch("stale", CPU, record=a.log):
            _launch(x, ws_floats=5, reads=4)                        # another size
    with pytest.raises(ScratchGuardError, match="stale replay"):
        with guarded_scratch("stale", CPU, record=a.log):
            pass                                                    # fewer allocations
    with pytest.raises(ScratchGuardError, match="stale replay"):
        with guarded_scratch("stale", CPU, record=a.log):
            _launch(x, ws_floats=4, reads=4)
            torch.empty(1)                                          # one more
    with pytest.raises(ValueError):
        guarded_scratch("stale", CPU)


def test_every_size_query_of_the_sources_is_in_the_case_table():
    """A new ``T2H_API size_t`` query cannot skip the table: each one needs a row where it is positive."""
    import test_scratch_guard_gpu as table
    names = set()
    for path in glob.glob(os.path.join(ROOT, "tomosar2height_amd", "csrc", "*.hip")):
        with open(path) as f:
            names.update(re.findall(r"^T2H_API\s+size_t\s+(\w+)\s*\(", f.read(), flags=re.M))
    assert len(names) >= 38
    positive = {q for case in table.CASES for q, _args, sign in case.queries if sign == ">0"}
    listed = {q for case in table.CASES for q, _args, _sign in case.queries}
    assert not (listed - names), f"the table names queries the sources do not export: {sorted(listed - names)}"
    assert not (names - positive), f"size queries without a guarded case where they are > 0: {sorted(names - positive)}"
    for case in table.CASES:
        assert case.fill in ("nan", "stale") and case.why, case.id
        assert all(sign in (">0", "==0") for _q, _a, sign in case.queries), case.id
    assert len({c.id for c in table.CASES}) == len(table.CASES)


def test_tabled_signs_of_the_size_queries_hold():
    """The queries are pure host functions of the shape: every row's ``> 0`` / ``== 0`` is confirmed without a GPU."""
    import tomosar2height_amd  # noqa: F401
    from tomosar2height_amd import _lib, pointops  # noqa: F401
    from tomosar2height_amd.encoder import hourglass  # noqa: F401
    import test_scratch_guard_gpu as table
    for case in table.CASES:
        for name, args, sign in case.queries:
            size = int(_lib._entry(name)(*args))
            assert (size > 0) == (sign == ">0"), (case.id, name, args, size)


def _standin(filename, name="build"):
    """A function that asks for a raw workspace like a wrapper of the package, compiled under another file name: the harness knows
    a call site by the file and function of the caller's frame.  ``overrun``: bytes written past the end (a host tensor write)."""
    src = (f"def {name}(nbytes, overrun=0):\n"
           "    from tomosar2height_amd import _lib\n"
           "    ws = _lib.workspace(nbytes, 'cpu')\n"
           "    if overrun:\n"
           "        base = ws._base if ws._base is not None else ws\n"
           "        start = ws.storage_offset() + ws.numel()\n"
           "        base[start:start + overrun] = 0\n"
           "    return ws\n")
    scope = {}
    exec(compile(src, filename, "exec"), scope)
    return scope[name]


def test_integer_sites_never_start_from_0xff():
    """A raw workspace asked for from tile.py (the tile builds: sort keys, histograms) is zero under "nan", the recorded run's
    bytes whenever a record is replayed -- also where ``nan_sites`` would make it NaN --, and banded like any other."""
    build = _standin("/somewhere/tomosar2height_amd/tile.py")
    other = _standin("/somewhere/tomosar2height_amd/ops.py")
    with guarded_scratch("nan", CPU) as g:
        ws, plain = build(48), other(48)
        assert bool((ws == 0).all()) and bool((plain == 0xFF).all())
    for _, n, view, buf, off, site in g.log:
        assert "tile.py" in site or "ops.py" in site
        assert view.data_ptr() % 512 == 0 and off >= GUARD and buf.numel() - off - n >= GUARD
        assert bool((buf[:off] == 0xFF).all()) and bool((buf[off + n:] == 0xFF).all())
    with guarded_scratch("record", CPU) as a:
        ws = build(48)
        assert bool((ws == 0).all())
        ws[:5] = torch.arange(1, 6, dtype=torch.uint8)
    for fill, kw in (("stale", {}), ("stale", {"nan_sites": ("tile.py",)}), ("nan", {}), ("zero", {})):
        with guarded_scratch(fill, CPU, record=a.log, **kw) as g:
            again = build(48)
            assert again.tolist() == [1, 2, 3, 4, 5] + [0] * 43, (fill, kw)
        assert g.damaged() == []
    with guarded_scratch("nan", CPU, int_sites=()):                  # (the default set is what makes it an integer site)
        assert bool((build(48) == 0xFF).all())
    with pytest.raises(ScratchGuardError) as e:
        with guarded_scratch("nan", CPU):
            build(48, overrun=1)
    msg = str(e.value)
    assert "tile.py" in msg and "(build)" in msg and "48-byte workspace" in msg and "byte +48" in msg
    with pytest.raises(ScratchGuardError, match="stale replay"):      # the sequence check holds for these sites too
        with guarded_scratch("nan", CPU, record=a.log):
            build(52)


def test_a_workspace_that_outlives_the_block_is_a_fresh_copy_in_the_stale_replay():
    """grid.py's ``SplitWeightCache._get`` keeps its buffer for the weight's lifetime: replaying hands out a NEW banded buffer
    with a copy of the recorded bytes (never the recorded buffer, which may be a live cache entry); 0xFF under "nan"."""
    get = _standin("/somewhere/tomosar2height_amd/grid.py", "_get")
    elsewhere = _standin("/somewhere/tomosar2height_amd/grid.py", "conv3x3_fwd_")
    with guarded_scratch("record", CPU) as a:
        kept, scratch = get(32), elsewhere(32)
        kept[:3] = 9
        scratch[:3] = 4
    with guarded_scratch("stale", CPU, record=a.log) as g:
        mine, again = get(32), elsewhere(32)
        assert mine.tolist() == [9] * 3 + [0] * 29 and mine.data_ptr() != kept.data_ptr()
        assert again.data_ptr() == scratch.data_ptr()
        mine[:] = 1                                                  # the cache updates in place: the recorded bytes stay
    assert kept.tolist() == [9] * 3 + [0] * 29 and g.damaged() == []
    entry = g.log[0]
    assert bool((entry[3][:entry[4]] == 0xFF).all()) and bool((entry[3][entry[4] + 32:] == 0xFF).all())
    with guarded_scratch("nan", CPU, record=a.log):
        assert bool((get(32) == 0xFF).all()) and bool((elsewhere(32) == 0xFF).all())
    with pytest.raises(ScratchGuardError, match="stale replay"):
        with guarded_scratch("stale", CPU, record=a.log):
            get(36)
    with pytest.raises(ScratchGuardError) as e:
        with guarded_scratch("stale", CPU, record=a.log):
            get(32, overrun=2), elsewhere(32)
    assert "grid.py" in str(e.value) and "(_get)" in str(e.value) and "byte +32" in str(e.value)


# device uint8 buffers of the package that are NOT scratch: typed results the caller keeps.  (file, a substring of the allocation)
_UINT8_RESULTS = (
    ("ops.py", "t2h_pool_winner_stride"),       # the max-pool's winner bytes per row: saved for the backward
    ("grid.py", "which = torch.empty("),        # the 2 x 2 max-pool's arg-max plane: saved for the backward
    ("evaluator.py", "out = torch.empty(t.shape"),   # a predicate's 0 / 1 plane: the mask the evaluator keeps
)


def test_every_uint8_device_buffer_of_the_package_is_a_lib_workspace():
    """Raw byte scratch comes from ``_lib.workspace`` alone (what scratch_guard.py bands): no other ``torch.empty`` / ``new_empty``
    of ``torch.uint8`` in the package's Python text, but for the typed results listed above."""
    hits = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tomosar2height_amd", "**", "*.py"), recursive=True)):
        with open(path) as f:
            text = f.read()
        for m in re.finditer(r"(?:torch\.empty|\.new_empty)\(", text):
            depth, end = 1, m.end()
            while depth and end < len(text):                        # the whole call, to its closing parenthesis
                depth += {"(": 1, ")": -1}.get(text[end], 0)
                end += 1
            call = text[text.rfind("\n", 0, m.start()) + 1:end]
            if "uint8" in call:
                hits.append((os.path.relpath(path, os.path.join(ROOT, "tomosar2height_amd")), " ".join(call.split())))
    assert ("_lib.py", "return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)") in hits   # the search finds it
    rest = [h for h in hits if h[0] != "_lib.py" and not any(h[0] == f and key in h[1] for f, key in _UINT8_RESULTS)]
    assert not rest, f"uint8 buffers allocated by hand (use _lib.workspace, or list a typed result): {rest}"
    unused = [a for a in _UINT8_RESULTS if not any(h[0] == a[0] and a[1] in h[1] for h in hits)]
    assert not unused, f"allow-list entries that match nothing: {unused}"
