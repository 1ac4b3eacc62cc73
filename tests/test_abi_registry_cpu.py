"""CPU (no GPU needed): the one registry of C-ABI signatures (``_lib.declare``) covers every public header exactly, nothing
undeclared can be called whatever the import and load order, and ``_lib.Derived`` refills when a source tensor changes."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from abi_ref import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a child that reaches tomosar2height_amd._lib WITHOUT the package's __init__ (which imports every binding module): the package
# is a bare namespace here, so what has been declared is what the child itself imports
ALONE = (
    "import os, sys, types\n"
    f"root = {ROOT!r}\n"
    "sys.path.insert(0, root)\n"
    "pkg = types.ModuleType('tomosar2height_amd'); pkg.__path__ = [os.path.join(root, 'tomosar2height_amd')]\n"
    "sys.modules['tomosar2height_amd'] = pkg\n"
    "import tomosar2height_amd._lib as _lib\n"
    "assert sorted(_lib._registry) == ['t2h.h'], sorted(_lib._registry)\n")


def run_child(code):
    out = subprocess.run([sys.executable, "-c", ALONE + code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stdout + out.stderr


def registry():
    import tomosar2height_amd  # noqa: F401  (imports every binding module)
    import tomosar2height_amd.encoder.hourglass  # noqa: F401
    import tomosar2height_amd.pointops  # noqa: F401
    from tomosar2height_amd import _lib
    return _lib


def test_registry_headers_are_the_public_headers():
    from tomosar2height_amd.csrc import build
    _lib = registry()
    assert sorted(_lib._registry) == sorted(os.path.basename(h) for h in build.PUBLIC_HEADERS)
    assert len(set(_lib._registry)) == len(build.PUBLIC_HEADERS) == 8


def test_registry_names_are_what_each_header_declares():
    _lib = registry()
    for header, table in _lib._registry.items():
        assert sorted(table) == declared_symbols(header), header


def test_no_name_under_two_headers():
    _lib = registry()
    names = [name for table in _lib._registry.values() for name in table]
    assert len(names) == len(set(names)) == len(_lib._declared)
    assert set(names) == set(_lib._declared)


def test_every_declared_name_is_exported_and_typed_after_load():
    from tomosar2height_amd.csrc import build
    _lib = registry()
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)                      # a second handle: the exports themselves
    lib = _lib.load()
    for header, table in _lib._registry.items():
        for name, (res, args) in table.items():
            assert hasattr(raw, name), f"{name} of {header} is not exported"
            fn = getattr(lib, name)
            assert (fn.restype, list(fn.argtypes)) == (res, list(args)), name


def test_binding_modules_keep_their_tables_and_share_one_load():
    from tomosar2height_amd import cloud_instances, evaluator, instances, interpolate, pointops
    from tomosar2height_amd.encoder import hourglass
    _lib = registry()
    want = {"t2h.h": _lib.SIGNATURES, "t2h_eval.h": evaluator.SIGNATURES, "t2h_inst.h": instances.SIGNATURES,
            "t2h_interp.h": interpolate.SIGNATURES, "t2h_tin.h": interpolate.TIN_SIGNATURES, "t2h_cloud.h": cloud_instances.SIGNATURES,
            "t2h_pnpp.h": pointops.SIGNATURES, "t2h_hg.h": hourglass.SIGNATURES}
    assert _lib._registry == want
    for module in (evaluator, instances, interpolate, cloud_instances, pointops, hourglass):
        assert module.load is _lib.load


def test_an_undeclared_entry_cannot_be_called():
    run_child(
        "p = 1 << 40\n"
        "for attempt in (lambda: _lib.call('t2h_inst_metrics', p, p, 4, p, None),\n"
        "                lambda: _lib.ws_bytes('t2h_inst_label_workspace_bytes', 8, 8)):\n"
        "    try:\n"
        "        attempt()\n"
        "    except _lib.T2HLibraryError as e:\n"
        "        assert 't2h_inst_' in str(e) and 'not declared' in str(e), e\n"
        "    else:\n"
        "        raise AssertionError('an undeclared entry was resolved')\n"
        "assert not _lib._fn_cache and not _lib._ws_cache\n"
        "import tomosar2height_amd.instances\n"
        "assert _lib.ws_bytes('t2h_inst_label_workspace_bytes', 8, 8) > 0\n"
        "print('child ok')\n")


CHECK_TYPED = (
    "from tomosar2height_amd import cloud_instances, evaluator, instances\n"
    "lib = _lib.load()\n"
    "seen = set()\n"
    "for module in (cloud_instances, instances, evaluator):\n"
    "    for name, (res, args) in module.SIGNATURES.items():\n"
    "        fn = getattr(lib, name)\n"
    "        assert (fn.restype, list(fn.argtypes)) == (res, list(args)), name\n"
    "        seen.add(name.split('_')[1])\n"
    "assert seen == {'cloud', 'inst', 'eval'}, seen\n"
    "print('child ok')\n")


@pytest.mark.parametrize("order", ("load_first", "import_first"))
def test_import_order_and_load_order_do_not_matter(order):
    if order == "load_first":
        run_child("lib = _lib.load()\n"
                  "assert lib.t2h_cloud_medians.argtypes is None and lib.t2h_eval_predicate.argtypes is None\n"
                  "import tomosar2height_amd.cloud_instances\n" + CHECK_TYPED)
    else:
        run_child("import tomosar2height_amd.cloud_instances\n"
                  "assert _lib._lib is None\n" + CHECK_TYPED)


def test_a_conflicting_second_declaration_raises():
    _lib = registry()
    before = {h: dict(t) for h, t in _lib._registry.items()}
    _lib.declare("t2h.h", dict(_lib.SIGNATURES))                                  # the same table again: a module reload
    with pytest.raises(_lib.T2HLibraryError, match="t2h_eval_stats"):             # a name another header holds
        _lib.declare("t2h_other.h", {"t2h_eval_stats": (ctypes.c_int, [])})
    with pytest.raises(_lib.T2HLibraryError, match="t2h_eval.h"):                 # the same header with another table
        _lib.declare("t2h_eval.h", {"t2h_eval_more": (ctypes.c_int, [])})
    assert _lib._registry == before and "t2h_eval_more" not in _lib._declared


def test_derived_fills_once_per_version_of_its_sources(monkeypatch):
    from tomosar2height_amd import _lib
    events = []
    monkeypatch.setattr(_lib.Ready, "mark", lambda self: events.append("mark"))   # (both need a device)
    monkeypatch.setattr(_lib.Ready, "wait", lambda self: events.append("wait"))
    a, b = torch.ones(3, requires_grad=True), torch.full((3,), 2.0)
    made = []

    def make():
        assert not torch.is_grad_enabled()
        made.append(1)
        return a * b

    cache = _lib.Derived()
    first = cache.get("k", (a, b), make)
    assert len(made) == 1 and events == ["mark"] and not first.requires_grad
    assert cache.get("k", (a, b), make) is first and len(made) == 1 and events == ["mark", "wait"]
    b.add_(1)                                                                     # bumps b._version
    second = cache.get("k", (a, b), make)
    assert second is not first and len(made) == 2 and events == ["mark", "wait", "mark"] and second.tolist() == [3.0] * 3
    assert cache.get("k", (a, b), make) is second and len(made) == 2
    other = cache.get("other", (a,), lambda: a + 1)                               # keys are independent
    assert other.tolist() == [2.0] * 3 and cache.get("k", (a, b), make) is second and len(made) == 2
    with torch.no_grad():
        a.data = a.data.clone()                                                   # new storage, as Module.to() leaves it
    assert cache.get("k", (a, b), make) is not second and len(made) == 3
