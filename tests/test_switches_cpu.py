"""tomosar2height_amd/switches.py against the sources, on text and imports only: every T2H_* name the package or its library
reads from the environment is a row of the table and is read at its declared owner (a library switch at ONE site in C, with the
row's default), nothing reads the environment beside the table's reader and the library's two helpers, the parser is strict, and
every A/B row is flipped by a GPU test."""
import ast
import glob
import os
import re

import pytest

from tomosar2height_amd import switches
from tomosar2height_amd.switches import SWITCHES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tomosar2height_amd")
NAME = r"T2H_[A-Z0-9_]+"
OWN_READERS = ("switches.py", os.path.join("csrc", "build.py"))        # the table's reader; the build, which also runs stand-alone


def _text(path):
    with open(path) as f:
        return f.read()


def _package_files(*patterns):
    return sorted(p for pat in patterns for p in glob.glob(os.path.join(PKG, "**", pat), recursive=True))


def _rel(path):
    return os.path.relpath(path, PKG)


def _python_reads():
    """{name: {file, ...}} of the ``switches.get("T2H_...")`` calls of the package, and of build.py's own reads."""
    reads = {}
    for p in _package_files("*.py"):
        pattern = r'os\.environ\.get\(\s*"(%s)"' % NAME if _rel(p) == OWN_READERS[1] else r'switches\.get\(\s*"(%s)"' % NAME
        for name in re.findall(pattern, _text(p)):
            reads.setdefault(name, set()).add(_rel(p))
    return reads


def _library_reads():
    """[(name, file, helper, default literal)] of the env_flag / env_ll calls of csrc/*.hip and csrc/*.h."""
    sites = []
    for p in _package_files("*.hip", "*.h"):
        for helper, name, dflt in re.findall(r'\b(env_flag|env_ll)\(\s*"(%s)"\s*,\s*([^)]+?)\s*\)' % NAME, _text(p)):
            sites.append((name, _rel(p), helper, dflt))
    return sites


def test_rows_are_well_formed():
    for name, row in SWITCHES.items():
        assert re.fullmatch(NAME, name) and set(row) <= {"kind", "default", "owner", "doc", "scope", "library", "mirror",
                                                          "covered_by"}, name
        kind = row["kind"]
        assert kind in ("flag", "int", "float", "str") or (isinstance(kind, tuple) and row["default"] in kind), name
        assert row.get("scope", "ab") in ("ab", "lab", "env") and row["doc"] and os.path.exists(os.path.join(PKG, row["owner"])), name
        assert switches.get(name, {}) == row["default"], name
    assert {n for n, r in SWITCHES.items() if r.get("scope") == "lab"} == {"T2H_CACHE_READY", "T2H_POISON_LDS", "T2H_SEAM_SYNC_CHECK"}
    assert {n for n, r in SWITCHES.items() if r.get("scope") == "env"} == {"T2H_LIBRARY", "T2H_ALLOW_LIBRARY_FALLBACK",
                                                                           "T2H_BUILD_JOBS", "T2H_LLVM_BIN"}


def test_every_name_read_is_a_row_read_at_its_owner():
    py, lib = _python_reads(), _library_reads()
    read_at = {n: set(files) for n, files in py.items()}
    for name, path, _, _ in lib:
        read_at.setdefault(name, set()).add(path)
    assert set(read_at) == set(SWITCHES), sorted(set(read_at) ^ set(SWITCHES))
    for name, row in SWITCHES.items():
        want = {row["owner"]} | ({row["mirror"]} if "mirror" in row else set())
        assert read_at[name] == want, f"{name}: read in {sorted(read_at[name])}, declared {sorted(want)}"
        assert "mirror" not in row or row.get("library"), f"{name}: only a library switch has a second reader"


def test_nothing_else_reads_the_environment_for_a_switch():
    for p in _package_files("*.py"):
        if _rel(p) not in OWN_READERS:
            text = _text(p)
            assert not ("os.environ" in text and re.search(NAME, text)), f"{_rel(p)}: reads os.environ beside T2H_ names"
    # build.py's own reads carry the rows' defaults
    for name, dflt in re.findall(r'os\.environ\.get\(\s*"(%s)"\s*,\s*"([^"]*)"\)' % NAME, _text(os.path.join(PKG, OWN_READERS[1]))):
        assert switches.get(name, {name: dflt}) == SWITCHES[name]["default"], name
    # the library: getenv in the two helpers only
    for p in _package_files("*.hip", "*.h", "*.cpp", "*.c"):
        n = len(re.findall(r"\bgetenv\b", _text(p)))
        assert n == (2 if _rel(p) == os.path.join("csrc", "t2h_common.h") else 0), f"{_rel(p)}: {n} getenv"
    common = _text(os.path.join(PKG, "csrc", "t2h_common.h"))
    assert re.search(r"inline bool env_flag\([^)]*\) \{[^}]*getenv\(name\)[^}]*\}", common)
    assert re.search(r"inline long long env_ll\([^)]*\) \{[^}]*getenv\(name\)[^}]*\}", common)


def test_library_reads_match_their_rows():
    sites = _library_reads()
    names = [s[0] for s in sites]
    assert len(names) == len(set(names)), f"read at more than one site in C: {sorted(n for n in set(names) if names.count(n) > 1)}"
    assert set(names) == {n for n, r in SWITCHES.items() if r.get("library")}
    for name, path, helper, dflt in sites:
        row = SWITCHES[name]
        assert path == row["owner"], name
        if helper == "env_flag":
            assert row["kind"] == "flag" and dflt in ("true", "false") and (dflt == "true") is row["default"], (name, dflt)
        else:
            assert row["kind"] == "int" and int(dflt) == row["default"], (name, dflt)


def test_parser():
    get = switches.get
    assert get("T2H_GEMM_BX3", {"T2H_GEMM_BX3": "0"}) is False and get("T2H_GEMM_BX3", {"T2H_GEMM_BX3": "1"}) is True
    assert get("T2H_GEMM_BX3", {}) is True and get("T2H_GEMM_BX3_WGRAD", {}) is False          # unset: the default
    for bad in ("true", "", "2"):
        with pytest.raises(ValueError, match="T2H_OVERLAP_WGRAD"):
            get("T2H_OVERLAP_WGRAD", {"T2H_OVERLAP_WGRAD": bad})
    assert [get("T2H_TRUNK_FUSED", {"T2H_TRUNK_FUSED": v}) for v in ("auto", "1", "0")] == ["auto", "1", "0"]
    with pytest.raises(ValueError, match="T2H_TRUNK_FUSED"):
        get("T2H_TRUNK_FUSED", {"T2H_TRUNK_FUSED": "yes"})
    with pytest.raises(ValueError, match="T2H_CONV_PRECISION"):
        get("T2H_CONV_PRECISION", {"T2H_CONV_PRECISION": "fp16"})
    assert get("T2H_COALESCE_TILES", {"T2H_COALESCE_TILES": "8"}) == 8 and get("T2H_COALESCE_TILES", {}) == 4
    v = get("T2H_GRID_FIRST_MIN_RATIO", {"T2H_GRID_FIRST_MIN_RATIO": "1e6"})
    assert v == 1e6 and isinstance(v, float) and isinstance(get("T2H_GRID_FIRST_MIN_RATIO", {}), float)
    with pytest.raises(ValueError):
        get("T2H_COALESCE_TILES", {"T2H_COALESCE_TILES": "four"})
    assert get("T2H_LIBRARY", {}) is None and get("T2H_LIBRARY", {"T2H_LIBRARY": "/x/lib.so"}) == "/x/lib.so"
    assert get("T2H_FPS_SLICE", {}) is None and get("T2H_FPS_SLICE", {"T2H_FPS_SLICE": "256"}) == 256
    with pytest.raises(KeyError):
        get("T2H_NO_SUCH_SWITCH")


def test_get_reads_the_environment_at_the_call(monkeypatch):
    monkeypatch.delenv("T2H_BATCH_REDUCE", raising=False)
    assert switches.get("T2H_BATCH_REDUCE") is True
    monkeypatch.setenv("T2H_BATCH_REDUCE", "0")
    assert switches.get("T2H_BATCH_REDUCE") is False


def _groups():
    tree = ast.parse(_text(os.path.join(ROOT, "tests", "test_switches.py")))
    return next(ast.literal_eval(n.value) for n in tree.body
                if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "GROUPS")


def test_every_ab_switch_is_flipped_by_a_gpu_test():
    groups = _groups()
    for g, env in groups.items():
        for name, value in env.items():
            assert name in SWITCHES, f"group {g} sets {name}, which nothing reads"
            switches.get(name, env)                                 # every value the groups set parses
    for name, row in SWITCHES.items():
        if row.get("scope", "ab") != "ab":
            continue
        flipped = any(name in env and switches.get(name, env) != row["default"] for env in groups.values())
        if "covered_by" in row:                                     # that file sets it; a literal value counts when it differs from the default
            text = _text(os.path.join(ROOT, row["covered_by"]))
            sets = re.findall(r'(?:setenv|setdefault)\(\s*"%s"\s*,\s*(?:"([^"]*)")?|environ\["%s"\]\s*=\s*(?:"([^"]*)")?' % (name, name), text)
            assert sets, f"{name}: {row['covered_by']} does not set it"
            flipped = flipped or any(switches.get(name, {name: v}) != row["default"] for pair in sets for v in pair if v)
        assert flipped, f"{name}: no group of tests/test_switches.py sets it to a value other than its default"
