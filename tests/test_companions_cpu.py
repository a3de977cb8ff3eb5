"""The fifteen side libraries (libslamhip_<name>.so beside libslamhip.so), the parts that need no GPU.  _lib.LIBRARIES
is the one table of them; COMPANIONS (header in include/) and EXTENSIONS (header in include/ext/) are its two halves.  For every
row the header, the ctypes table, the library's exports and the Julia binding name the same symbols with the same number of
arguments, and the library is linked against the product library and exactly the side libraries its row names; no symbol is
declared or exported twice anywhere; and the one loader refuses a foreign SLAMHIP_LIBRARY and names the build command for a
library that was not built.

What is particular to one library (its argument types, constants, exported Julia words, Python methods and null-handle status
codes) stays in that library's own test_<feature>_ref_cpu.py."""
import ctypes
import glob
import itertools
import os
import shutil
import subprocess
import sys

import pytest

from __graft_entry__ import load_package
from tests import abi_surface as ABI

L = load_package()._lib                    # at collection: the parametrisation below is the table itself
PRODUCT_HEADERS = ("slamhip.h", "slamhip_diag.h")
COMPANIONS = ["frame", "join", "evidence", "jc", "path", "copy", "handover", "pfcopy"]
EXTENSIONS = ["factor", "linear", "proposal", "local", "iterated", "fej", "wide"]
# what a side library may need besides the project's own libraries and the HIP runtime
SYSTEM = ("libstdc++", "libm.", "libgcc_s", "libc.", "libdl", "libpthread", "librt", "ld-linux")


def _header(loader):
    return os.path.join(ABI.ROOT, loader.header)


def test_the_tables_list_the_fifteen_libraries_in_the_order_they_were_added():
    assert list(L.COMPANIONS) == COMPANIONS
    assert list(L.EXTENSIONS) == EXTENSIONS
    assert list(L.LIBRARIES) == COMPANIONS + EXTENSIONS
    for name, loader in L.LIBRARIES.items():
        assert loader is getattr(L, f"{name}_lib") and loader.name == name
        assert loader is (L.EXTENSIONS if loader.ext else L.COMPANIONS)[name]
        assert loader.signatures is getattr(L, f"{name.upper()}_SIGNATURES")
        assert loader.path == getattr(L, f"{name.upper()}_LIB_PATH") == os.path.join(os.path.dirname(L.LIB_PATH), f"libslamhip_{name}.so")
        # ext says where the header actually lies
        assert loader.ext is (name in EXTENSIONS)
        assert loader.header == ("include/ext/" if loader.ext else "include/") + f"slamhip_{name}.h"
        assert os.path.isfile(_header(loader)), loader.header
        assert os.path.exists(os.path.join(ABI.INCLUDE, "ext", f"slamhip_{name}.h")) == loader.ext
        assert os.path.exists(os.path.join(ABI.INCLUDE, f"slamhip_{name}.h")) == (not loader.ext)
        assert isinstance(loader.libs, tuple) and all(x in L.LIBRARIES and x != name for x in loader.libs)


@pytest.mark.parametrize("name", list(L.LIBRARIES))
def test_header_ctypes_library_and_julia_name_the_same_surface(name):
    loader = L.LIBRARIES[name]
    sigs = loader.signatures
    # the header, the ctypes table and the library: the same names
    names = ABI.declared(_header(loader))
    assert names and names == set(sigs) == ABI.exported(loader.path), (names, set(sigs), ABI.exported(loader.path))
    # every prototype: as many C parameters as argtypes, and int as the return type of the binding
    protos = ABI.prototypes(_header(loader))
    assert set(protos) == names
    for sym, (res, args) in sigs.items():
        assert protos[sym] == len(args), (sym, protos[sym], len(args))
        assert res is ctypes.c_int, sym
    # it finds the product library beside itself; of the project's libraries it needs that one and exactly the side libraries
    # its row names; beyond them the HIP runtime and the system's, neither torch nor python
    own = {"libslamhip.so"} | {f"libslamhip_{x}.so" for x in loader.libs}
    needed = ABI.dynamic_section(loader.path)
    assert "libslamhip.so" in needed and "$ORIGIN" in needed
    libs = {line.split("[")[1].split("]")[0] for line in needed.splitlines() if "(NEEDED)" in line}
    assert {x for x in libs if x.startswith("libslamhip")} == own, (libs, own)
    assert {x for x in libs if not x.startswith(SYSTEM)} == own | {x for x in libs if x.startswith("libamdhip64")}, libs
    assert any(x.startswith("libamdhip64") for x in libs)
    assert "torch" not in needed and "python" not in needed
    ldd = subprocess.run(["ldd", loader.path], capture_output=True, text=True).stdout
    assert {word for line in ldd.splitlines() for word in line.split()[:1] if word.startswith("libslamhip")} == own, ldd
    assert "libslamhip.so" in ldd and "torch" not in ldd and "python" not in ldd
    # the loader opens it once, with every symbol bound
    lib = loader()
    assert lib is loader() and all(getattr(lib, sym).argtypes == args for sym, (_res, args) in sigs.items())
    # SLAMHip.jl: every name is called as (:name, libslamhip_<name>), with the ctypes table's number of argument types and Cint
    calls = ABI.julia_ccalls(f"libslamhip_{name}")
    assert {c[0] for c in calls} == names
    for sym, ret, nargs in calls:
        assert ret == "Cint" and nargs == len(sigs[sym][1]), (sym, ret, nargs, len(sigs[sym][1]))
    with open(ABI.JULIA) as f:
        src = f.read()
    for sym in names:
        assert f"(:{sym}, libslamhip_{name})" in src
    assert f"SLAMHIP_{name.upper()}_LIB" in src


def test_no_symbol_is_exported_or_declared_twice():
    """The sixteen libraries' export sets are pairwise disjoint, and so are the seventeen headers' declared sets and the sixteen
    ctypes tables: a side library never takes a name of the product library or of another side library.  Every library
    exports what its header (the product library's two headers) declares and its table lists, and include/ and include/ext/ hold
    the table's headers and no other."""
    exports = {"libslamhip": ABI.exported(L.LIB_PATH)}
    exports.update((f"libslamhip_{name}", ABI.exported(c.path)) for name, c in L.LIBRARIES.items())
    headers = {os.path.join("include", h): ABI.declared(os.path.join(ABI.INCLUDE, h)) for h in PRODUCT_HEADERS}
    headers.update((c.header, ABI.declared(_header(c))) for c in L.LIBRARIES.values())
    tables = {"SIGNATURES": set(L.SIGNATURES)}
    tables.update((f"{name.upper()}_SIGNATURES", set(c.signatures)) for name, c in L.LIBRARIES.items())
    assert (len(exports), len(headers), len(tables)) == (16, 17, 16) == (1 + len(L.LIBRARIES), 2 + len(L.LIBRARIES), 1 + len(L.LIBRARIES))
    product = headers["include/slamhip.h"] | headers["include/slamhip_diag.h"]
    assert exports["libslamhip"] == product == tables["SIGNATURES"]
    for name, c in L.LIBRARIES.items():
        assert exports[f"libslamhip_{name}"] == headers[c.header] == tables[f"{name.upper()}_SIGNATURES"], name
    top = [os.path.basename(p) for p in glob.glob(os.path.join(ABI.INCLUDE, "slamhip*.h"))]
    ext = [os.path.basename(p) for p in glob.glob(os.path.join(ABI.INCLUDE, "ext", "slamhip*.h"))]
    assert sorted(top) == sorted(list(PRODUCT_HEADERS) + [f"slamhip_{name}.h" for name in L.COMPANIONS])
    assert sorted(ext) == sorted(f"slamhip_{name}.h" for name in L.EXTENSIONS)
    for sets in (exports, headers, tables):
        assert all(sets.values())
        for a, b in itertools.combinations(sets, 2):
            assert not sets[a] & sets[b], (a, b, sorted(sets[a] & sets[b]))


# ---- the loader's two refusals, each in a child process (SLAMHIP_LIBRARY and the package's directory are read at import) --------
REFUSAL = """
import os, sys
sys.path.insert(0, {root!r})
from __graft_entry__ import load_package
L = load_package()._lib                                        # importing under a foreign SLAMHIP_LIBRARY succeeds
assert L.LIB_PATH == os.environ["SLAMHIP_LIBRARY"]
own = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "libslamhip.so")
for name, loader in L.LIBRARIES.items():
    try:
        loader()
    except ImportError as e:
        for word in ("libslamhip_" + name + ".so", own, L.LIB_PATH, "SLAMHIP_LIBRARY"):
            assert word in str(e), (name, word, str(e))
    else:
        raise SystemExit(name + ": opened although the handles belong to another library")
print("refused", len(L.LIBRARIES))
"""

MISSING = """
import importlib.util, os, sys
d = {copy!r}
spec = importlib.util.spec_from_file_location("slam_copy_without_side_libraries", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
mod = importlib.util.module_from_spec(spec)
sys.modules[spec.name] = mod
spec.loader.exec_module(mod)                                   # importing with only libslamhip.so built succeeds
L = mod._lib
assert L.LIB_PATH == os.path.join(d, "libslamhip.so")
for name, loader in L.LIBRARIES.items():
    assert loader.path == os.path.join(d, "libslamhip_" + name + ".so") and not os.path.exists(loader.path)
    try:
        loader()
    except ImportError as e:
        for word in (loader.path, "is missing", "make -C slam.jl_amd/csrc"):
            assert word in str(e), (name, word, str(e))
    else:
        raise SystemExit(name + ": opened although it is not there")
print("missing", len(L.LIBRARIES))
"""


def _child(script, env):
    res = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    return res.stdout.split()


def test_every_loader_refuses_a_foreign_product_library(tmp_path):
    """SLAMHIP_LIBRARY points at a copy of libslamhip.so: the handles would be that library's, the side libraries are linked
    against the package's own."""
    foreign = str(tmp_path / "libslamhip.so")
    shutil.copy(L.LIB_PATH, foreign)
    assert _child(REFUSAL.format(root=ABI.ROOT), dict(os.environ, SLAMHIP_LIBRARY=foreign)) == ["refused", "15"]


def test_every_loader_names_the_build_command_for_a_library_that_was_not_built(tmp_path):
    """A copy of the package with only libslamhip.so built imports, and each side library is an ImportError at its first use."""
    copy = tmp_path / "pkg"
    copy.mkdir()
    pkgdir = os.path.dirname(os.path.abspath(L.__file__))
    for path in glob.glob(os.path.join(pkgdir, "*.py")) + [os.path.join(pkgdir, "libslamhip.so")]:
        shutil.copy(path, str(copy))
    env = {k: v for k, v in os.environ.items() if k != "SLAMHIP_LIBRARY"}
    assert _child(MISSING.format(copy=str(copy)), env) == ["missing", "15"]
