"""What a header declares, what a shared library exports and how it finds its neighbours: the helpers behind the ABI tests of the
product library (tests/test_abi_cpu.py) and of its companion libraries (tests/test_companions_cpu.py).  Nothing here needs a GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
JULIA = os.path.join(ROOT, "slam.jl_amd", "SLAMHip.jl")


def _code(header):
    """The header's text with its comments taken out."""
    with open(header) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def declared(header):
    """The slam_* symbols a header declares."""
    return set(re.findall(r"\b(slam_[a-z0-9_]+)\s*\(", _code(header)))


def prototypes(header):
    """name -> number of C parameters, of every slam_* prototype in a header."""
    return {name: 0 if params.strip() in ("", "void") else len(params.split(","))
            for name, params in re.findall(r"\b(slam_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _code(header))}


def exported(library):
    """The slam_* text symbols a shared library exports."""
    out = subprocess.run(["nm", "-D", "--defined-only", library], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("slam_")}


def dynamic_section(library):
    """`readelf -d` of a shared library: the libraries it needs and its run path."""
    return subprocess.run(["readelf", "-d", library], capture_output=True, text=True, check=True).stdout


def julia_ccalls(libname="libslamhip"):
    """(symbol, return type, number of argument types) of every `ccall((:symbol, libname), ...)` in SLAMHip.jl."""
    with open(JULIA) as f:
        src = f.read()
    out = []
    for m in re.finditer(r"ccall\(\(:(slam_[a-z0-9_]+),\s*" + re.escape(libname) + r"\),\s*([A-Za-z0-9]+),\s*\(", src):
        i = m.end()                                  # just past the "(" of the argument-type tuple
        depth, j = 1, i
        while depth:
            depth += {"(": 1, ")": -1}.get(src[j], 0)
            j += 1
        body = src[i:j - 1]
        d, parts, cur = 0, [], ""
        for ch in body:                              # split at top-level commas (Ref{Ptr{Cvoid}} has none, tuples might)
            if ch in "({":
                d += 1
            elif ch in ")}":
                d -= 1
            if ch == "," and d == 0:
                parts.append(cur)
                cur = ""
            else:
                cur += ch
        if cur.strip():
            parts.append(cur)
        out.append((m.group(1), m.group(2), len([x for x in parts if x.strip()])))
    return out
