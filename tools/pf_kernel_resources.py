#!/usr/bin/env python3
"""Before/after table of the particle path's kernels from their device assembly -- no GPU needed.

    for f in pf_legacy pf_auto pf_batch pf_unknown; do
        hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S slam.jl_amd/csrc/$f.hip -o DIR/$f.s
    done                                   # once in a checkout of the parent commit, once in this tree
    python tools/pf_kernel_resources.py BEFORE_DIR AFTER_DIR > profiles/pf_kernel_resources.txt

Per kernel: .vgpr_count, .sgpr_count, .private_segment_fixed_size (scratch) and .group_segment_fixed_size (LDS) of the
metadata block, before -> after, the waves per SIMD the VGPR count allows, and whether the instruction stream is the same
text once comments, labels and symbol names are taken out.  Exit status 1 if a kernel's LDS size changed, its scratch
grew, or its VGPR count crossed a step in waves per SIMD.
"""
import glob
import os
import re
import subprocess
import sys

FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
CXXFILT = "c++filt"


def waves_per_simd(vgprs):
    """gfx950: 512 VGPRs per lane and SIMD, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // max(8, -(-vgprs // 8) * 8))


def kernels_of(path):
    """{mangled name: ({field: value}, [instruction lines])} of one .s file."""
    text = open(path).read()
    meta = {}
    for entry in re.split(r"\n  - \.", text[text.index("amdhsa.kernels:"):])[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", entry, re.M)
        if name:
            meta[name.group(1)] = {f: int(re.search(re.escape(f) + r":\s*(\d+)", entry).group(1)) for f in FIELDS}
    out = {}
    for name, fields in meta.items():
        start = text.index("\n" + name + ":")
        body = text[start:text.index(".Lfunc_end", start)].split("\n")[2:]
        stream = []
        for line in body:
            line = line.split(";")[0].strip()
            if not line or line.endswith(":") or line.startswith("."):
                continue                                       # comments, labels, directives
            line = re.sub(r"\.LBB\d+_(\d+)", r"L\1", line)       # branch targets: the number inside the function stays
            line = re.sub(r"_Z\w+|\b[A-Za-z_]\w*(?=@)", "SYM", line)
            stream.append(re.sub(r"\s+", " ", line))
        out[name] = (fields, stream)
    return out


def main(before_dir, after_dir):
    rows, bad = [], False
    for after_path in sorted(glob.glob(os.path.join(after_dir, "*.s"))):
        unit = os.path.basename(after_path)
        before, after = kernels_of(os.path.join(before_dir, unit)), kernels_of(after_path)
        names = sorted(set(before) | set(after))
        plain = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        for name, shown in zip(names, plain):
            shown = re.sub(r"\(.*$", "", re.sub(r"^(void )?\(anonymous namespace\)::", "", shown))
            if name not in before or name not in after:
                rows.append((unit, shown, "only " + ("after" if name in after else "before"), "", "", "", "", ""))
                bad = True
                continue
            (fb, sb), (fa, sa) = before[name], after[name]
            wb, wa = waves_per_simd(fb[FIELDS[0]]), waves_per_simd(fa[FIELDS[0]])
            if fb[FIELDS[3]] != fa[FIELDS[3]] or fa[FIELDS[2]] > fb[FIELDS[2]] or wa < wb:
                bad = True
            cell = lambda f: str(fb[f]) if fb[f] == fa[f] else f"{fb[f]} -> {fa[f]}"
            same = "identical" if sb == sa else f"differs ({len(sb)} -> {len(sa)} instructions)"
            rows.append((unit[:-2], shown, cell(FIELDS[0]), f"{wb}" if wb == wa else f"{wb} -> {wa}", cell(FIELDS[1]),
                         cell(FIELDS[2]), cell(FIELDS[3]), same))
    head = ("unit", "kernel", "VGPR", "waves/SIMD", "SGPR", "scratch B", "LDS B", "instruction stream")
    width = [max(len(str(r[i])) for r in rows + [head]) for i in range(len(head))]
    for r in [head] + rows:
        print("  ".join(str(c).ljust(w) for c, w in zip(r, width)).rstrip())
    n_same = sum(r[-1] == "identical" for r in rows)
    print(f"\n{len(rows)} kernels, {n_same} with an identical instruction stream, {len(rows) - n_same} that differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
