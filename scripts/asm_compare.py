#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 assembly of two source trees (no GPU needed).

    python scripts/asm_compare.py TREE_A TREE_B tdec.hip tdec_mix.hip pdsch.hip

Every file is compiled in both trees with the flags of srslte-emane_amd/csrc/Makefile plus --cuda-device-only -S, the output is split per
function, the lines that differ between any two builds (__hip_cuid_, the function index in local labels) are neutralised, and every
function is reported as `same` or `differs` with both line counts and, for kernels, the resource figures of the code-object metadata.
Exit status 1 on any `differs` and on a function that only one tree has."""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("srslte-emane_amd", "csrc")
FIGURES = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count")


def makefile_flags(csrc):
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    return [var["HIPCC"]] + re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["CXXFLAGS"]).split()


def assemble(tree, name, tmp):
    csrc = os.path.join(os.path.abspath(tree), CSRC)
    out = os.path.join(tmp, name + ".s")
    subprocess.run(makefile_flags(csrc) + ["--cuda-device-only", "-S", name, "-o", out], cwd=csrc, check=True)
    return open(out).read()


def split(asm):
    """-> {function: normalised lines}, {kernel: {figure: value}}"""
    text, _, meta = asm.partition(".amdgpu_metadata")
    funcs, cur, ended = {}, None, False
    for line in text.splitlines():
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur, ended = funcs.setdefault(m.group(1), []), False
        elif ended and re.match(r"\s*\.(text|section\s+\.text)", line):  # the next function's header
            cur = None
        ended = ended or line.startswith(".Lfunc_end")
        if cur is not None and "__hip_cuid_" not in line:
            cur.append(re.sub(r"(\.L[A-Za-z_]+|\bBB)\d+", r"\1#", line))  # .LBB<n>_<m>, .Lfunc_end<n>, "Header=BB<n>_<m>"
    figures = {}
    for entry in re.split(r"\n\s*- \.agpr_count:", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        figures[name] = {f: re.search(re.escape(f) + r":\s+(\d+)", entry).group(1) for f in FIGURES}
    return funcs, figures


def demangle(name):
    try:
        out = subprocess.run(["c++filt", name], stdout=subprocess.PIPE, check=True).stdout.decode().strip()
        return re.sub(r"\(anonymous namespace\)::|^void |\(.*", "", out)
    except (OSError, subprocess.CalledProcessError):
        return name


def main():
    tree_a, tree_b, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        for name in files:
            (fa, ma), (fb, mb) = split(assemble(tree_a, name, ta)), split(assemble(tree_b, name, tb))
            print("## %s" % name)
            for fn in sorted(set(fa) | set(fb)):
                if fn not in fa or fn not in fb:
                    verdict = "missing" if fn in fa else "new"
                else:
                    verdict = "same" if fa[fn] == fb[fn] and ma.get(fn) == mb.get(fn) else "differs"
                bad += verdict != "same"
                lines = "%s / %s lines" % (len(fa[fn]) if fn in fa else "-", len(fb[fn]) if fn in fb else "-")
                figs = " ".join("%s %s/%s" % (f[1:], ma.get(fn, {}).get(f, "-"), mb.get(fn, {}).get(f, "-")) for f in FIGURES) if fn in ma or fn in mb else ""
                print("%-8s %s  %s  %s" % (verdict, demangle(fn), lines, figs))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
