"""Per-function comparison of two builds' device assembly (CPU only; the gate of a refactor that must not change the kernels):
    for f in stainlib_amd/csrc/*.hip; do hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S $f -o DIR/$(basename $f .hip).s; done
once per tree, then
    python tools/isa_diff.py DIR_A DIR_B [--all]
For every function symbol of every .s file both directories hold it compares the instruction lines (comments, directives and
blank lines stripped, local labels renumbered by their order of appearance) and the NumVgprs / NumAgprs / ScratchSize /
Occupancy / codeLenInByte figures of the function's footer.  It prints one `same` count per file (with --all one line per function)
and one row per function that differs: both sets of figures and the number of changed instruction lines (marked when the two
streams are the same instructions in the same order on differently numbered registers).  Exit status 1 if
anything differs or a function exists on one side only."""
import difflib
import os
import re
import sys

FIGS = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "codeLenInByte")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?\b")
REG = re.compile(r"\b[vsa](\d+|\[\d+:\d+\])")


def functions(path):
    """{symbol: (instruction lines, {figure: int})} of one .s file."""
    out, name, body, info = {}, None, [], None
    for raw in open(path, errors="replace"):
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", raw)
        if m:
            name, body, info = m.group(1), [], None
            out[name] = (body, {})
            continue
        if name is None:
            continue
        s = raw.strip()
        if re.match(r";\s*(Kernel|Function) info:", s):
            info = out[name][1]
            continue
        m = re.match(r";\s*(\w+)\s*:\s*(-?\d+)", s) or re.match(r";\s*(\w+)\s*=\s*(-?\d+)", s)
        if info is not None and m and m.group(1) in FIGS:
            info.setdefault(m.group(1), int(m.group(2)))
            if len(info) == len(FIGS):
                name, info = None, None
            continue
        if info is not None:
            continue
        s = s.split(";", 1)[0].strip()                # comments
        if not s or s.startswith(".") and not s.endswith(":") or s == name + ":":
            continue                                   # blank lines, directives, the function's own label
        body.append(s)
    for body, _ in out.values():                       # local labels: numbered by first appearance, so an added function elsewhere
        seen = {}                                      # in the file does not show up as a change
        body[:] = [LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), ln) for ln in body]
    return out


def changed(a, b):
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")


def demangle(names):
    try:
        import subprocess
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except Exception:
        return {n: n for n in names}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    show_all = "--all" in sys.argv
    da, db = args
    fa = {f for f in os.listdir(da) if f.endswith(".s")}
    fb = {f for f in os.listdir(db) if f.endswith(".s")}
    bad = 0
    for f in sorted(fa ^ fb):
        print(f"{f}: only in {da if f in fa else db}")
        bad += 1
    for f in sorted(fa & fb):
        A, B = functions(os.path.join(da, f)), functions(os.path.join(db, f))
        nice = demangle(sorted(set(A) | set(B)))
        same, rows = 0, []
        for n in sorted(set(A) | set(B)):
            if n not in A or n not in B:
                rows.append(f"  only in {'A' if n in A else 'B'}: {nice[n]}")
                continue
            (ia, ga), (ib, gb) = A[n], B[n]
            if ia == ib and ga == gb:
                same += 1
                if show_all:
                    rows.append(f"  same: {nice[n]}")
                continue
            figs = " ".join(f"{k} {ga.get(k, '-')}->{gb.get(k, '-')}" for k in FIGS)
            renamed = [REG.sub("r", ln) for ln in ia] == [REG.sub("r", ln) for ln in ib]      # the same instructions on other registers
            rows.append(f"  DIFF {changed(ia, ib)} of {len(ia)} lines{' (register numbers only)' if renamed else ''} | {figs} | {nice[n]}")
        bad += sum(1 for r in rows if not r.startswith("  same"))
        print(f"{f}: {same} of {len(set(A) | set(B))} functions same")
        for r in rows:
            print(r)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
