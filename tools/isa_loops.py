"""Instruction counts of the loops of one function in a device-only `-S` build (CPU only; see tools/isa_diff.py for how to make the .s):
    python tools/isa_loops.py FILE.s SYMBOL_SUBSTRING [min_lines=40]
A loop is the span from a local label to the last backward branch to it.  For every loop of at least min_lines instruction lines it
prints the VALU (v_*), SALU (s_* without waits, nops and branches), branch, wait, LDS (ds_*) and memory (global_/flat_/scratch_/buffer_)
instruction counts, the number of `v_mov_b32` among the VALU (a register rotation on the back-edge shows up here) and the smallest
`vmcnt` any `s_waitcnt` of the span waits for (0: the loop drains its loads and stores; `-`: it waits for none) of the span WITHOUT
its inner loops (an inner loop -- the drain of the cube sweeps -- runs a data-dependent number of times), the inner loops' own
counts indented below it, and the function's register and scratch figures."""
import re
import sys

VMCNT = re.compile(r"vmcnt\((\d+)\)")


def body_of(path, sym):
    lines, name, on = [], None, False
    foot = {}
    for raw in open(path, errors="replace"):
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", raw)
        if m:
            if on:
                break
            on = sym in m.group(1)
            name = m.group(1) if on else name
            continue
        if not on:
            continue
        s = raw.strip()
        m = re.match(r";\s*(NumVgprs|NumSgprs|NumAgprs|ScratchSize|Occupancy|codeLenInByte|SGPRSpill|VGPRSpill)\w*\s*[:=]\s*(-?\d+)", s)
        if m:
            foot.setdefault(m.group(1), int(m.group(2)))
            continue
        s = s.split(";", 1)[0].strip()
        if not s or (s.startswith(".") and not s.endswith(":")):
            continue
        lines.append(s)
    return name, lines, foot


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "scratch_", "buffer_")):
        return "mem"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")) or op == "s_endpgm":
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    path, sym = sys.argv[1], sys.argv[2]
    min_lines = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    name, L, foot = body_of(path, sym)
    if name is None or not L:
        sys.exit(f"no function matching {sym!r} in {path}")
    label_at = {ln[:-1]: i for i, ln in enumerate(L) if ln.endswith(":")}
    loops = {}
    for i, ln in enumerate(L):
        parts = ln.split()
        if parts and parts[0].startswith(("s_cbranch", "s_branch")) and parts[-1] in label_at and label_at[parts[-1]] < i:
            loops[parts[-1]] = (label_at[parts[-1]], i)            # the last backward branch to the label wins
    spans = []
    for a, b in sorted(loops.values()):                            # a span that straddles the end of an earlier one is no loop: the way back
        if not any(x < a <= y < b for x, y in spans):              # from a block the compiler placed behind the loop it belongs to
            spans.append((a, b))
    print(f"{name}: " + " ".join(f"{k} {v}" for k, v in foot.items()))

    def count(a, b, holes):
        c = dict(valu=0, salu=0, branch=0, wait=0, lds=0, mem=0, other=0, mov=0, vmcnt=None)
        for i in range(a, b + 1):
            if L[i].endswith(":") or any(x <= i <= y for x, y in holes):
                continue
            op = L[i].split()[0]
            c[classify(op)] += 1
            c["mov"] += op.startswith("v_mov_b32")                  # register rotation shows up here (counted within VALU too)
            m = VMCNT.search(L[i]) if op.startswith("s_waitcnt") else None
            if m:                                                  # the smallest count waited for: 0 = the loop drains its loads and stores
                c["vmcnt"] = int(m.group(1)) if c["vmcnt"] is None else min(c["vmcnt"], int(m.group(1)))
        return c

    def rot(c):
        return f"v_mov_b32 {c['mov']} min vmcnt {'-' if c['vmcnt'] is None else c['vmcnt']}"

    for a, b in spans:
        if any(x < a and b < y for x, y in spans):
            continue                                                # inner loops are listed under their parent
        inner = [(x, y) for x, y in spans if a < x and y < b]
        if b - a + 1 < min_lines:
            continue
        c = count(a, b, inner)
        print(f"  loop at line {a}..{b}: VALU {c['valu']} SALU {c['salu']} branch {c['branch']} wait {c['wait']} LDS {c['lds']} mem {c['mem']} other {c['other']} {rot(c)}"
              f"  (VALU + SALU {c['valu'] + c['salu']}, with branches {c['valu'] + c['salu'] + c['branch']}, {len(inner)} inner loops left out)")
        for x, y in inner:
            if any(p < x and y < q for p, q in inner):
                continue
            ci = count(x, y, [])
            print(f"      inner {x}..{y}: VALU {ci['valu']} SALU {ci['salu']} branch {ci['branch']} wait {ci['wait']} LDS {ci['lds']} mem {ci['mem']} {rot(ci)}")
        # the short path of one trip: every wave-uniform forward skip inside the loop (s_cbranch_scc*: the drain test) is taken,
        # exec-dependent skips fall through, forward s_branch is followed
        p = dict(valu=0, salu=0, branch=0, wait=0, lds=0, mem=0, other=0)
        i, skips = a, 0
        while i <= b:
            ln = L[i]
            if ln.endswith(":"):
                i += 1
                continue
            op, tgt = ln.split()[0], ln.split()[-1]
            p[classify(op)] += 1
            fwd = tgt in label_at and i < label_at[tgt] <= b
            if fwd and (op.startswith("s_cbranch_scc") or op == "s_branch"):
                skips += op != "s_branch"
                i = label_at[tgt]
                continue
            i += 1
        print(f"      short path ({skips} uniform skips taken): VALU {p['valu']} SALU {p['salu']} branch {p['branch']} wait {p['wait']} LDS {p['lds']} mem {p['mem']}"
              f"  (VALU + SALU {p['valu'] + p['salu']}, with branches {p['valu'] + p['salu'] + p['branch']})")


if __name__ == "__main__":
    main()
