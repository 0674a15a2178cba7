#!/usr/bin/env python3
"""Compares two device assemblies of the library (make -C mcl_3dl_amd/csrc device-asm), function by function.

    python scripts/kernel_isa_diff.py [--resources] BASE.s NEW.s

A refactor of the kernels should leave their instruction streams alone; this says where it did not. Each assembly is cut
into its functions; comments and alignment directives are dropped and the .LBB* labels are renumbered per function in order
of appearance (the function's number in the file is part of them), so that two functions compare equal exactly when they
hold the same instructions and directives in the same order. Printed: how many functions are identical, the ones present on
one side only and, for each one that differs, its demangled name, the instruction count before and after and the five
opcodes whose counts changed most. --resources also compares the kernel descriptors (VGPRs, SGPRs, LDS, private segment) of
every kernel, identical stream or not. It compares and counts; it does not look for any particular instruction.
Standard library and c++filt only.
"""
import argparse
import collections
import re
import subprocess
import sys

TYPE_RE = re.compile(r"^\s*\.type\s+([^\s,]+)\s*,\s*@function")
END_RE = re.compile(r"^\.Lfunc_end\d+:")
LABEL_RE = re.compile(r"\.LBB\d+_\d+")
ALIGN_RE = re.compile(r"^\.(p2align|align|balign)\b")
RESOURCES = collections.OrderedDict([
    (".amdhsa_next_free_vgpr", "vgpr"),
    (".amdhsa_next_free_sgpr", "sgpr"),
    (".amdhsa_group_segment_fixed_size", "lds"),
    (".amdhsa_private_segment_fixed_size", "private"),
])


class Function:
    def __init__(self):
        self.lines = []      # normalised: instructions, labels and the directives between them
        self.resources = {}  # short resource name -> the descriptor's value (a string: it may be an expression)

    def opcodes(self):
        return [ln.split()[0] for ln in self.lines if not ln.startswith(".") and not ln.endswith(":")]


def parse_asm(text):
    """{mangled name: Function} of every function the assembly defines."""
    funcs = collections.OrderedDict()
    pending = cur = None
    in_desc = False
    labels = {}
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        m = TYPE_RE.match(line)
        if m:
            pending = m.group(1)
            continue
        if cur is None:
            if pending is not None and line == pending + ":":
                cur, pending, in_desc, labels = Function(), None, False, {}
                funcs[line[:-1]] = cur
            continue
        if END_RE.match(line):
            cur = None
            continue
        if line.startswith(".amdhsa_kernel"):
            in_desc = True
            continue
        if line.startswith(".end_amdhsa_kernel"):
            in_desc = False
            continue
        if in_desc:
            parts = line.split(None, 1)
            if parts[0] in RESOURCES and len(parts) == 2:
                cur.resources[RESOURCES[parts[0]]] = parts[1].strip()
            continue
        if ALIGN_RE.match(line):
            continue
        cur.lines.append(LABEL_RE.sub(lambda mm: labels.setdefault(mm.group(0), ".L%d" % len(labels)), line))
    return funcs


def demangle(names):
    names = list(names)
    if not names:
        return {}
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
        plain = out.splitlines()
        if len(plain) == len(names):
            return dict(zip(names, plain))
    except (OSError, subprocess.CalledProcessError):
        pass
    return {n: n for n in names}


def compare(base, new):
    """base, new: parse_asm() results. Returns a dict: identical (count), total (functions on both sides), only_base,
    only_new (names), differing: [{name, insts: (before, after), opcodes: [(opcode, before, after)] at most five, by |change|}],
    resources: [{name, changes: [(resource, before, after)]}] for every common function whose descriptor values differ."""
    common = [n for n in base if n in new]
    res = {"identical": 0, "total": len(common), "only_base": [n for n in base if n not in new],
           "only_new": [n for n in new if n not in base], "differing": [], "resources": []}
    for n in common:
        b, w = base[n], new[n]
        changes = [(r, b.resources.get(r), w.resources.get(r)) for r in RESOURCES.values()
                   if b.resources.get(r) != w.resources.get(r)]
        if changes:
            res["resources"].append({"name": n, "changes": changes})
        if b.lines == w.lines:
            res["identical"] += 1
            continue
        ob, ow = b.opcodes(), w.opcodes()
        cb, cw = collections.Counter(ob), collections.Counter(ow)
        moved = sorted(((op, cb[op], cw[op]) for op in set(cb) | set(cw) if cb[op] != cw[op]),
                       key=lambda x: (-abs(x[2] - x[1]), x[0]))
        res["differing"].append({"name": n, "insts": (len(ob), len(ow)), "opcodes": moved[:5]})
    return res


def render(res, resources=False):
    names = res["only_base"] + res["only_new"] + [d["name"] for d in res["differing"]] + [r["name"] for r in res["resources"]]
    plain = demangle(names)
    out = ["identical: %d of %d functions present in both" % (res["identical"], res["total"])]
    for key, label in (("only_base", "only in BASE"), ("only_new", "only in NEW")):
        out.append("%s: %d" % (label, len(res[key])))
        out += ["  " + plain[n] for n in res[key]]
    out.append("differing: %d" % len(res["differing"]))
    by_name = {r["name"]: r["changes"] for r in res["resources"]}
    for d in res["differing"]:
        before, after = d["insts"]
        out.append("  " + plain[d["name"]])
        out.append("    instructions %d -> %d (%+d)" % (before, after, after - before))
        if d["opcodes"]:
            out.append("    opcodes      " + ", ".join("%s %d -> %d" % o for o in d["opcodes"]))
        else:
            out.append("    opcodes      same counts: order, operands or registers differ")
        if resources:
            ch = by_name.get(d["name"])
            out.append("    resources    " + (", ".join("%s %s -> %s" % c for c in ch) if ch else "unchanged"))
    if resources:
        rest = [r for r in res["resources"] if r["name"] not in {d["name"] for d in res["differing"]}]
        out.append("descriptors that differ (vgpr, sgpr, lds, private): %d of %d" % (len(res["resources"]), res["total"]))
        for r in rest:
            out.append("  " + plain[r["name"]])
            out.append("    resources    " + ", ".join("%s %s -> %s" % c for c in r["changes"]))
    return "\n".join(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("base")
    ap.add_argument("new")
    ap.add_argument("--resources", action="store_true", help="compare the kernel descriptors' register, LDS and scratch sizes too")
    a = ap.parse_args(argv)
    with open(a.base) as f:
        base = parse_asm(f.read())
    with open(a.new) as f:
        new = parse_asm(f.read())
    print(render(compare(base, new), a.resources))
    return 0


if __name__ == "__main__":
    sys.exit(main())
