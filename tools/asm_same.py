#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two gfx950 assembly listings (hipcc --cuda-device-only -S) of the
same source file before and after a refactor.

    tools/asm_same.py OLD.s NEW.s [--alias OLD_NAME=NEW_NAME ...]

Kernels are paired by demangled name without the parameter list, without `(anonymous namespace)::`
and without template arguments of class type (a policy type added by the refactor); --alias
renames a kernel of OLD first.  The instruction stream of a kernel is its lines between the entry
label and the end label with comments and directives dropped, symbol names replaced by SYM<k>
and basic-block labels by L<k> in order of first appearance.  Prints one table row per kernel:
the verdict (same / kernarg offsets / scalar-load order: the same instructions with scalar
loads issued at other places / DIFFERENT / only in one listing), the instruction count, the
differing lines if there are few, and the metadata fields that differ.  Exit status 1 if any
kernel is DIFFERENT or unpaired."""
import argparse
import difflib
import re
import subprocess
import sys

META = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def key_of(demangled, alias):
    s = demangled.replace("(anonymous namespace)::", "")
    s = re.sub(r"^void ", "", s)
    depth, cut = 0, len(s)
    for i, ch in enumerate(s):   # the parameter list starts at the first '(' outside <>
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            cut = i
            break
    s = s[:cut]
    m = re.match(r"(\w+)(?:<(.*)>)?$", s)
    name, targs = m.group(1), m.group(2)
    name = alias.get(name, name)
    if targs is None:
        return name
    keep = [t.strip() for t in targs.split(",") if re.fullmatch(r"\s*(-?\d+|true|false)\s*", t)]
    return f"{name}<{', '.join(keep)}>"


def parse(path):
    """{mangled name: (instruction lines, {metadata field: value})}"""
    lines = open(path).read().split("\n")
    kernels = [m.group(1) for ln in lines if (m := re.match(r"\t\.amdhsa_kernel (\S+)", ln))]
    body = {}
    for k in kernels:
        start = lines.index(next(ln for ln in lines if ln.startswith(k + ":")))
        ins, syms, labels = [], {}, {}
        for ln in lines[start + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            ln = ln.split(";")[0].rstrip()
            if not ln.strip() or (ln.startswith("\t.") and not ln.rstrip().endswith(":")):
                continue
            ln = re.sub(r"_Z\w+", lambda m: syms.setdefault(m.group(0), f"SYM{len(syms)}"), ln)
            ln = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), f"L{len(labels)}"), ln)
            ins.append(" ".join(ln.split()))
        body[k] = ins
    meta, cur = {}, None
    in_meta = False
    for ln in lines:
        if ln.startswith("amdhsa.kernels:"):
            in_meta = True
        elif in_meta and ln.startswith("  - ."):
            cur = {}
        if in_meta and cur is not None:
            m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)", ln)
            if m and m.group(1) in META:
                cur[m.group(1)] = m.group(2)
            if m and m.group(1) == "name":
                meta[m.group(2)] = cur
    return {k: (body[k], meta.get(k, {})) for k in kernels}


def offsets_only(a, b):
    """The differing line pairs if a and b differ only in the offset of scalar kernel-argument loads."""
    if len(a) != len(b):
        return None
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    for x, y in diff:
        mx, my = (re.fullmatch(r"(s_load_dword\w* \S+ s\[\d+:\d+\]), (0x[0-9a-f]+|\d+)", z) for z in (x, y))
        if not (mx and my and mx.group(1) == my.group(1)):
            return None
    return diff


def load_order_only(a, b):
    """The diff if a and b are the same stream apart from where scalar loads are issued."""
    is_load = lambda z: z.startswith("s_load_dword")   # noqa: E731
    if [z for z in a if not is_load(z)] != [z for z in b if not is_load(z)]:
        return None
    if sorted(filter(is_load, a)) != sorted(filter(is_load, b)):
        return None
    return [ln for ln in difflib.unified_diff(a, b, lineterm="", n=1) if not ln.startswith(("---", "+++"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--alias", action="append", default=[])
    args = ap.parse_args()
    alias = dict(a.split("=") for a in args.alias)
    old, new = parse(args.old), parse(args.new)
    dm = demangle(list(old) + list(new))
    ko = {key_of(dm[k], alias): k for k in old}
    kn = {key_of(dm[k], {}): k for k in new}
    bad = False
    print(f"{'kernel':58s} {'verdict':18s} {'instr old/new':>14s}  metadata")
    for key in sorted(set(ko) | set(kn)):
        if key not in ko or key not in kn:
            print(f"{key:58s} only in {'old' if key in ko else 'new'}")
            bad = True
            continue
        (a, ma), (b, mb) = old[ko[key]], new[kn[key]]
        diff = offsets_only(a, b)
        moved = load_order_only(a, b) if diff is None else None
        verdict = "same" if a == b else ("kernarg offsets" if diff is not None else
                                         ("scalar-load order" if moved is not None else "DIFFERENT"))
        bad |= verdict == "DIFFERENT"
        md = ", ".join(f"{f} {ma.get(f)} -> {mb.get(f)}" for f in META if ma.get(f) != mb.get(f)) or "same"
        print(f"{key:58s} {verdict:18s} {len(a):>6d}/{len(b):<7d}  {md}")
        for x, y in diff or []:
            print(f"    {x}   ->   {y}")
        for ln in moved or []:
            print(f"    {ln}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
