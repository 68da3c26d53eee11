"""Compares the gfx950 instruction streams and code-object metadata of the 256x256 GEMM kernels in two sets of hipcc -S outputs.

    python scratch/isa_compare.py --old OLD.s [OLD2.s ...] --new NEW.s [NEW2.s ...]

Kernels are matched by (namespace, kind, EPI): gemm256w4_kernel<E, 0> / <E> is the bf16 / f16 kernel, <E, 1> / <E, 2> and
gemm256w4_split_kernel<E, false / true> the split and the K-sliced split kernel.  Before comparing, assembler comments and the
.loc / .file / .ident lines are dropped, and the mangled kernel symbols, the __hip_cuid_* symbol and the per-function prefix of the block labels (.LBB<n>_) are
replaced by fixed names.
Prints one line per kernel of --new; exit status 1 unless every one is identical to its --old counterpart.
"""
import argparse
import re
import sys

META = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size")
SYM = re.compile(r"_ZN(2ed|4ed16)2g4\d+gemm256w4_(split_)?kernelILi(\d)E(?:L([ib])(\d)E)?EE\w+")


def label(m):
    ns, split, epi, _, second = m.groups()
    kind = "split" if split or second in ("1", "2") and not split else "w4"
    ksliced = (split and second == "1") or (not split and second == "2")
    return f"{'ed16' if ns == '4ed16' else 'ed'}::{kind}<{epi}{', K-sliced' if ksliced else ''}>"


def kernels(path):
    text = SYM.sub(lambda m: label(m).replace(" ", ""), open(path).read())
    text = re.sub(r"__hip_cuid_\w+", "__hip_cuid", text)
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)      # block labels carry the kernel's position in its file
    out, cur = {}, None
    for line in text.splitlines():
        line = line.split(";")[0].rstrip()
        if not line.strip() or re.match(r"\s*\.(loc|file|ident)\b", line):
            continue
        m = re.match(r"^(ed(?:16)?::\w+<[^>]+>):$", line)
        if m:
            cur = out.setdefault(m.group(1), {"ins": [], "meta": {}})
        elif cur is not None:
            cur["ins"].append(line)
            if line.strip() == "s_endpgm":
                cur = None
    name, pending = None, {}
    for line in text.splitlines():       # the metadata item of a kernel starts with .agpr_count, its .name comes later
        if re.match(r"\s*-\s*\.agpr_count:", line):
            name, pending = None, {}
        m = re.match(r"\s*\.name:\s+(\S+)", line)
        if m and m.group(1) in out:
            name = m.group(1)
            out[name]["meta"].update(pending)
        m = re.match(r"\s*(?:-\s*)?\.(\w+):\s+(\d+)\s*$", line)
        if m and m.group(1) in META:
            (out[name]["meta"] if name else pending)[m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    old, new = {}, {}
    for f in a.old:
        old.update(kernels(f))
    for f in a.new:
        new.update(kernels(f))
    bad = 0
    for k in sorted(new):
        o, n = old.get(k), new[k]
        same = o is not None and o["ins"] == n["ins"] and o["meta"] == n["meta"]
        bad += not same
        verdict = "identical" if same else ("NO COUNTERPART" if o is None else "DIFFERENT")
        print(f"{k:28s} {len(n['ins']):6d} lines  {verdict:10s} " + " ".join(f"{m}={n['meta'].get(m)}" for m in META))
    gone = sorted(set(old) - set(new))
    print(f"{len(new)} kernels in --new, {len(new) - bad} identical; in --old only: {', '.join(gone) if gone else 'none'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
