"""Compares the gfx950 instruction streams and code-object metadata of every kernel in two sets of hipcc -S outputs.

    python scratch/isa_compare.py --old OLD.s [OLD2.s ...] --new NEW.s [NEW2.s ...]

Kernels are the entries of each file's amdhsa.kernels metadata and are matched by their (mangled) symbol.  A kernel's
instruction stream is everything from its label to its .Lfunc_end label; before comparing, assembler comments and the
.loc / .file / .ident lines are dropped, and the __hip_cuid_* symbol and the per-function prefix of the block labels
(.LBB<n>_) are replaced by fixed names.
Prints one line per kernel of --new; exit status 1 unless every one is identical to its --old counterpart.
"""
import argparse
import re
import subprocess
import sys

META = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size")


def kernels(path):
    text = re.sub(r"__hip_cuid_\w+", "__hip_cuid", open(path).read())
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)      # block labels carry the kernel's position in its file
    out = {}
    for item in re.split(r"\n\s*-\s*\.agpr_count:", text)[1:]:     # one metadata item per kernel, .agpr_count first
        item = ".agpr_count:" + item
        name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M).group(1)
        meta = {k: int(v) for k, v in re.findall(r"^\s*\.(\w+):\s+(\d+)\s*$", item, re.M) if k in META}
        body = re.search(rf"^{re.escape(name)}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S).group(1)
        ins = [ln.split(";")[0].rstrip() for ln in body.splitlines()]
        out[name] = {"ins": [ln for ln in ins if ln.strip() and not re.match(r"\s*\.(loc|file|ident)\b", ln)], "meta": meta}
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, (re.sub(r"^void |\(.*", "", ln.replace("(anonymous namespace)", "{anon}")) for ln in r.stdout.splitlines()))) if r.returncode == 0 else {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    old, new = {}, {}
    for files, into in ((a.old, old), (a.new, new)):
        for f in files:
            k = kernels(f)
            assert not set(k) & set(into), f"{f}: kernel symbols already seen in another file: {sorted(set(k) & set(into))}"
            into.update(k)
    nice = demangle(sorted(set(old) | set(new)))
    bad = 0
    for k in sorted(new, key=nice.get):
        o, n = old.get(k), new[k]
        same = o is not None and o["ins"] == n["ins"] and o["meta"] == n["meta"]
        bad += not same
        verdict = "identical" if same else ("NO COUNTERPART" if o is None else "DIFFERENT")
        print(f"{nice[k]:90s} {len(n['ins']):6d} lines  {verdict:10s} " + " ".join(f"{m}={n['meta'].get(m)}" for m in META))
    gone = sorted(nice[k] for k in set(old) - set(new))
    print(f"{len(old)} kernels in --old, {len(new)} in --new, {len(new) - bad} identical; in --old only: {', '.join(gone) if gone else 'none'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
