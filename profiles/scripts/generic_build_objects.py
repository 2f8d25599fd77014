"""Device code of the K0 / K5 build objects, before and after a change of how their kernels are written: profiles/generic_build_objects.txt.

    python profiles/scripts/generic_build_objects.py PARENT_BUILD_DIR THIS_BUILD_DIR [--bench DIR] [--control DIR] > profiles/generic_build_objects.txt

Compares the device listings the Makefile keeps next to each object (*-hip-amdgcn-amd-amdhsa-gfx950.s) of the 18 generic objects,
psnode_capi and psnode_backward.  Only symbol names are normalised: the n-th kernel of a listing becomes KERNEL<n> wherever its mangled
name stands (label, directives, resource symbols, metadata), the per-translation-unit __hip_cuid_<hash> symbol (a hash that takes in the
source path) becomes __hip_cuid_X, and the IR block name a label's comment carries (`; %vector.body774`: the compiler's running number
of a value in the function, not code) is dropped.  Every other comment stays, the resource summaries among them.  Kernels are paired by
their position in the listing.  Everything else is compared as text, line by line.
Per object: the kernel count, per kernel the instruction count and the VGPR / SGPR / scratch / LDS figures of its kernel descriptor on both
sides, and whether the normalised text is identical; if it is not, every differing line.  Exit status 1 if any kernel's figures differ
or any line differs.

--bench DIR: also prints the bench.py lines found in DIR/parent_*.jsonl and DIR/this_*.jsonl (one JSON result per line, as bench.py prints
them), per workload the runs of both sides and whether each of this build's runs lies inside the parent's min .. max.  The runs: the
headline (`bench.py --gpus 1 --steps 20 --warmup 3`) and the four generic lines as calls of their own (`--workload ode01_x20 --method rk4`,
`--workload dae01_zvi16 --method rk4`, and both with `--method euler --train`; `--steps 3 --warmup 2`, as bench.py's --full takes them),
the parent's library through PSNODE_LIB_PATH.
--control DIR: the same table for a session in which both sides ran the parent's library (not counted in the exit status)."""
import difflib
import glob
import json
import os
import re
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
FAMILIES = ["", "_act", "_pre", "_rk", "_sub", "_lin", "_pev", "_ab", "_ms"]
OBJECTS = ["psnode_generic" + f for f in FAMILIES] + ["psnode_generic_bwd" + f for f in FAMILIES] + ["psnode_capi", "psnode_backward"]
FIGURES = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"))


def load(path):
    """-> (normalised text, [(name, {figure: value})] in listing order)"""
    text = open(path).read()
    names = re.findall(r"^\t\.amdhsa_kernel (\S+)$", text, re.M)
    stats = []
    for name in names:
        body = text[text.index("\n" + name + ":"):]
        code = body[:body.index(".Lfunc_end")]
        desc = body[body.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        fig = {"insts": sum(1 for ln in code.split("\n")[1:] if re.match(r"\t[a-z]", ln))}
        for key, directive in FIGURES:
            fig[key] = int(re.search(r"\.amdhsa_" + directive + r" (\d+)", desc).group(1))
        stats.append((name, fig))
    order = sorted(range(len(names)), key=lambda i: -len(names[i]))      # longest first: a name may be the prefix of another
    for i in order:
        text = text.replace(names[i], f"KERNEL{i}")
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)
    text = re.sub(r"[ \t]*; %\S+$", "", text, flags=re.M)      # the IR block a label came from: names the compiler numbers through the function
    return text, stats


def bench_table(d, title):
    runs = {}
    for side in ("parent", "this"):
        for path in sorted(glob.glob(os.path.join(d, side + "_*.jsonl"))):
            for line in open(path):
                line = line.strip()
                if not line.startswith("{"):
                    continue
                r = json.loads(line)
                runs.setdefault(r["metric"], {"parent": [], "this": [], "unit": r.get("unit", "")})[side].append(r["value"])
    ok = True
    print("\n" + title)
    for wl, r in runs.items():
        lo, hi = min(r["parent"]), max(r["parent"])
        inside = all(lo <= v <= hi for v in r["this"])
        ok &= inside
        print(f"  {wl}  [{r['unit']}]")
        print("    parent: " + "  ".join(f"{v:.6g}" for v in r["parent"]) + f"    (min {lo:.6g}, max {hi:.6g})")
        far = max(max(lo - v, v - hi, 0.0) / lo for v in r["this"])
        print("    this:   " + "  ".join(f"{v:.6g}" for v in r["this"]) +
              ("    every run inside the parent's min .. max" if inside else f"    OUTSIDE the parent's min .. max, by up to {100 * far:.2f} %"))
    return ok


def main():
    argv = sys.argv[1:]
    tables = {}
    for opt in ("--bench", "--control"):
        if opt in argv:
            i = argv.index(opt)
            tables[opt] = argv[i + 1]
            del argv[i:i + 2]
    a, b = argv
    bad = 0
    print("Device listings of the K0 / K5 build objects, parent -> this build (profiles/scripts/generic_build_objects.py; kernel symbol names and the")
    print("per-file cuid symbol normalised, IR block names in label comments dropped, nothing else).")
    print("Per kernel: instructions, VGPRs, SGPRs, scratch bytes, static LDS bytes.\n")
    for stem in OBJECTS:
        ta, sa = load(os.path.join(a, stem + SUFFIX))
        tb, sb = load(os.path.join(b, stem + SUFFIX))
        diff = [ln for ln in difflib.unified_diff(ta.split("\n"), tb.split("\n"), "parent", "this", n=0, lineterm="") if not ln.startswith(("---", "+++", "@@"))]
        print(f"{stem}: {len(sa)} kernels -> {len(sb)} kernels, normalised text {'identical' if not diff else 'DIFFERS in %d lines' % len(diff)}")
        bad += len(sa) != len(sb)
        for i in range(max(len(sa), len(sb))):
            fa, fb = (sa[i][1] if i < len(sa) else None), (sb[i][1] if i < len(sb) else None)
            show = lambda f: "  ".join(f"{k} {v}" for k, v in f.items()) if f else "(none)"
            same = fa == fb
            bad += not same
            print(f"  KERNEL{i}  {show(fb)}  {'= parent' if same else '!= parent: ' + show(fa)}  {sb[i][0] if i < len(sb) else sa[i][0]}")
        for ln in diff:
            print("    " + ln)
        bad += len(diff)
    print("\nEVERY OBJECT IDENTICAL" if not bad else f"\n{bad} DIFFERENCES")
    if "--bench" in tables and not bench_table(tables["--bench"], "Speed: bench.py, the parent's library and this build's alternating in one session, P T P T P T P (every run of each side, in the order taken)"):
        bad += 1
    if "--control" in tables:
        bench_table(tables["--control"], "Control: the same, with the parent's library on BOTH sides (one file under two names): what the rule says of two identical libraries")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
