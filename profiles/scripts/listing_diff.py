"""Compare the device listings (*-hip-amdgcn-amd-amdhsa-gfx950.s, kept by the Makefile next to each object) of two builds, kernel by kernel.

    python profiles/scripts/listing_diff.py [--rename REGEX=REPL ...] BUILD_DIR_A BUILD_DIR_B [OBJECT_STEM ...]

Per object: the number of kernels, how many are identical, the names of those that differ and of those only one side has.  A kernel is
identical when its instruction stream, its .amdhsa_* directives, its resource symbols (.set NAME.num_vgpr, ...) and its metadata entry
(kernarg segment size, argument offsets and sizes, LDS, scratch, VGPR / AGPR / SGPR counts) are equal as text.  Normalised before the
comparison: the per-translation-unit __hip_cuid_<hash> symbol (a hash of the source path) and the function index inside local labels
(.LBB<n>_<m>, .Lfunc_end<n>: the position of the kernel in its file) and the listing's comments (they carry the compiler's IR
block names, `; %vector.body3159`, numbered through the whole file; every resource figure they repeat is compared as a directive).  Objects named as OBJECT_STEM (e.g. psnode_generic_bwd) are compared
per kernel; every other object has to be the same file, apart from the cuid.  Exit status 1 if anything differs.

--rename REGEX=REPL (repeatable) rewrites symbol names in the listings of BOTH builds before anything is compared: a kernel whose source moved
into a template with another name (K6's `masked_mse_fast_kernel<D, VT>` -> `loss_fast_kernel<RhoMse, LossDev, D, VT, false>`) is compared
under one neutral name given for its old and its new mangled spelling.  Nothing but the text the regex matches changes."""
import glob
import os
import re
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"


RENAMES = []     # (compiled regex, replacement) from --rename


def norm(text):
    for rx, repl in RENAMES:
        text = rx.sub(repl, text)
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    text = re.sub(r"[ \t]*;.*$", "", text, flags=re.M)       # comments: they carry the compiler's IR block names, numbered through the file
    text = re.sub(r"\n{2,}", "\n", text)
    return text


def kernels(path):
    """{kernel name: (code + descriptor + resource symbols, metadata entry)}"""
    text = norm(open(path).read())
    names = re.findall(r"^\t\.amdhsa_kernel (\S+)$", text, re.M)
    out = {}
    for name in names:
        try:
            start = text.index("\n" + name + ":")
            end = text.index(".Lfunc_end", start)
            tail = text[end:text.index(".section\t.AMDGPU.csdata", end)]
            out[name] = [text[start:end] + tail, None]
        except ValueError:      # a listing without the expected markers never compares equal
            out[name] = [f"<no code found in {path}>", None]
    meta = text[text.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""
    for entry in re.split(r"\n  - (?=\.agpr_count:)", meta)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)$", entry, re.M)
        entry = entry.split("\namdhsa.target:")[0]
        if m and m.group(1) in out:
            out[m.group(1)][1] = entry
    return out


def main():
    argv = sys.argv[1:]
    while argv and argv[0] == "--rename":
        rx, repl = argv[1].split("=", 1)
        RENAMES.append((re.compile(rx), repl))
        argv = argv[2:]
    a, b = argv[0], argv[1]
    per_kernel = set(argv[2:])
    stems = sorted({os.path.basename(p)[:-len(SUFFIX)] for d in (a, b) for p in glob.glob(os.path.join(d, "*" + SUFFIX))})
    bad = 0
    for stem in stems:
        pa, pb = os.path.join(a, stem + SUFFIX), os.path.join(b, stem + SUFFIX)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{stem}: only in {a if os.path.exists(pa) else b}")
            bad += 1
            continue
        ka, kb = kernels(pa), kernels(pb)
        if stem not in per_kernel:
            same = norm(open(pa).read()) == norm(open(pb).read())
            print(f"{stem}: {len(ka)} kernels, whole file {'identical' if same else 'DIFFERS'}")
            bad += not same
            continue
        only = sorted(set(ka) ^ set(kb))
        differ = sorted(n for n in set(ka) & set(kb) if ka[n] != kb[n])
        print(f"{stem}: {len(ka)} kernels / {len(kb)} kernels, {len(set(ka) & set(kb)) - len(differ)} identical"
              f" (instructions, .amdhsa_* directives, resource symbols, metadata), {len(differ)} differ, {len(only)} on one side only")
        for n in differ:
            what = [w for w, i in (("code", 0), ("metadata", 1)) if ka[n][i] != kb[n][i]]
            print(f"    differs ({', '.join(what)}): {n}")
        for n in only:
            print(f"    only in {a if n in ka else b}: {n}")
        bad += len(differ) + len(only)
    print("ALL IDENTICAL" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
