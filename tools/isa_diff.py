#!/usr/bin/env python3
"""Is the device code of two source trees the same, kernel by kernel?  (the gate of a "no behaviour change" edit)

    python tools/isa_diff.py TREE_A TREE_B [-DNAME[=VALUE] ...] [-v]

Compiles every device unit (icikendalltau_amd/csrc/*.hip) of both trees to gfx950 assembly with the flags of
_lib.build() plus `-S --cuda-device-only` and compares, for every kernel symbol,
  * its instruction text between the function label and `.Lfunc_end`, with comments and whitespace stripped and the
    labels that carry the function's NUMBER in its module (.LBB<n>_<m>, .Ltmp<n>, .Lfunc_end<n>) renumbered in order
    of appearance -- a kernel may move inside its unit, or to another unit, and still compare equal;
  * its `.amdhsa_kernel` block (registers, LDS, scratch, kernarg layout).
A kernel is matched by its symbol, whichever unit of a tree defines it.  Exit status 1 when a kernel differs, or is
missing or defined twice on either side; 2 when a unit does not compile.  -v prints a unified diff of what differs.
"""
import difflib, glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC"]   # == _lib.build()


def compile_unit(tree, src, defines, out):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
    cmd = [hipcc, *FLAGS, *defines, "-S", "--cuda-device-only", "-I", os.path.join(tree, "include"),
           "-I", os.path.join(tree, "icikendalltau_amd", "csrc"), "-o", out, src]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{res.stdout}{res.stderr}")
    with open(out) as f:
        return f.read()


def kernels_of(asm):
    """{symbol: (normalised instruction lines, .amdhsa_kernel lines)} of one unit's assembly."""
    lines = asm.split("\n")
    res = {}
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", l)
        if not m:
            continue
        sym = m.group(1)
        start = next(k for k in range(i, -1, -1) if lines[k].startswith(sym + ":"))
        hsa_end = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
        end = next(k for k in range(hsa_end, len(lines)) if lines[k].startswith(".Lfunc_end"))
        strip = lambda ls: [t for t in (" ".join(x.split(";")[0].split()) for x in ls) if t]
        ids = {}
        text = [re.sub(r"\.L(BB|tmp|func_end)\d+", lambda mm: ids.setdefault(mm.group(0), f".L{mm.group(1)}#{len(ids)}"), t)
                for t in strip(lines[start + 1:i] + lines[hsa_end + 1:end + 1])]
        res[sym] = (text, strip(lines[i:hsa_end + 1]))
    return res


def tree_kernels(tree, defines, tmp, pool):
    """({symbol: (unit, text, hsa)}, [symbols defined in more than one unit])"""
    units = sorted(glob.glob(os.path.join(tree, "icikendalltau_amd", "csrc", "*.hip")))
    if not units:
        raise RuntimeError(f"no device units under {tree}")
    out = tempfile.mkdtemp(dir=tmp)
    asms = pool.map(lambda u: compile_unit(tree, u, defines, os.path.join(out, os.path.basename(u) + ".s")), units)
    found, dup = {}, []
    for unit, asm in zip(units, asms):
        for sym, (text, hsa) in kernels_of(asm).items():
            if sym in found:
                dup.append(sym)
            found[sym] = (os.path.basename(unit), text, hsa)
    return found, dup


def short(sym):
    try:
        return subprocess.run(["c++filt", "-p", sym], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return sym


def main(argv):
    trees = [a for a in argv if not a.startswith("-")]
    defines = [a for a in argv if a.startswith("-D")]
    verbose = "-v" in argv
    if len(trees) != 2:
        sys.exit(__doc__)
    try:
        with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            (A, dupA), (B, dupB) = (tree_kernels(os.path.abspath(t), defines, tmp, pool) for t in trees)
    except RuntimeError as e:
        print(e, file=sys.stderr)
        return 2
    bad = 0
    per_unit = {}
    for sym in sorted(set(A) | set(B)):
        name = short(sym)
        if sym not in A or sym not in B:
            print(f"MISSING in {trees[0] if sym not in A else trees[1]}: {name}")
            bad += 1
            continue
        (ua, ta, ha), (ub, tb, hb) = A[sym], B[sym]
        same_t, same_h = ta == tb, ha == hb
        per_unit.setdefault(ub, [0, 0])[0 if same_t and same_h else 1] += 1
        where = ua if ua == ub else f"{ua} -> {ub}"
        if same_t and same_h:
            print(f"equal    {name}  [{where}; {len(tb)} lines]")
            continue
        bad += 1
        print(f"DIFFERS  {name}  [{where}]: " + ", ".join(
            w for w, s in ((f"instructions ({len(ta)} -> {len(tb)} lines)", same_t), (".amdhsa_kernel block", same_h)) if not s))
        if verbose:
            for d in difflib.unified_diff(ta + ha, tb + hb, trees[0], trees[1], lineterm="", n=2):
                print("    " + d)
    for side, dup in ((trees[0], dupA), (trees[1], dupB)):
        for sym in dup:
            print(f"DUPLICATE in {side}: {short(sym)}")
            bad += 1
    for unit, (eq, ne) in sorted(per_unit.items()):
        print(f"{unit}: {eq} kernels equal" + (f", {ne} DIFFER" if ne else ""))
    total = sum(eq for eq, _ in per_unit.values())
    print(f"{total} kernels equal, {bad} differing / missing / duplicated" + (f"  (built with {' '.join(defines)})" if defines else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
