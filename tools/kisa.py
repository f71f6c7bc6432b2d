"""Per-kernel gfx950 instruction-stream comparison of one HIP source in two source trees.

    python tools/kisa.py <source, relative to a tree's root> <tree A> <tree B> [extra hipcc flags...]

Both copies are compiled to device assembly with the CXXFLAGS of the Makefile beside the source
(tree B's), block-label numbers are normalised (.LBB<function>_<n> -> .LBB_<n>: they count the
functions ahead of a kernel), and each kernel's stream of instructions and labels is compared:
IDENT, or the number of differing lines and the first few of them.
"""
import difflib, os, re, subprocess, sys

src, trees, extra = sys.argv[1], sys.argv[2:4], sys.argv[4:]
mk = open(os.path.join(trees[1], os.path.dirname(src), "Makefile")).read()
hipcc, arch = (re.search(r"^%s \?= (.*)$" % v, mk, re.M).group(1) for v in ("HIPCC", "ARCH"))
flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()


def kernels(tree):
    """{kernel symbol: [instruction and label lines]} of tree/src"""
    cmd = [hipcc] + flags + extra + ["-x", "hip", "-S", "--cuda-device-only",
                                                      os.path.basename(src), "-o", "-"]
    asm = subprocess.run(cmd, cwd=os.path.join(tree, os.path.dirname(src)), capture_output=True,
                         text=True, check=True).stdout
    out, cur = {}, None
    for line in asm.splitlines():
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip())
        m = re.match(r"([A-Za-z_]\w*):$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line and (not line.startswith(".") or line.startswith(".LBB_")):
            cur.append(line)
    return {k: v for k, v in out.items() if any(l.startswith("s_endpgm") for l in v)}


def short(sym):  # mangled name without the namespace prefix and the argument list (as kres.py)
    return re.sub(r"^_ZN3gpk(12_GLOBAL__N_1)?\d+|E?vNS_.*$|Ev?PK.*$", "", sym)


a, b = kernels(trees[0]), kernels(trees[1])
for sym in sorted(set(a) | set(b), key=short):
    if sym not in a or sym not in b:
        print(f"{short(sym):34s} only in {trees[0] if sym in a else trees[1]}")
        continue
    n = [sum(not l.endswith(":") for l in k[sym]) for k in (a, b)]
    diff = [l for l in difflib.unified_diff(a[sym], b[sym], lineterm="", n=0) if l[0] in "+-" and l[:3] not in ("+++", "---")]
    print(f"{short(sym):34s} {n[0]:6d} {n[1]:6d}  " + ("IDENT" if not diff else f"{len(diff)} lines differ"))
    for l in diff[:8]:
        print("      " + l)
