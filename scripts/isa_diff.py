"""Do two source trees compile to the same kernels?  Every unit of crucible_amd/csrc/Makefile's UNITS, device only, to assembly
(--offload-device-only -S, the Makefile's flags, as kernel_resources.py compiles them), cut into one text per function -- its
code, its kernel descriptor and the compiler's resource summary --, and the texts compared as text.  Two things are taken out
first, because they name the translation unit and not the kernel: lines with the __hip_cuid_ symbol (a hash of the unit), and the
function's ordinal within its unit in local labels (.LBB12_3 -> .LBB_3).  Prints the demangled name of every kernel whose text
differs, or that only one tree has, and nothing for equal ones; exits 1 on a difference.  The proof a refactor of the kernel
headers needs: profiles/experiments/stage_scene_isa.txt.
usage: python scripts/isa_diff.py PARENT_TREE TREE   (CPU only; a few minutes per tree on 8 cores)
       python scripts/isa_diff.py --keep DIR PARENT_TREE TREE   keeps the .s files under DIR/a and DIR/b, and takes a unit's
       file that is already there as compiled (so a parent is compiled once while the tree changes: delete DIR/b between runs)
EXTRA="-DNAME=VALUE ..." adds flags, as the Makefile's EXTRA does."""
import concurrent.futures, os, re, subprocess, sys, tempfile

FLAGS = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fvisibility=hidden", "-Wno-unused-function", "--offload-device-only", "-S"]


def compile_tree(tree, out, pool):
    csrc = os.path.join(tree, "crucible_amd", "csrc")
    units = re.search(r"^UNITS := (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    os.makedirs(out, exist_ok=True)

    def one(u):
        s = os.path.join(out, u + ".s")
        if not os.path.exists(s):
            r = subprocess.run(FLAGS + os.environ.get("EXTRA", "").split() + ["-o", s + ".tmp", u + ".hip"], capture_output=True, text=True, cwd=csrc)
            if r.returncode:
                sys.exit(f"{tree}: {u}.hip does not compile\n{r.stderr}")
            os.replace(s + ".tmp", s)
        return s
    return [pool.submit(one, u) for u in units]


def functions(paths):
    """{(unit, mangled name): text} over the units' assembly (several units may emit a static device function of one name)"""
    out = {}
    for path in paths:
        unit = os.path.basename(path)[:-2]
        txt = "".join(l for l in open(path) if "__hip_cuid_" not in l)
        txt = txt.split("\t.section\t.AMDGPU.gpr_maximums")[0]
        # a function runs from its .type line to the .section line that opens the next one
        pieces = re.split(r"^\t\.type\t(\S+),@function\n", txt, flags=re.M)
        for name, body in zip(pieces[1::2], pieces[2::2]):
            body = re.split(r"^\t\.section\t\.text\S*\n\t\.(?:protected|globl|weak|hidden)", body, flags=re.M)[0]
            body = re.sub(r"\.L(BB|func_begin|func_end)\d+", r".L\1", body)
            out[unit, name] = body
    return out


def main(argv):
    keep = None
    if argv[:1] == ["--keep"]:
        keep, argv = argv[1], argv[2:]
    if len(argv) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        jobs = [compile_tree(t, os.path.join(keep or tmp, d), pool) for t, d in zip(argv, "ab")]
        a, b = (functions([j.result() for j in js]) for js in jobs)
    differing = sorted(n for n in a.keys() | b.keys() if a.get(n) != b.get(n))
    if differing:
        dem = subprocess.run(["c++filt"] + [name for _, name in differing], capture_output=True, text=True).stdout.splitlines()
        for n, d in zip(differing, dem):
            print(f"{d}   [{n[0]}.hip]" + ("" if n in a and n in b else "   (only in %s)" % (argv[0] if n in a else argv[1])))
    print(f"{len(a)} / {len(b)} functions, {len(differing)} differ", file=sys.stderr)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
