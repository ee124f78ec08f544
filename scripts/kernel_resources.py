"""Resource usage of every kernel of libcrucible_hip.so as the compiler allocated it (-Rpass-analysis=kernel-resource-usage on the
same sources and flags as crucible_amd/csrc/Makefile, every translation unit, remarks merged): allocated VGPRs / SGPRs, scratch
bytes, spill counts, waves per SIMD.  A kernel that two units emit is an error.
rocprofv3's `arch_vgpr_count` halves the allocation on gfx950 (64 for a 128-VGPR kernel); this is the figure bench.py reports.
usage: python scripts/kernel_resources.py > profiles/r03_kernel_resources.json   (CPU only, ~1 min on 8 cores)
EXTRA="-DNAME=VALUE ..." adds flags, as the Makefile's EXTRA does (variant builds of an experiment)."""
import concurrent.futures, json, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
csrc = os.path.join(ROOT, "crucible_amd", "csrc")
units = [os.path.join(csrc, u + ".hip") for u in re.search(r"^UNITS := (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()]
cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
       "-fhip-fp32-correctly-rounded-divide-sqrt", "-fvisibility=hidden", "-Wno-unused-function", "--offload-device-only", "-c",
       "-Rpass-analysis=kernel-resource-usage", "-o", "/dev/null"] + os.environ.get("EXTRA", "").split()
with concurrent.futures.ThreadPoolExecutor(max_workers=12) as pool:
    texts = list(pool.map(lambda src: subprocess.run(cmd + [src], capture_output=True, text=True, cwd=csrc).stderr, units))
out, unit_of = {}, {}
for src, txt in zip(units, texts):
    blocks = re.split(r"remark: [^\n]*Function Name: ", txt)[1:]
    names = [b.split()[0] for b in blocks]
    if not names:
        continue   # a unit without kernels
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    for b, d in zip(blocks, dem):
        def g(k):
            m = re.search(k + r": (\d+)", b)
            return int(m.group(1)) if m else None
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(cr::KernelArgs<\w+>\)$", "", d)
        if d in out:
            sys.exit(f"{d}: emitted by {unit_of[d]} and by {os.path.basename(src)}")
        unit_of[d] = os.path.basename(src)
        out[d] = {"vgprs": g("VGPRs"), "agprs": g("AGPRs"), "sgprs": g("TotalSGPRs"), "scratch_bytes_per_lane": g(r"ScratchSize \[bytes/lane\]"),
                  "sgpr_spills": g("SGPRs Spill"), "vgpr_spills": g("VGPRs Spill"), "waves_per_simd": g(r"Occupancy \[waves/SIMD\]")}
json.dump({"source": "hipcc -Rpass-analysis=kernel-resource-usage, flags of crucible_amd/csrc/Makefile", "kernels": out}, sys.stdout, indent=0, sort_keys=True)
